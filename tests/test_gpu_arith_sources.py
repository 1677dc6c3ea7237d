"""GPU suite: arithmetic-coded source files (SOF9, SOF10) on the chip -- mjh_decode_arith.hip in front of the pixel, export and
entropy-coding kernels.  The case list is that of test_simt_arith_sources.py (tests/arith_source_cases.py); every expected value
comes from the reference at test time and is compared for exact equality.  Nothing here is built to provoke a fault: the damaged
files are data errors that the kernel survives (every segment read is bounded by the segment's length)."""
import pytest

import mozjpeg_amd as M
import arith_source_cases as AC

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not AC.have_tools(), reason="reference cjpeg / djpeg / jpegtran / refenc / libjpeg.so.62 or tests/native/coef_dump not built")]


# ---- 1. coefficients, pixels, planes, files -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", AC.NAMES)
def test_coefficients_match_the_reference(src):
    AC.check_coefficients(M, src)


@pytest.mark.parametrize("src", AC.NAMES)
def test_pixels_match_the_reference(src):
    AC.check_pixels(M, src)


@pytest.mark.parametrize("src", AC.OPTION_SOURCES)
def test_scale_fast_dct_rgb565_and_bottom_up(src):
    AC.check_pixel_options(M, src)


@pytest.mark.parametrize("src", AC.PLANE_SOURCES)
def test_planes_match_the_reference(src):
    AC.check_planes(M, src)


@pytest.mark.parametrize("sw", list(AC.RECOMPRESS))
@pytest.mark.parametrize("src", AC.THREE)
def test_recompressed_file_matches_jpegtran(src, sw):
    AC.check_recompress(M, src, sw)


def test_markers_are_copied():
    AC.check_marker_copy(M)


def test_huffman_and_arithmetic_files_of_both_kinds_in_one_call():
    AC.check_mixed_batch(M)


# ---- 2. damaged data ----------------------------------------------------------------------------------------------------------------------
def test_a_bad_arithmetic_code_damages_its_file_alone():
    AC.check_bad_code_in_a_batch(M)


def test_entropy_data_cut_short_decodes_as_in_the_reference():
    AC.check_truncated(M)


# ---- 3. refusals, defaults, probing -----------------------------------------------------------------------------------------------------
def test_refusals_and_the_words_of_before_without_the_flag():
    AC.check_refusals(M)


def test_incomplete_script_is_read_and_recoded_but_not_turned_into_pixels():
    AC.check_incomplete_script(M)


def test_probe_reports_file_type_tables_and_conditioning():
    AC.check_probe(M)
