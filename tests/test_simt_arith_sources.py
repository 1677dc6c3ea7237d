"""CPU suite: arithmetic-coded source files (SOF9, SOF10) through decode_coefficients, decode, decode_planes and recompress with
arithmetic_sources=True, with the kernels -- mjh_decode_arith.hip in front of the existing pixel, export and entropy-coding kernels
-- executed by the lock-step wave64 emulator (tools/simt, SIMT_STRICT), whose device buffers end at unmapped pages.  The cases are
tests/arith_source_cases.py's; every expected value comes from the reference at test time and is compared for exact equality.
No case is left to the chip alone."""
import os
import sys

import pytest

import mozjpeg_amd as M
import arith_source_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "simt"))

pytestmark = pytest.mark.skipif(not AC.have_tools(), reason="reference cjpeg / djpeg / jpegtran / refenc / libjpeg.so.62 or tests/native/coef_dump not built")


@pytest.fixture(scope="module")
def simt():
    """the ctypes layer bound to the emulator's library for this module only"""
    import build_simt
    path = build_simt.build()
    saved = (M.LIB_PATH, M._lib, os.environ.get("SIMT_STRICT"))
    M.LIB_PATH, M._lib = path, None
    os.environ["SIMT_STRICT"] = "1"
    try:
        yield path
    finally:
        M.LIB_PATH, M._lib = saved[:2]
        if saved[2] is None:
            os.environ.pop("SIMT_STRICT", None)
        else:
            os.environ["SIMT_STRICT"] = saved[2]


# ---- 1. coefficients, pixels, planes, files -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", AC.NAMES)
def test_coefficients_match_the_reference(simt, src):
    AC.check_coefficients(M, src)


@pytest.mark.parametrize("src", AC.NAMES)
def test_pixels_match_the_reference(simt, src):
    AC.check_pixels(M, src)


@pytest.mark.parametrize("src", AC.OPTION_SOURCES)
def test_scale_fast_dct_rgb565_and_bottom_up(simt, src):
    AC.check_pixel_options(M, src)


@pytest.mark.parametrize("src", AC.PLANE_SOURCES)
def test_planes_match_the_reference(simt, src):
    AC.check_planes(M, src)


@pytest.mark.parametrize("sw", list(AC.RECOMPRESS))
@pytest.mark.parametrize("src", AC.THREE)
def test_recompressed_file_matches_jpegtran(simt, src, sw):
    AC.check_recompress(M, src, sw)


def test_markers_are_copied(simt):
    AC.check_marker_copy(M)


def test_huffman_and_arithmetic_files_of_both_kinds_in_one_call(simt):
    AC.check_mixed_batch(M)


# ---- 2. damaged data (the emulator's device buffers end at unmapped pages) -----------------------------------------------------------------
def test_a_bad_arithmetic_code_damages_its_file_alone(simt):
    AC.check_bad_code_in_a_batch(M)


def test_entropy_data_cut_short_decodes_as_in_the_reference(simt):
    AC.check_truncated(M)


# ---- 3. refusals, defaults, probing -----------------------------------------------------------------------------------------------------
def test_refusals_and_the_words_of_before_without_the_flag(simt):
    AC.check_refusals(M)


def test_incomplete_script_is_read_and_recoded_but_not_turned_into_pixels(simt):
    AC.check_incomplete_script(M)


def test_probe_reports_file_type_tables_and_conditioning():
    AC.check_probe(M)
