"""GPU suite: progressive source files (SOF2) on the chip -- mjh_decode_prog.hip in front of the pixel, export and entropy-coding
kernels.  The cases are those of test_simt_prog_sources.py (tests/prog_source_cases.py); every expected value comes from the reference at test time and is compared for exact
equality.  The cut and bit-flipped files run on the emulator only; one truncated file in a batch with a good one stays here."""
import pytest

import mozjpeg_amd as M
import prog_source_cases as PC

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not PC.have_tools(), reason="reference cjpeg / djpeg / jpegtran / libjpeg.so.62 or tests/native/coef_dump not built")]


# ---- 1. the three paths -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", PC.NAMES)
def test_coefficients_match_the_reference(src):
    PC.check_coefficients(M, src)


@pytest.mark.parametrize("src", PC.NAMES)
def test_pixels_match_djpeg(src):
    PC.check_pixels(M, src)


@pytest.mark.parametrize("mode", [m for m in PC.PIXEL_MODES if m != "default"])
def test_pixel_options_on_a_progressive_source(mode):
    PC.check_pixels(M, "simple_420", mode)


@pytest.mark.parametrize("sw", PC.RECOMPRESS_SWITCHES)
@pytest.mark.parametrize("src", PC.NAMES)
def test_recompressed_file_matches_jpegtran(src, sw):
    PC.check_recompress(M, src, sw)


def test_incomplete_script_is_read_and_recoded_but_not_turned_into_pixels():
    PC.check_incomplete_script(M)


# ---- 2. batching and the subsequence length -----------------------------------------------------------------------------------------------
def test_eight_files_of_two_scripts_and_both_kinds_in_one_call():
    PC.check_batch_of_eight(M)


def test_subsequence_lengths_16_and_0_give_the_same_bytes():
    PC.check_subsequence_lengths(M)


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------
def test_more_scans_than_the_cap():
    PC.check_too_many_scans(M)


def test_bogus_progressions_are_refused():
    PC.check_bogus_progressions(M)


def test_without_the_keyword_a_progressive_file_is_refused_as_before():
    PC.check_default_refusals(M)


def test_a_transform_with_a_progressive_file_is_refused():
    PC.check_transform_refused(M)


# ---- 4. untrusted input: one file that ends inside its AC refinement, next to a good one ------------------------------------------------
def test_a_truncated_file_next_to_a_good_one():
    assert PC.check_damaged(M, ["end_ac_refine"]) == 1
