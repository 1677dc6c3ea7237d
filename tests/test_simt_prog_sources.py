"""CPU suite: progressive source files (SOF2) through decode_coefficients, decode and recompress with progressive_sources=True, with
the kernels -- mjh_decode_prog.hip in front of the existing pixel, export and entropy-coding kernels -- executed by the lock-step
wave64 emulator (tools/simt, SIMT_STRICT), whose device buffers end at unmapped pages.  The cases are tests/prog_source_cases.py's;
every expected value comes from the reference at test time and is compared for exact equality.

No case is left to the chip alone (prog_source_cases.GPU_ONLY is empty): the largest, the flat 2048 x 1032 image, takes the emulator
about a second."""
import os
import sys

import pytest

import mozjpeg_amd as M
import prog_source_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "simt"))

pytestmark = pytest.mark.skipif(not PC.have_tools(), reason="reference cjpeg / djpeg / jpegtran / libjpeg.so.62 or tests/native/coef_dump not built")

EMULATED = [n for n in PC.NAMES if n not in PC.GPU_ONLY]


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


# ---- 1. the three paths -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", EMULATED)
def test_coefficients_match_the_reference(simt, src):
    PC.check_coefficients(M, src)


@pytest.mark.parametrize("src", EMULATED)
def test_pixels_match_djpeg(simt, src):
    PC.check_pixels(M, src)


@pytest.mark.parametrize("mode", [m for m in PC.PIXEL_MODES if m != "default"])
def test_pixel_options_on_a_progressive_source(simt, mode):
    PC.check_pixels(M, "simple_420", mode)


@pytest.mark.parametrize("sw", PC.RECOMPRESS_SWITCHES)
@pytest.mark.parametrize("src", EMULATED)
def test_recompressed_file_matches_jpegtran(simt, src, sw):
    PC.check_recompress(M, src, sw)


def test_incomplete_script_is_read_and_recoded_but_not_turned_into_pixels(simt):
    PC.check_incomplete_script(M)


# ---- 2. batching and the subsequence length -----------------------------------------------------------------------------------------------
def test_eight_files_of_two_scripts_and_both_kinds_in_one_call(simt):
    PC.check_batch_of_eight(M)


def test_subsequence_lengths_16_and_0_give_the_same_bytes(simt):
    PC.check_subsequence_lengths(M)


# ---- 3. the marker walk -----------------------------------------------------------------------------------------------------------------
def test_prog_scans_are_the_script():
    PC.check_prog_scans(M)


def test_more_scans_than_the_cap(simt):
    PC.check_too_many_scans(M)


def test_bogus_progressions_are_refused(simt):
    PC.check_bogus_progressions(M)


def test_without_the_keyword_a_progressive_file_is_refused_as_before(simt):
    PC.check_default_refusals(M)


def test_a_transform_with_a_progressive_file_is_refused(simt):
    PC.check_transform_refused(M)


# ---- 4. untrusted input (the emulator's device buffers end at unmapped pages) -----------------------------------------------------------
def test_damaged_files_get_a_status_and_the_good_file_its_arrays(simt):
    assert PC.check_damaged(M) >= 4          # the four files that end inside a scan or lack DC refinement bits cannot decode
