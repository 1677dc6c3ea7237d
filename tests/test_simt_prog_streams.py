"""CPU suite: valid progressive files (SOF2) that no libjpeg encoder writes, through decode_coefficients, decode and recompress with
progressive_sources=True, with the kernels of mjh_decode_prog.hip executed by the lock-step wave64 emulator (tools/simt,
SIMT_STRICT), whose device buffers end at unmapped pages.  The cases are tests/prog_stream_cases.py's (files from
tests/jpeg_writer_progressive.py at test time).  The premise of every case -- the writer's expected arrays are what the
reference reads, the reference's programs take the file without a message, the construct the case exists for is in its bytes --
involves no kernel and runs first; then every coefficient array is compared with the writer's, every pixel with the reference's
djpeg and every re-coded byte with its jpegtran, for exact equality.

No case is left to the chip alone (prog_stream_cases.GPU_ONLY is empty): the largest, the 16 512-block file of EOB14 runs, takes
the emulator under a second a path."""
import os
import sys

import pytest

import mozjpeg_amd as M
import prog_stream_cases as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "simt"))

pytestmark = pytest.mark.skipif(not PS.have_tools(), reason="reference cjpeg / djpeg / jpegtran / libjpeg.so.62 or tests/native/coef_dump not built")

EMULATED = [n for n in PS.NAMES if n not in PS.GPU_ONLY]


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


@pytest.fixture
def subseq(monkeypatch):
    def set_(s):
        if s is None:
            monkeypatch.delenv("MJH_DECODE_SUBSEQ", raising=False)
        else:
            monkeypatch.setenv("MJH_DECODE_SUBSEQ", str(s))
    return set_


# ---- 1. the writer against the reference: no kernel ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PS.NAMES)
def test_premise(name):
    PS.check_premise(M, name)


# ---- 2. the three paths -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EMULATED)
def test_coefficients_are_the_writers(simt, name):
    PS.check_coefficients(M, name)


@pytest.mark.parametrize("name", EMULATED)
def test_pixels_match_djpeg(simt, name):
    PS.check_pixels(M, name)


@pytest.mark.parametrize("sw", PS.RECOMPRESS_SWITCHES)
@pytest.mark.parametrize("name", [n for n in PS.RECOMPRESS if n in EMULATED])
def test_recompressed_file_matches_jpegtran(simt, name, sw):
    PS.check_recompress(M, name, sw)


@pytest.mark.parametrize("a,b", [("eob_none", "eob_max"), ("eob_split", "eob_max"), ("marker_noise", "marker_clean")])
def test_files_that_differ_decode_alike(simt, a, b):
    PS.check_same_decode(M, a, b)


# ---- 3. subsequences and batching -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PS.SUBSEQ_CASES))
def test_subsequence_lengths_give_the_same_results(simt, subseq, name):
    PS.check_subseq(M, name, subseq)


def test_sixteen_files_of_every_kind_in_one_call(simt):
    PS.check_mixed_batch(M)
