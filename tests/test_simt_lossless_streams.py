"""CPU suite: lossless files (SOF3) that the reference reads silently and no libjpeg encoder writes, through
decode(lossless_sources=True) with the kernels of mjh_decode_lossless.hip executed by the lock-step wave64 emulator (tools/simt,
SIMT_STRICT), whose device buffers end at unmapped pages.  The cases are tests/lossless_stream_cases.py's (files from
tests/jpeg_writer_lossless.py at test time).  The premise of every case -- the reference's djpeg takes the file without a
message and returns the writer's samples, the construct the case exists for is in its bytes -- involves no kernel and runs first;
then every sample is compared with djpeg's for exact equality.  Beside them run the files of the reference's own cjpeg that the
lists of tests/lossless_decode_cases.py lack (lossless_stream_cases.CJPEG_CASES), through that module's check."""
import os
import sys

import pytest

import mozjpeg_amd as M
import lossless_stream_cases as LS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "simt"))

pytestmark = pytest.mark.skipif(not LS.have_tools(), reason="reference cjpeg / djpeg not built (oracle/_ref)")


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


# ---- 1. the writer against the reference: no kernel ------------------------------------------------------------------------------------
def test_the_case_lists_are_complete():
    LS.check_lists()


@pytest.mark.parametrize("name", LS.NAMES)
def test_premise(name):
    LS.check_premise(name)


# ---- 2. samples == djpeg's --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LS.NAMES)
def test_samples_match_djpeg(simt, name):
    LS.check_decode(M, name)


@pytest.mark.parametrize("c", LS.CJPEG_CASES, ids=LS.LD.case_id)
def test_cjpeg_files_the_older_lists_lack(simt, c):
    LS.LD.check_case(M, c)


@pytest.mark.parametrize("name", LS.MULTI_SCAN)
def test_probe_reports_the_scans_as_written(simt, name):
    LS.check_scans(M, name)


@pytest.mark.parametrize("name", LS.LAYOUT_CASES)
def test_layouts_and_bottom_up(simt, name):
    LS.check_layouts(M, name)


@pytest.mark.parametrize("name", list(LS.REFUSED))
def test_refused_by_the_reference_and_here(simt, name):
    LS.check_refused(M, name)


# ---- 3. synchronisation and batching ------------------------------------------------------------------------------------------------------
def test_a_segment_of_many_subsequences_under_16_bit_codes(simt):
    LS.check_sync_long(M)


def test_four_hand_written_files_in_one_call(simt):
    LS.check_batch(M)
