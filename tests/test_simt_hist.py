"""CPU suite: the optimal-table kernel (gen_table_body of mjh_kernels.hip, through k_gen_tables and k_gen_tables_list) and the
forced flush of buffered correction bits (mjh_prog.hip: the parallel chain and the in-order walk) under DICTATED symbol histograms,
executed by the lock-step wave64 emulator (tools/simt, SIMT_STRICT).  The inputs come from tests/hist_cases.py at test time; every
expected byte comes from the reference's jpegtran / cjpeg, run at test time, and equality is exact.  Every case first proves, from
the reference's files and from restatements of jchuff.c / jcphuff.c, that the branch it exists for runs (test_*_premise)."""
import os
import sys

import pytest

import mozjpeg_amd as M
import hist_cases as HC
import stream_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "simt"))

pytestmark = pytest.mark.skipif(not HC.have_tools(), reason="reference cjpeg / jpegtran / djpeg not built (oracle/_ref)")


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


# ---- family A: AC histograms through re-compression ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HC.A_NAMES)
def test_ac_premise(simt, name):
    HC.check_a_premise(M, name)


@pytest.mark.parametrize("name,sw", HC.A_PAIRS, ids=["%s-%s" % p for p in HC.A_PAIRS])
def test_ac_transcode_matches_jpegtran(simt, name, sw):
    HC.check_transcode(M, HC.a_case(name).c, sw)


@pytest.mark.parametrize("name", HC.A_NAMES)
def test_ac_coefficients_are_the_writers(simt, name):
    SC.check_coefficients(M, HC.a_case(name).c)


@pytest.mark.parametrize("sw", HC.BATCH_CODINGS)
def test_batch_distinct_tables(simt, sw):
    HC.check_batch(M, sw)


# ---- family B: lossless category histograms ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HC.B_NAMES)
def test_lossless_premise(simt, name):
    HC.check_b_premise(M, name)


@pytest.mark.parametrize("name", HC.B_NAMES)
def test_lossless_matches_cjpeg(simt, name):
    HC.check_b_encode(M, name)


# ---- family C: forced flush of buffered correction bits -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HC.C_NAMES)
def test_flush_premise(simt, name):
    HC.check_c_premise(M, name)


@pytest.mark.parametrize("name,sw", HC.C_PAIRS, ids=["%s-%s" % p for p in HC.C_PAIRS])
def test_flush_transcode_matches_jpegtran(simt, name, sw):
    HC.check_transcode(M, HC.c_case(name), sw)


@pytest.mark.parametrize("name", HC.C_NAMES)
def test_flush_coefficients_are_the_writers(simt, name):
    SC.check_coefficients(M, HC.c_case(name))
