"""GPU (-m gpu): the optimal-table kernel (gen_table_body of mjh_kernels.hip) and the forced flush of buffered correction bits
(mjh_prog.hip) under dictated symbol histograms, on the chip.  The families of test_simt_hist.py (tests/hist_cases.py); every
expected byte comes from the reference's jpegtran / cjpeg (oracle/_ref), run at test time, and equality is exact."""
import pytest

import mozjpeg_amd as M
import hist_cases as HC
import stream_cases as SC

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not HC.have_tools(), reason="reference cjpeg / jpegtran / djpeg not built (oracle/_ref)")]


# ---- family A: AC histograms through re-compression ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HC.A_NAMES)
def test_ac_premise(name):
    HC.check_a_premise(M, name)


@pytest.mark.parametrize("name,sw", HC.A_PAIRS, ids=["%s-%s" % p for p in HC.A_PAIRS])
def test_ac_transcode_matches_jpegtran(name, sw):
    HC.check_transcode(M, HC.a_case(name).c, sw)


@pytest.mark.parametrize("name", HC.A_NAMES)
def test_ac_coefficients_are_the_writers(name):
    SC.check_coefficients(M, HC.a_case(name).c)


@pytest.mark.parametrize("sw", HC.BATCH_CODINGS)
def test_batch_distinct_tables(sw):
    HC.check_batch(M, sw)


# ---- family B: lossless category histograms ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HC.B_NAMES)
def test_lossless_premise(name):
    HC.check_b_premise(M, name)


@pytest.mark.parametrize("name", HC.B_NAMES)
def test_lossless_matches_cjpeg(name):
    HC.check_b_encode(M, name)


# ---- family C: forced flush of buffered correction bits -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HC.C_NAMES)
def test_flush_premise(name):
    HC.check_c_premise(M, name)


@pytest.mark.parametrize("name,sw", HC.C_PAIRS, ids=["%s-%s" % p for p in HC.C_PAIRS])
def test_flush_transcode_matches_jpegtran(name, sw):
    HC.check_transcode(M, HC.c_case(name), sw)


@pytest.mark.parametrize("name", HC.C_NAMES)
def test_flush_coefficients_are_the_writers(name):
    SC.check_coefficients(M, HC.c_case(name))
