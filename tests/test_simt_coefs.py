"""CPU suite: reading DCT coefficients (mjh_decode_opts.raw_coefs, jpeg_read_coefficients of the stand-alone libjpeg.so.62, the
reference's unchanged jpegtran on that library alone) with the kernels -- the Huffman decoder of mjh_decode.hip and k_export_coefs of
mjh_kernels.hip -- executed by the lock-step wave64 emulator (tools/simt, SIMT_STRICT), whose device buffers end at unmapped pages.
Every expected value comes from the reference at test time (tests/coef_cases.py); comparison is exact equality."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import mozjpeg_amd as M
import coef_cases as CC
import djpeg_cases as DJ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "simt"))

pytestmark = pytest.mark.skipif(not CC.have_tools(), reason="reference jpegtran / libjpeg.so.62 or tests/native/coef_dump not built")


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


@pytest.fixture(scope="module")
def R():
    """the stand-alone libjpeg.so.62 next to the emulator build of libmozjpeg_hip.so"""
    import fuzz_cjpeg
    return DJ.Runner(os.path.join(fuzz_cjpeg.dropin_dir(), "standalone"), env={"SIMT_STRICT": "1"})


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", CC.SOURCES)
def test_arrays_match_the_reference(simt, src):
    CC.check_parity(M, src)


@pytest.mark.parametrize("src", CC.SOURCES)
def test_coef_dump_on_the_standalone_library(R, src):
    CC.check_dump_parity(R, src)


# ---- 2. batching --------------------------------------------------------------------------------------------------------------------
def test_mixed_batch_keeps_order(simt):
    CC.check_mixed_batch(M)


def test_alternating_calls(simt):
    CC.check_alternating_calls(M)


def test_damaged_file_leaves_nothing_of_the_batch_before(simt):
    """the emulator's device memory is the process's own: the arrays behind coefficients_device() are read in place.  The damaged
    file's slot is zeros (not the batch before), the good file's slot is the reference's, the padding columns are zeros."""
    enc = CC.check_stale_buffer(M)
    ref = CC.reference("revert")
    for c in range(3):
        base, stride, bpr, hib, wib = enc.coefficients_device(c)
        assert stride == hib * bpr * 128
        got = np.frombuffer(C.string_at(base, 2 * stride), np.int16).reshape(2, hib, bpr, 64)
        assert not got[0].any()
        assert np.array_equal(got[1][:, :wib], ref[c]) and not got[1][:, wib:].any()
    enc.close()


# ---- 3. round trip ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,sw", CC.ROUND_TRIP, ids=["%s-%s" % p for p in CC.ROUND_TRIP])
def test_round_trip(simt, src, sw):
    CC.check_round_trip(M, src, sw)


def test_values_beyond_1023_are_the_encoders_to_refuse(simt):
    CC.check_big_ac_is_refused_by_the_encoder(M)


# ---- 4. the unchanged jpegtran ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CC.JPEGTRAN_CASES))
def test_unchanged_jpegtran(R, case):
    CC.check_jpegtran(R, case)


def test_jpegtran_refuses_a_progressive_source(R):
    CC.check_jpegtran_refuses_progressive(R)


# ---- 5. API scenarios -----------------------------------------------------------------------------------------------------------------
def test_two_files_through_one_object(R):
    CC.check_two_files(R)


def test_tables_only_then_abbreviated_image(R):
    CC.check_abbreviated(R)


def test_read_coefficients_after_start_decompress(R):
    CC.check_bad_state(R)


def test_abort_then_reuse(R):
    CC.check_abort_then_reuse(R)


def test_client_edits_the_arrays_and_writes_them(R):
    CC.check_zero_ac_and_write(R)


# ---- 6. untrusted input (the emulator's device buffers end at unmapped pages) -----------------------------------------------------------
def test_truncated_files_fail(simt):
    assert CC.check_truncated(M) > 20


def test_bit_flips_read_as_the_reference_or_fail(simt):
    CC.check_bit_flips(M)
