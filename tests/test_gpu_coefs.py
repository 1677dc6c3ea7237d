"""GPU suite: reading DCT coefficients on the chip -- mjh_decode_opts.raw_coefs and k_export_coefs, the coefficients
staying in HBM on their way into the entropy coder, jpeg_read_coefficients of the stand-alone libjpeg.so.62 and the reference's
unchanged jpegtran on that library alone.  The cases are those of test_simt_coefs.py (tests/coef_cases.py); every expected value comes
from the reference at test time (tests/native/coef_dump and jpegtran on oracle/_ref) and is compared for exact equality.  The
truncated and bit-flipped files run on the emulator only; one damaged file stays here, as in test_gpu_decode.py."""
import functools
import os

import numpy as np
import pytest

import mozjpeg_amd as M
import coef_cases as CC
import djpeg_cases as DJ
import transcode_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STANDALONE_DIR = os.path.join(ROOT, "mozjpeg_amd", "standalone")

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not (CC.have_tools() and os.path.exists(os.path.join(STANDALONE_DIR, "libjpeg.so.62"))),
                                 reason="reference jpegtran / libjpeg.so.62, tests/native/coef_dump or the stand-alone library not built")]


@pytest.fixture(scope="module")
def R():
    return DJ.Runner(STANDALONE_DIR)


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", CC.SOURCES)
def test_arrays_match_the_reference(src):
    CC.check_parity(M, src)


@pytest.mark.parametrize("src", CC.SOURCES)
def test_coef_dump_on_the_standalone_library(R, src):
    CC.check_dump_parity(R, src)


# ---- 2. batching --------------------------------------------------------------------------------------------------------------------
def test_mixed_batch_keeps_order():
    CC.check_mixed_batch(M)


def test_alternating_calls():
    CC.check_alternating_calls(M)


class _DeviceView:
    """the encoder's coefficient arrays as an object torch can wrap without a copy"""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = dict(shape=shape, strides=None, typestr="<i2", data=(ptr, False), version=2)


def _device_tensors(enc, n):
    import torch
    out = []
    for c in range(enc.params.num_components):
        base, stride, bpr, hib, wib = enc.coefficients_device(c)
        assert stride == hib * bpr * 128 and bpr >= wib
        t = torch.as_tensor(_DeviceView(base, (n, hib, bpr, 64)), device="cuda:0")
        assert t.is_cuda and t.data_ptr() == base and t.dtype == torch.int16 and t.is_contiguous()
        out.append(t)
    return out


def test_damaged_file_leaves_nothing_of_the_batch_before_torch():
    """the device arrays after a batch with a damaged file: its slot is zeros (not the batch before), the good file's slot is the
    reference's, the padding columns are zeros"""
    enc = CC.check_stale_buffer(M)
    with pytest.raises(M.MjhError):
        enc.wait_decode()
    ref = CC.reference("revert")
    for c, t in enumerate(_device_tensors(enc, 2)):
        got = t.cpu().numpy()
        wib = ref[c].shape[1]
        assert not got[0].any()
        assert np.array_equal(got[1][:, :wib], ref[c]) and not got[1][:, wib:].any()
    enc.close()


def test_profiling_reports_the_export_kernel():
    CC.check_profiling(M)


# ---- 3. round trip ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,sw", CC.ROUND_TRIP, ids=["%s-%s" % p for p in CC.ROUND_TRIP])
def test_round_trip(src, sw):
    CC.check_round_trip(M, src, sw)


def test_values_beyond_1023_are_the_encoders_to_refuse():
    CC.check_big_ac_is_refused_by_the_encoder(M)


@pytest.mark.parametrize("src,sw", [("revert", "revert_opt"), ("s_mixed", "progressive"), ("gray_r5b", "revert_restart2"), ("scans3_2x2_r2", "revert")],
                         ids=lambda v: v)
def test_round_trip_without_leaving_hbm_torch(src, sw):
    """coefficients_device() wrapped as torch tensors goes into encode_coefficients_tensors: on the encoder that decoded, and on a
    second one; two files per call"""
    import torch
    files = [TC.source(src), TC.source(src)]
    ref = TC.reference(src, sw)
    kw = TC.SWITCHES[sw][0]
    enc = M.Encoder(M.params_from_jpeg(files[0], **kw), max_batch=2)
    enc.submit_decode(files, coefficients=True)
    enc.wait_decode()
    tensors = _device_tensors(enc, 2)
    other = M.Encoder(M.params_from_jpeg(files[0], **kw), max_batch=2)
    other.encode_coefficients_tensors(tensors)
    assert [other.get_jpeg(i) for i in range(2)] == [ref, ref]
    other.close()
    enc.encode_coefficients_tensors(tensors)            # the arrays are a buffer of their own: the encoder's planes are free to be written
    assert [enc.get_jpeg(i) for i in range(2)] == [ref, ref]
    torch.cuda.synchronize()
    enc.close()


# ---- 4. the unchanged jpegtran ------------------------------------------------------------------------------------------------------
def test_only_the_standalone_library_is_mapped(R, tmp_path):
    """the loader's own trace names every object it maps: this libjpeg.so.62, never the reference's"""
    inp, outp = str(tmp_path / "in.jpg"), str(tmp_path / "out.jpg")
    with open(inp, "wb") as f:
        f.write(CC.source("revert"))
    r = R.run(True, [TC.JPEGTRAN, "-copy", "none", "-outfile", outp, inp], env={"LD_DEBUG": "libs"})
    assert r.returncode == 0
    loaded = [ln.split("trying file=")[1] for ln in r.stderr.decode(errors="replace").splitlines() if "trying file=" in ln and "libjpeg" in ln]
    assert loaded and all(os.path.realpath(p.strip()).startswith(os.path.realpath(STANDALONE_DIR)) for p in loaded), loaded


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


# ---- 6. a full-size batch ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _files_4k():
    import oracle_lib as O
    files = [TC.cjpeg(O.synthetic_frame(3840, 2160, seed=100 + i), ["-revert", "-quality", "75", "-sample", "2x2"]) for i in range(2)]
    refs = []
    for f in files:
        rc, text, data = CC.dump_files(O.REF_DIR, "dump", [f])
        assert rc == 0, text
        refs.append(CC.parse_dump(data))
    return files, refs


def test_full_size_batch():
    """2 distinct 4K 4:2:0 q75 files in one call: 480 x 270 luma blocks, 2026 workgroups per image"""
    files, refs = _files_4k()
    outs = M.decode_coefficients(files, max_batch=2)
    for o, ref in zip(outs, refs):
        assert CC.same_arrays(o, ref)
