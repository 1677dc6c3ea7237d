"""Lossless JPEG (SOF3) on the GPU through the C ABI, byte for byte against the reference: its TurboJPEG library
(oracle/_ref/libturbojpeg.so.0, tj3Compress8/12/16 with TJPARAM_LOSSLESS*) and its cjpeg (`-revert -lossless psv,Pt`), both built by
oracle/Makefile.  Precision 8 / 12 / 16 x PSV 1..7 x Pt in {0, 1, P-1}, gray and RGB and two extended layouts, sizes from 1x1 to 4K,
restart intervals, random / flat / smooth / extreme images (the 16-bit difference 32768), batches of distinct 4K frames with two
batches in flight and one, the host entry and the refusals."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import mozjpeg_amd as M
import lossless_cases as LC

pytestmark = pytest.mark.gpu


def _ref(a, psv, pt, prec, rows=0):
    return LC.tj_compress(a, psv, pt, prec, "GRAY" if a.shape[2] == 1 else "RGB", rows)


def _ours(a, psv, pt, prec, rows=None, max_batch=1):
    enc = M.Encoder(LC.params(M, a, psv, pt, prec, rows), max_batch=max_batch)
    return enc.encode_host(a)[0]


@pytest.mark.parametrize("prec", [8, 12, 16])
@pytest.mark.parametrize("comps", [1, 3])
def test_lossless_every_predictor_and_point_transform(prec, comps):
    a = LC.image("smooth", 149, 227, comps, prec, seed=prec + comps)
    bad = []
    for psv in range(1, 8):
        for pt in sorted({0, 1, prec - 1}):
            if _ours(a, psv, pt, prec) != _ref(a, psv, pt, prec):
                bad.append((psv, pt))
    assert not bad


@pytest.mark.parametrize("kind", ["random", "flat", "smooth", "extreme"])
@pytest.mark.parametrize("prec", [8, 12, 16])
@pytest.mark.parametrize("rows", [None, 1, 3, 7])
def test_lossless_images_and_restart_intervals(kind, prec, rows):
    """restart intervals of 1, 3 and 7 rows (7 does not divide the 149 rows)"""
    for comps, psv in ((3, 1), (1, 6)):
        a = LC.image(kind, 149, 227, comps, prec, seed=11)
        assert _ours(a, psv, 0, prec, rows) == _ref(a, psv, 0, prec, rows or 0), (comps, psv)


@pytest.mark.parametrize("hw", [(1, 1), (1, 37), (53, 1), (149, 227), (2, 1025), (3, 2049)])
def test_lossless_sizes(hw):
    h, w = hw
    for prec in (8, 16):
        for comps in (1, 3):
            a = LC.image("random", h, w, comps, prec, seed=h * w)
            for psv in (1, 7):
                assert _ours(a, psv, 0, prec, 1) == _ref(a, psv, 0, prec, 1), (prec, comps, psv)
                assert _ours(a, psv, 0, prec) == _ref(a, psv, 0, prec), (prec, comps, psv)


def test_lossless_difference_32768():
    """16-bit: 0 next to 32768 with PSV 1 gives the difference -32768, category 16 with no value bits (jclhuff.c:359-365); 0 next to
    65535 gives 65535 = -1 mod 2^16"""
    a = LC.image("extreme", 64, 96, 1, 16)
    enc = M.Encoder(LC.params(M, a, 1, 0, 16), max_batch=1)
    out = enc.encode_host(a)[0]
    counts = np.zeros(17, np.uint32)
    n = M.C.c_size_t()
    M._chk(M.lib().mjh_read_tap(enc._h, M.TAP_LL_COUNTS, 0, 0, counts.ctypes.data, counts.nbytes, M.C.byref(n)))
    assert counts[16] > 0 and counts.sum() == 64 * 96
    assert out == _ref(a, 1, 0, 16) == LC.reference(a, 1, 0, 16)


@pytest.mark.parametrize("fmt", ["BGRX", "XRGB"])
@pytest.mark.parametrize("prec", [8, 16])
def test_lossless_extended_pixel_layouts(fmt, prec):
    a = LC.image("smooth", 61, 83, 3, prec, seed=5)
    px, off = LC.TJPF_LAYOUT[fmt]
    b = np.full((61, 83, px), (1 << prec) - 1, a.dtype)
    for c in range(3):
        b[..., off[c]] = a[..., c]
    p = LC.params(M, a, 5, 1, prec, 2)
    p.input_pixel_size = px
    for c in range(3):
        p.rgb_offset[c] = off[c]
    out = M.Encoder(p, max_batch=1).encode_host(b)[0]
    assert out == LC.tj_compress(b, 5, 1, prec, fmt, 2) == _ref(a, 5, 1, prec, 2)


def test_lossless_cjpeg_agrees():
    """the same files as cjpeg -revert -lossless (the switch vocabulary of make_params), 8 / 12 / 16 bits"""
    for prec, comps, psv, pt, rows in ((8, 3, 1, 0, None), (12, 1, 4, 3, 2), (16, 3, 7, 0, 1), (16, 1, 2, 15, None)):
        a = LC.image("random", 40, 70, comps, prec, seed=prec)
        assert _ours(a, psv, pt, prec, rows) == LC.reference(a, psv, pt, prec, rows), (prec, comps, psv, pt, rows)


def _frames_4k(n, prec, comps, seed):
    """distinct 4K frames: the SURVEY 8d synthetic frame with a seed per frame (16-bit: the 12-bit variant x 16 + noise in the low bits)"""
    import oracle_lib as O
    out = []
    for i in range(n):
        if prec == 8:
            out.append(np.ascontiguousarray(O.synthetic_frame(3840, 2160, seed=seed * 100 + i)[..., :comps]))
        else:
            f = O.synthetic_frame12(3840, 2160, seed=seed * 100 + i)[..., :comps].astype(np.uint32) * 16
            out.append((f + np.random.RandomState(i).randint(0, 16, f.shape)).astype(np.uint16))
    return out


def _refs(frames, psv, prec):
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda f: _ref(f, psv, 0, prec), frames))


def _device_files(enc, frames):
    import torch
    t = torch.from_numpy(np.stack(frames).view(np.int16) if frames[0].dtype == np.uint16 else np.stack(frames)).cuda()
    torch.cuda.synchronize()
    enc.encode_tensor(t)
    return [enc.get_jpeg(i) for i in range(len(frames))]


@pytest.mark.parametrize("prec,comps,psv", [(8, 3, 1), (16, 1, 1)])
def test_lossless_4k_device_batch_twice_in_flight(prec, comps, psv):
    """8 distinct 4K frames per call, two calls back to back with different inputs while two batches are in flight; then the
    same with mjh_set_inflight(1): every file equals the reference's"""
    import torch  # noqa: F401
    fa, fb = _frames_4k(8, prec, comps, 1), _frames_4k(8, prec, comps, 2)
    ra, rb = _refs(fa, psv, prec), _refs(fb, psv, prec)
    enc = M.Encoder(LC.params(M, fa[0], psv, 0, prec), max_batch=8)
    import torch as T
    ta = T.from_numpy(np.stack(fa).view(np.int16) if prec > 8 else np.stack(fa)).cuda()
    tb = T.from_numpy(np.stack(fb).view(np.int16) if prec > 8 else np.stack(fb)).cuda()
    T.cuda.synchronize()
    enc.encode_tensor(ta, stream="own")
    enc.encode_tensor(tb, stream="own")       # (the second buffer set, while the first call may still run on the first)
    got_b = [enc.get_jpeg(i) for i in range(8)]
    assert got_b == rb
    enc.encode_tensor(ta, stream="own")
    assert [enc.get_jpeg(i) for i in range(8)] == ra
    enc.set_inflight(1)
    assert _device_files(enc, fb) == rb
    assert _device_files(enc, fa) == ra


def test_lossless_4k_host_path_and_collect():
    """mjh_encode_host with two batches queued before the first is collected"""
    fa, fb = _frames_4k(4, 8, 3, 3), _frames_4k(4, 8, 3, 4)
    ra, rb = _refs(fa, 6, 8), _refs(fb, 6, 8)
    enc = M.Encoder(LC.params(M, fa[0], 6, 0, 8), max_batch=4)
    enc.submit_host(np.stack(fa))
    enc.submit_host(np.stack(fb))
    assert enc.collect(age=1) == ra
    assert enc.collect(age=0) == rb


def test_lossless_pool():
    frames = [LC.image("random", 50, 60, 3, 8, seed=s) for s in range(5)]
    pool = M.Pool(LC.params(M, frames[0], 2, 0, 8), max_batch_per_device=2, devices=[0])
    assert pool.encode_host(np.stack(frames)) == [_ref(f, 2, 0, 8) for f in frames]
    pool.close()


def test_lossless_refusals_match_the_reference():
    """cjpeg -lossless without -revert (trellis quantization: "Bogus buffer control mode"), -restart 3B and -arithmetic fail in the
    reference; the library returns an error for the same parameters"""
    import subprocess
    import tempfile
    a = LC.image("random", 8, 10, 3, 8)
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "in.ppm")
        LC.write_pnm(f, a, 8)
        r = subprocess.run([LC.CJPEG, "-lossless", "1", f], capture_output=True)
    assert r.returncode != 0 and b"Bogus buffer control mode" in r.stderr
    p = M.make_params(10, 8, lossless=(1, 0))
    p.compress_profile = M.PROFILE_FASTEST          # (trellis_quant stays on from the max-compression defaults)
    assert p.trellis_quant
    with pytest.raises(M.MjhError):
        M.Encoder(p, max_batch=1)
    assert not isinstance(LC.reference(a, 1, 0, 8, extra=["-restart", "3B"]), bytes)
    p = LC.params(M, a, 1, 0, 8)
    p.restart_interval = 3
    with pytest.raises(M.MjhError) as ei:
        M.Encoder(p, max_batch=1)
    assert "restart interval" in str(ei.value)
    assert not isinstance(LC.reference(a, 1, 0, 8, extra=["-arithmetic"]), bytes)
    p = LC.params(M, a, 1, 0, 8)
    p.arith_code = 1
    with pytest.raises(M.MjhError):
        M.Encoder(p, max_batch=1)
