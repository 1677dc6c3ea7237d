"""The case list and helpers of the tests of the twelve other IDCT sizes (test_simt_decode_scale_all.py on the emulator,
test_gpu_decode_scale_all.py on the chip): djpeg -scale 3/8, 5/8, 6/8, 7/8 and 9/8 to 16/8, the transforms jpeg_idct_3x3 to
jpeg_idct_16x16 of jidctint.c, reached with all_scales=True (mjh_decode_opts.all_scales) and, in the drop-in libraries, with
MOZJPEG_HIP_ALL_SCALES=1.

Sources are those of scale_cases.py; the expected pixels always come from the reference's djpeg at test time
(oracle/_ref/djpeg -scale M/8 + switches), planes from the reference's TurboJPEG library, and every comparison is exact
equality, shape and dtype included."""
import ctypes as C
import functools
import json
import math
import os
import sys
import traceback

import numpy as np

import cmyk_cases as CM
import decode_cases as DC
import djpeg_cases as DJ
import scale_cases as SC
import tj_decompress_cases as TD
import transcode_cases as TC

have_tools = SC.have_tools

NEW_SIZES = (3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16)
SOURCES = ["revert", "s_mixed", "gray_r5b", "q90_2x1_r1", "s1x2", "1x1", "17x9_2x1", "8x8_2x1", "noise_q100", "absurd_quant"]

CASES = [(s, "default", k) for s in SOURCES for k in NEW_SIZES]
CASES += [(s, "nosmooth", k) for s in ("revert", "s_mixed", "17x9_2x1", "absurd_quant") for k in NEW_SIZES]
CASES += [(s, "grayscale", k) for s in ("revert", "rgb") for k in NEW_SIZES]
CASES += [("gray_r5b", "rgb", k) for k in NEW_SIZES]
# fractions that are not M/8 -> the size djpeg resolves them to (jdmaster.c:105ff)
FRACTIONS = {"1/3": 3, "2/3": 6, "3/5": 5, "5/4": 10, "17/10": 14, "3/1": 16}
FRACTION_CASES = [(s, f) for s in ("revert", "17x9_2x1") for f in FRACTIONS]
LAYOUT_SIZES = (3, 7, 11, 16)
LAYOUT_CASES = [(s, k) for s in ("revert", "17x9_2x1") for k in LAYOUT_SIZES]
PLANE_CASES = [(s, k) for s in ("revert", "s_mixed") for k in (3, 6, 9, 16)]


def case_id(c):
    return "-".join(str(v) for v in c).replace("/", "_")


def arg(k):
    return "%d/8" % k


def run(M, name, mode, scale, **kw):
    return SC.run(M, name, mode, scale, all_scales=True, **kw)


# ---- 1. every new size against djpeg ------------------------------------------------------------------------------------------------
def check_case(M, name, mode, k):
    ref = SC.reference(name, mode, arg(k))
    out = run(M, name, mode, (k, 8))
    assert out.shape == SC.scaled_shape(M, name, mode, k) == ref.shape, "%s, the reference %s" % (out.shape, ref.shape)
    assert SC.same(out, ref)


# ---- 2. the premise of the case list ------------------------------------------------------------------------------------------------
def check_every_transform_size_is_reached(M):
    seen = set()
    for name, mode, k in CASES:
        if mode == "default":
            seen.add((name, tuple(SC.dct_scaled_sizes(M.jpeg_info(SC.source(name)), k))))
    for k in (3, 5, 6, 7):
        assert ("revert", (k, 2 * k, 2 * k)) in seen, (k, sorted(seen))
        assert ("s_mixed", (k, 2 * k, k)) in seen, (k, sorted(seen))
    for k in range(9, 17):
        assert ("revert", (k, k, k)) in seen, (k, sorted(seen))
    for k in NEW_SIZES:
        assert ("gray_r5b", (k,)) in seen, (k, sorted(seen))
    # the widths that pick the plain and the fancy h2v1 function at k = 3: chroma stays at 3 and is 2 / 4 samples wide
    for name, dw in (("8x8_2x1", 2), ("17x9_2x1", 4)):
        info = M.jpeg_info(SC.source(name))
        assert SC.dct_scaled_sizes(info, 3) == [3, 3, 3]
        assert -(-info.image_width * 1 * 3 // (2 * 8)) == dw


# ---- 3. fractions -------------------------------------------------------------------------------------------------------------------
def check_fraction(M, name, frac):
    k = FRACTIONS[frac]
    num, denom = (int(v) for v in frac.split("/"))
    assert M.scale_idct_size(num, denom) == k
    ref = SC.reference(name, "default", frac)
    assert ref.shape == SC.scaled_shape(M, name, "default", k), "the reference resolves %s otherwise" % frac
    assert SC.same(run(M, name, "default", frac), ref)
    assert SC.same(run(M, name, "default", (num, denom)), ref)


# ---- 4. layouts and colour kernels --------------------------------------------------------------------------------------------------
def check_layouts(M, name, k):
    src = SC.source(name)
    rgb = SC.reference(name, "rgb", arg(k))
    out = M.decode([src], color="rgb", layout="bgrx", scale=(k, 8), all_scales=True)[0]
    DC.check_layout(rgb, out, "bgrx")
    for dither in (True, False):
        out = M.decode([src], color="rgb565", dither=dither, scale=arg(k), all_scales=True)[0]
        ref = DJ.djpeg565(src, dither, True, arg(k))
        assert DJ.same565(out, ref), "rgb565 dither %s: %s %s, the reference %s" % (dither, out.shape, out.dtype, ref.shape)
    up = M.decode([src], scale=(k, 8), all_scales=True, bottom_up=True)[0]
    assert SC.same(up[::-1], SC.reference(name, "default", arg(k)))


def check_four_components(M):
    """a YCCK 4:2:0 file (chroma at 6 beside Y and K at 3; every component at 9) and a CMYK file, against the reference's
    tj3Decompress8 with TJPF_CMYK"""
    for name in ("tj_ycck420", "cmyk"):
        src = CM.source(name)
        for sf in ((3, 8), (9, 8)):
            rc, ref, text = CM.tj_pixels(src, scale=sf)
            assert rc == 0, text
            out = M.decode([src], scale=sf, all_scales=True)[0]
            assert not isinstance(out, Exception), out
            assert CM.same(out, ref), (name, sf)


@functools.lru_cache(maxsize=None)
def arithmetic_source():
    return TC.cjpeg(TC.testorig(), ["-revert", "-arithmetic"])


def check_other_entropy_coders(M):
    """a progressive and an arithmetic-coded source, which share the pixel stage, with their opt-ins"""
    for src, kw in ((TD.progressive(), dict(progressive_sources=True)), (arithmetic_source(), dict(arithmetic_sources=True))):
        for k in (5, 13):
            out = M.decode([src], scale=(k, 8), all_scales=True, **kw)[0]
            assert not isinstance(out, Exception), out
            assert SC.same(out, DC.djpeg(src, ["-scale", arg(k)])), (sorted(kw), k)


# ---- 5. raw planes ------------------------------------------------------------------------------------------------------------------
def reference_planes(jpeg, sf):
    """the planes of the reference's tj3DecompressToYUVPlanes8 at scaling factor sf, or None where it has no TJSAMP for the file"""
    L = CM.tj()
    h = L.tj3Init(TD.TJINIT_DECOMPRESS)
    try:
        assert L.tj3DecompressHeader(h, jpeg, len(jpeg)) == 0, TD.err(L, h)
        w, ht, sub = L.tj3Get(h, TD.P_JPEGWIDTH), L.tj3Get(h, TD.P_JPEGHEIGHT), L.tj3Get(h, TD.P_SUBSAMP)
        if sub < 0:
            return None
        g = math.gcd(*sf)
        sf = (sf[0] // g, sf[1] // g)                                 # (the library knows its 16 factors in lowest terms)
        assert L.tj3SetScalingFactor(h, TD.ScalingFactor(*sf)) == 0, TD.err(L, h)
        dims = TD._plane_dims(L, w, ht, sub, sf)
        planes = [np.zeros((ph, pw), np.uint8) for pw, ph in dims]
        ptrs = (C.c_void_p * 3)(*([q.ctypes.data for q in planes] + [None] * (3 - len(planes))))
        assert L.tj3DecompressToYUVPlanes8(h, jpeg, len(jpeg), ptrs, None) == 0, TD.err(L, h)
        return planes
    finally:
        L.tj3Destroy(h)


def check_planes(M, name, k):
    """decode_planes against the reference's TurboJPEG; where that library has no subsampling name for the file (2x2,1x1,2x1),
    against the luma of djpeg -grayscale and the geometry, and in both cases the device view against mjh_get_plane"""
    src = SC.source(name)
    info = M.jpeg_info(src)
    got = M.decode_planes([src], scale=(k, 8), all_scales=True)[0]
    assert not isinstance(got, Exception), got
    ref = reference_planes(src, (k, 8))
    if ref is not None:
        assert len(got) == len(ref)
        for c, (a, b) in enumerate(zip(got, ref)):
            assert SC.same(a, b), (name, k, c)
    else:
        gray = SC.reference(name, "grayscale", arg(k))
        assert np.array_equal(got[0][:gray.shape[0], :gray.shape[1]], gray)
    assert [a.shape for a in got] == [M.yuv_plane_size(info, c, k) for c in range(info.num_components)]


def device_planes(M, enc, n, comps, fetch):
    """component c of image i of the last raw_planes batch through mjh_get_planes_device; fetch(ptr, nbytes) -> bytes"""
    out = []
    for c in range(comps):
        ptr, pitch, stride, w, h = enc.planes_device(c)
        raw = np.frombuffer(fetch(ptr, stride * (n - 1) + pitch * (h - 1) + w), np.uint8)
        out.append([np.stack([raw[i * stride + y * pitch:i * stride + y * pitch + w] for y in range(h)]) for i in range(n)])
    return out


def check_device_planes(M, name, k, fetch):
    """mjh_get_planes_device against mjh_get_plane, two images in the batch: offsets, pitch and image stride of the call's layout"""
    src = SC.source(name)
    info = M.jpeg_info(src)
    enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=2)
    host = enc.decode_host([src, src], scale=(k, 8), all_scales=True, raw_planes=True)
    enc.submit_decode([src, src], scale=(k, 8), all_scales=True, raw_planes=True)
    enc.wait_decode()
    dev = device_planes(M, enc, 2, info.num_components, fetch)
    for c in range(info.num_components):
        _, pitch, stride, w, h = enc.planes_device(c)
        wib, hib = enc.geometry(c)[:2]
        assert (w, h) == (wib * k, hib * k) and pitch == (w + 3) & ~3 and stride >= pitch * h
        for i in range(2):
            ph, pw = host[i][c].shape
            assert np.array_equal(dev[c][i][:min(ph, h), :min(pw, w)], host[i][c][:min(ph, h), :min(pw, w)]), (name, k, c, i)
    enc.close()


# ---- 6. one encoder, many scales ----------------------------------------------------------------------------------------------------
def check_one_encoder_serves_every_scale(M):
    for name in ("revert", "s_mixed", "gray_r5b"):
        src = SC.source(name)
        full = DC.reference(name, "default")
        enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=1)
        for scale, k in (("2/1", 16), ("1/8", 1), ("3/8", 3), ("1/1", 8), ("9/8", 9), ("1/2", 4), ("7/8", 7), ("1/1", 8)):
            out = enc.decode_host([src], scale=scale, all_scales=True)[0]
            st = enc.decode_stats()
            assert (st["height"], st["width"]) == out.shape[:2] == SC.scaled_shape(M, name, "default", k)[:2]
            assert SC.same(out, full if k == 8 else SC.reference(name, "default", arg(k))), (name, scale)
        enc.close()


# ---- 7. a mixed batch with a damaged file -------------------------------------------------------------------------------------------
def check_mixed_batch(M):
    names = ["revert", "gray_r5b", "17x9_2x1", "s_mixed", "revert_opt", "rgb", "8x8", "q90_2x1_r1"]
    files = [SC.source(s) for s in names]
    files.insert(3, SC.damaged(TC.source("revert"), M))
    names.insert(3, None)
    for k in (3, 11):
        outs = M.decode(files, max_batch=4, scale=(k, 8), all_scales=True)
        for s, o in zip(names, outs):
            if s is None:
                assert isinstance(o, M.MjhError) and o.code == M.EINVAL and "Corrupt" in str(o)
            else:
                assert SC.same(o, SC.reference(s, "default", arg(k))), (s, k)


# ---- 9. the opt-in is the only door -------------------------------------------------------------------------------------------------
def raw_opts(M, num, denom, all_scales):
    o = SC.raw_opts(M, num, denom)
    o.all_scales = all_scales
    return o


def check_opt_in(M):
    src = TC.source("revert")
    M._decode_encoders.clear()
    for scale, word in (("3/8", "3x3"), ((2, 1), "16x16")):
        with SC.pytest_raises(M, M.EUNSUPPORTED, word):
            M.decode([src], scale=scale)
        with SC.pytest_raises(M, M.EUNSUPPORTED, word):
            M.decode([src], scale=scale, all_scales=False)
        with SC.pytest_raises(M, M.EUNSUPPORTED, word):
            M.decode_planes([src], scale=scale)
    for scale in ((0, 3), (-1, 8), (1, 0)):
        with SC.pytest_raises(M, M.EINVAL, "scale"):
            M.decode([src], scale=scale, all_scales=True)
    assert not M._decode_encoders                                     # refused before anything was grouped
    enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=1)
    full = enc.decode_host([src])[0]
    for (num, denom), word in (((3, 8), "3x3"), ((2, 1), "16x16")):
        with SC.pytest_raises(M, M.EUNSUPPORTED, word):
            enc.decode_host([src], opts=raw_opts(M, num, denom, 0))
        assert M.lib().mjh_transcode_batch_size(enc._h) == 0
    for num, denom in ((0, 3), (-1, 8), (1, 0)):
        with SC.pytest_raises(M, M.EINVAL, "scale"):
            enc.decode_host([src], opts=raw_opts(M, num, denom, 1))
    assert SC.same(enc.decode_host([src], opts=raw_opts(M, 3, 8, 1))[0], SC.reference("revert", "default", "3/8"))
    assert SC.same(enc.decode_host([src], opts=raw_opts(M, 1000, 1, 1))[0], SC.reference("revert", "default", "16/8"))
    o = M.DecodeOpts()                                                # a zeroed struct is still 1/1 (and no fancy upsampling)
    assert (o.scale_num, o.scale_denom, o.all_scales) == (0, 0, 0)
    assert SC.same(enc.decode_host([src], opts=o)[0], DC.reference("revert", "nosmooth"))
    o.all_scales = 1
    assert SC.same(enc.decode_host([src], opts=o)[0], DC.reference("revert", "nosmooth"))
    assert SC.same(enc.decode_host([src])[0], full)
    enc.close()
    enc = M.Encoder(M.params_from_jpeg(src, revert=True, transform="flip_h"), max_batch=1)
    with SC.pytest_raises(M, M.EUNSUPPORTED, "transform"):
        enc.decode_host([src], scale="3/8", all_scales=True)
    enc.close()


# ---- 10. the drop-in libraries ------------------------------------------------------------------------------------------------------
ENV = "MOZJPEG_HIP_ALL_SCALES"
DJPEG_SWITCHES = {"scale3_8": ["-scale", "3/8"], "scale5_4": ["-scale", "5/4"], "scale2_1_nosmooth": ["-scale", "2/1", "-nosmooth"]}
DJPEG_PAIRS = [(s, k) for s in ("revert", "gray_r5b") for k in DJPEG_SWITCHES]


def check_djpeg(R, name, switches):
    """R: a djpeg_cases.Runner whose stand-alone runs have MOZJPEG_HIP_ALL_SCALES=1"""
    DJ.check_djpeg(R, name, DJPEG_SWITCHES[switches])


def check_djpeg_refuses_without_the_variable(R0):
    """R0: a Runner without the variable -- the refusal of today"""
    DJ.check_djpeg_refused(R0, DC.source("revert"), ["-scale", "3/8"], "3x3")


@TD.with_pair
def check_tj_factors(p):
    os.environ[ENV] = "1"
    src = TD.source("s420")
    n = C.c_int()
    fs = p.R.tj3GetScalingFactors(C.byref(n))
    assert n.value == 16
    for i in range(16):
        p.pixels(src, TD.PF_RGB, sf=(fs[i].num, fs[i].denom))
    p.pixels(src, TD.PF_BGRX, pitch_extra=5, sf=(11, 8))
    p.pixels(TD.source("gray"), TD.PF_GRAY, sf=(3, 8))


@TD.with_pair
def check_tj_legacy(p):
    """tjDecompress2 with a requested 100 x 70 on the 227 x 149 file: the first factor that fits is 3/8 (86 x 56)"""
    os.environ[ENV] = "1"
    src = TD.source("s420")
    ra, rb, a, b = TD._legacy(p, src, 100, 70, 0)
    assert rb == 0 and np.array_equal(a, b) and not (a == TD.FILL).all()
    ra, rb, a, b = TD._legacy(p, src, 199, 131, 0)                    # the 7/8 size
    assert rb == 0 and np.array_equal(a, b)


@TD.with_pair
def check_tj_planes(p):
    os.environ[ENV] = "1"
    src = TD.source("s420")
    w, h, sub = p.size(src)
    for sf in ((3, 8), (9, 8), (2, 1)):
        assert p.same("tj3SetScalingFactor", TD.ScalingFactor(*sf)) == 0
        n = p.R.tj3YUVBufSize(TD.scaled(w, *sf), 4, TD.scaled(h, *sf), sub)
        a = np.full((n + 16,), TD.FILL, np.uint8)
        b = a.copy()
        ra, rb = p.S.tj3DecompressToYUV8(p.hs, src, len(src), a.ctypes.data, 4), p.R.tj3DecompressToYUV8(p.hr, src, len(src), b.ctypes.data, 4)
        assert ra == rb == 0 and np.array_equal(a, b), "tj3DecompressToYUV8 at %s: %s" % (sf, TD.err(p.S, p.hs))


@TD.with_pair
def check_tj_unset_refuses(p):
    """the variable is read per call: set, 3/8 decodes; unset in the same process, it is refused as it always was"""
    src = TD.source("s420")
    os.environ[ENV] = "1"
    p.pixels(src, TD.PF_RGB, sf=(3, 8))
    os.environ.pop(ENV, None)
    w, h, _ = p.size(src)
    assert p.same("tj3SetScalingFactor", TD.ScalingFactor(3, 8)) == 0
    a = np.full((TD.scaled(w, 3, 8) * TD.scaled(h, 3, 8) * 3,), TD.FILL, np.uint8)
    assert p.S.tj3Decompress8(p.hs, src, len(src), a.ctypes.data, 0, TD.PF_RGB) == -1
    assert "3/8" in TD.err(p.S, p.hs) and (a == TD.FILL).all()
    p.pixels(src, TD.PF_RGB, sf=(1, 2))


TJ_CHECKS = {"factors": check_tj_factors, "legacy": check_tj_legacy, "planes": check_tj_planes, "unset_refuses": check_tj_unset_refuses}


def main(shim_path):
    """every TurboJPEG check against the library at shim_path, in a process of its own; prints {"name": "ok" | traceback}"""
    S, R = TD.load(shim_path), TD.load(TD.TJLIB)
    res = {}
    for name, fn in TJ_CHECKS.items():
        try:
            fn(S, R)
            res[name] = "ok"
        except BaseException:
            res[name] = traceback.format_exc()
        finally:
            os.environ.pop(ENV, None)
    print("SCALE_ALL_TJ_RESULTS " + json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1])
