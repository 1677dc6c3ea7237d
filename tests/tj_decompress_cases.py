"""The cases and checkers of the TurboJPEG decompress tests: the shipped mozjpeg_amd/libmozjpeg_hip_turbojpeg.so next to the
reference's oracle/_ref/libturbojpeg.so.0, both loaded through ctypes in one process, the same calls made on both and the bytes
they leave compared for exact equality -- the destination's padding included: both buffers start from the same pattern.

test_gpu_tj_decompress.py runs the checks on the chip.  test_simt_tj_decompress.py runs this file as a program in ONE child
process, with a copy of the shipped library whose libmozjpeg_hip.so is the kernel sources on the wave64 emulator
(tools/simt/fuzz_cjpeg.dropin_dir): a process can hold only one library of that name, and the test process may hold the
device one.  The child prints one JSON object, check name -> "ok" or the traceback.

Sources are made at test time with the reference's cjpeg."""
import ctypes as C
import functools
import json
import os
import sys
import threading
import traceback

import numpy as np

import decode_cases as DC
import fast_idct_cases as FC
import oracle_lib as O
import transcode_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TJSHIM = os.path.join(ROOT, "mozjpeg_amd", "libmozjpeg_hip_turbojpeg.so")
TJLIB = FC.TJLIB

TJINIT_COMPRESS, TJINIT_DECOMPRESS = 0, 1
(P_STOPONWARNING, P_BOTTOMUP, P_NOREALLOC, P_QUALITY, P_SUBSAMP, P_JPEGWIDTH, P_JPEGHEIGHT, P_PRECISION, P_COLORSPACE, P_FASTUPSAMPLE,
 P_FASTDCT, P_OPTIMIZE, P_PROGRESSIVE, P_SCANLIMIT, P_ARITHMETIC, P_LOSSLESS, P_LOSSLESSPSV, P_LOSSLESSPT, P_RESTARTBLOCKS,
 P_RESTARTROWS, P_XDENSITY, P_YDENSITY, P_DENSITYUNITS, P_MAXMEMORY, P_MAXPIXELS) = range(25)
HEADER_PARAMS = (P_JPEGWIDTH, P_JPEGHEIGHT, P_SUBSAMP, P_COLORSPACE, P_PRECISION, P_XDENSITY, P_YDENSITY, P_DENSITYUNITS, P_PROGRESSIVE,
                 P_ARITHMETIC, P_LOSSLESS)
# TJPF_: RGB BGR RGBX BGRX XBGR XRGB GRAY RGBA BGRA ABGR ARGB CMYK
PIXEL_SIZE = [3, 3, 4, 4, 4, 4, 1, 4, 4, 4, 4, 4]
PF_RGB, PF_BGRX, PF_GRAY, PF_CMYK = 0, 3, 6, 11
FLAG_BOTTOMUP, FLAG_FASTUPSAMPLE, FLAG_FASTDCT = 2, 256, 2048
TJSAMP_GRAY = 3
FILL = 0xA5


def have_tools():
    return FC.have_tools() and os.path.exists(TJSHIM)


class ScalingFactor(C.Structure):
    _fields_ = [("num", C.c_int), ("denom", C.c_int)]


class Region(C.Structure):
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("w", C.c_int), ("h", C.c_int)]


def load(path):
    L = C.CDLL(path)
    vp, cp, i, sz, ul = C.c_void_p, C.c_char_p, C.c_int, C.c_size_t, C.c_ulong
    L.tj3Init.restype = vp
    L.tj3Init.argtypes = [i]
    L.tjInitDecompress.restype = vp
    L.tj3Destroy.argtypes = [vp]
    L.tjDestroy.argtypes = [vp]
    L.tj3Set.argtypes = [vp, i, i]
    L.tj3Get.argtypes = [vp, i]
    L.tj3GetErrorStr.restype = cp
    L.tj3GetErrorStr.argtypes = [vp]
    L.tj3GetErrorCode.argtypes = [vp]
    L.tj3GetScalingFactors.restype = C.POINTER(ScalingFactor)
    L.tj3GetScalingFactors.argtypes = [C.POINTER(i)]
    L.tj3SetScalingFactor.argtypes = [vp, ScalingFactor]
    L.tj3SetCroppingRegion.argtypes = [vp, Region]
    L.tj3DecompressHeader.argtypes = [vp, cp, sz]
    L.tjDecompressHeader3.argtypes = [vp, cp, ul] + [C.POINTER(i)] * 4
    L.tj3Decompress8.argtypes = [vp, cp, sz, vp, i, i]
    L.tj3Decompress12.argtypes = [vp, cp, sz, vp, i, i]
    L.tjDecompress2.argtypes = [vp, cp, ul, vp, i, i, i, i, i]
    L.tj3DecompressToYUVPlanes8.argtypes = [vp, cp, sz, C.POINTER(vp), C.POINTER(i)]
    L.tj3DecompressToYUV8.argtypes = [vp, cp, sz, vp, i]
    L.tjDecompressToYUV2.argtypes = [vp, cp, ul, vp, i, i, i, i]
    L.tj3YUVPlaneWidth.argtypes = [i] * 3
    L.tj3YUVPlaneHeight.argtypes = [i] * 3
    L.tj3YUVBufSize.restype = sz
    L.tj3YUVBufSize.argtypes = [i] * 4
    return L


SOURCES = {
    "s444": lambda: FC.source("s444"),
    "s422": lambda: TC.source("q90_2x1_r1"),
    "s420": lambda: TC.source("revert"),
    "gray": lambda: TC.source("gray_r5b"),
    "s440": lambda: TC.source("s1x2"),
    "s411": lambda: DC.source("s4x1"),
    "rgb": lambda: TC.source("rgb"),
    "density": lambda: TC.patch_jfif(TC.source("revert"), 1, 1, 2, 300, 150),
    "17x9": lambda: TC.source("17x9"),
    "17x9_422": lambda: FC.source("17x9_2x1"),
    "17x9_444": lambda: FC.source("17x9_444"),
    "17x9_gray": lambda: FC.source("17x9_gray"),
    "33x47": lambda: DC.source("33x47"),
    "47x33_422": lambda: DC.source("47x33_2x1"),
    "noise": lambda: TC.source("noise_q100"),
    "1x1": lambda: TC.source("1x1"),
    "8x8": lambda: TC.source("8x8"),
}


@functools.lru_cache(maxsize=None)
def source(name):
    return SOURCES[name]()


@functools.lru_cache(maxsize=None)
def progressive():
    return TC.cjpeg(TC.testorig(), ["-quality", "75"])


def truncated():
    src = source("s420")
    return src[:len(src) * 2 // 3]


def err(L, h):
    return (L.tj3GetErrorStr(h) or b"").decode()


def scaled(v, num, denom):
    return (v * num + denom - 1) // denom


class Pair:
    """the same calls on a handle of the shipped library (S) and one of the reference's (R)"""

    def __init__(self, S, R):
        self.S, self.R = S, R
        self.hs, self.hr = S.tj3Init(TJINIT_DECOMPRESS), R.tj3Init(TJINIT_DECOMPRESS)
        assert self.hs, "tj3Init(TJINIT_DECOMPRESS) of the shipped library returns NULL"
        assert self.hr

    def close(self):
        self.S.tj3Destroy(self.hs)
        self.R.tj3Destroy(self.hr)

    def both(self, fn, *args):
        """(shipped library's return value, the reference's)"""
        return getattr(self.S, fn)(self.hs, *args), getattr(self.R, fn)(self.hr, *args)

    def same(self, fn, *args):
        a, b = self.both(fn, *args)
        assert a == b, "%s%s: %d (%s), the reference %d (%s)" % (fn, args, a, err(self.S, self.hs), b, err(self.R, self.hr))
        return a

    def set(self, **kw):
        for k, v in kw.items():
            assert self.same("tj3Set", globals()["P_" + k.upper()], int(v)) == 0

    def size(self, src):
        assert self.same("tj3DecompressHeader", src, len(src)) == 0
        return self.R.tj3Get(self.hr, P_JPEGWIDTH), self.R.tj3Get(self.hr, P_JPEGHEIGHT), self.R.tj3Get(self.hr, P_SUBSAMP)

    def pixels(self, src, pf, pitch_extra=None, sf=(1, 1)):
        """tj3Decompress8 on both, into buffers of the same pattern with a spare row behind: the whole buffers must be equal"""
        w, h, _ = self.size(src)
        assert self.same("tj3SetScalingFactor", ScalingFactor(*sf)) == 0
        sw, sh = scaled(w, *sf), scaled(h, *sf)
        tight = sw * PIXEL_SIZE[pf]
        pitch = 0 if pitch_extra is None else tight + pitch_extra
        a = np.full(((pitch or tight) * (sh + 1),), FILL, np.uint8)
        b = a.copy()
        ra, rb = self.S.tj3Decompress8(self.hs, src, len(src), a.ctypes.data, pitch, pf), self.R.tj3Decompress8(self.hr, src, len(src), b.ctypes.data, pitch, pf)
        assert ra == rb == 0, "tj3Decompress8: %d (%s), the reference %d (%s)" % (ra, err(self.S, self.hs), rb, err(self.R, self.hr))
        assert np.array_equal(a, b), "tj3Decompress8 pf %d pitch %d at %d/%d: %d bytes differ" % (pf, pitch, sf[0], sf[1], int((a != b).sum()))
        return a


def with_pair(fn):
    @functools.wraps(fn)
    def run(S, R):
        p = Pair(S, R)
        try:
            fn(p)
        finally:
            p.close()
    return run


# ---- 1. headers ------------------------------------------------------------------------------------------------------------------
@with_pair
def check_headers(p):
    for prm in HEADER_PARAMS + (P_FASTUPSAMPLE, P_FASTDCT, P_BOTTOMUP, P_SCANLIMIT, P_MAXMEMORY, P_MAXPIXELS, P_QUALITY):
        assert p.same("tj3Get", prm) == p.R.tj3Get(p.hr, prm)             # a fresh handle
    for name in ("s444", "s422", "s420", "gray", "s440", "s411", "rgb", "density", "17x9", "1x1"):
        src = source(name)
        assert p.same("tj3DecompressHeader", src, len(src)) == 0, name
        for prm in HEADER_PARAMS:
            p.same("tj3Get", prm)
    assert (p.S.tj3Get(p.hs, P_SUBSAMP), p.S.tj3Get(p.hs, P_JPEGWIDTH)) == (2, 1)
    src = source("density")
    assert p.same("tj3DecompressHeader", src, len(src)) == 0
    assert [p.S.tj3Get(p.hs, q) for q in (P_XDENSITY, P_YDENSITY, P_DENSITYUNITS)] == [300, 150, 2]
    # the legacy form
    for L, h in ((p.S, p.hs), (p.R, p.hr)):
        out = [C.c_int(-5) for _ in range(4)]
        src = source("s440")
        assert L.tjDecompressHeader3(h, src, len(src), *[C.byref(v) for v in out]) == 0
        assert [v.value for v in out] == [227, 149, 4, 1]
    # the 16 scaling factors
    n, m = C.c_int(), C.c_int()
    fs, fr = p.S.tj3GetScalingFactors(C.byref(n)), p.R.tj3GetScalingFactors(C.byref(m))
    assert n.value == m.value == 16
    assert [(fs[k].num, fs[k].denom) for k in range(16)] == [(fr[k].num, fr[k].denom) for k in range(16)]
    for k in range(16):
        assert p.same("tj3SetScalingFactor", fs[k]) == 0
    for bad in ((1, 3), (0, 1), (3, 1), (2, 2)):
        assert p.same("tj3SetScalingFactor", ScalingFactor(*bad)) == -1
    # tj3Set as the reference has it for an instance without COMPRESS: every parameter, values inside and outside the range
    for prm in range(-1, 27):
        for v in (-1, 0, 1, 2, 7, 500):
            p.same("tj3Set", prm, v)
            p.same("tj3Get", prm)


# ---- 2. tj3Decompress8 --------------------------------------------------------------------------------------------------------
@with_pair
def check_pixel_formats(p):
    src = source("s420")
    for pf in range(11):
        a = p.pixels(src, pf)
        if pf in (7, 8, 9, 10):
            assert (a == 0xFF).sum() >= 227 * 149                           # the alpha byte
    for pf in (PF_RGB, PF_GRAY, PF_BGRX):
        p.pixels(source("gray"), pf)
        p.pixels(source("rgb"), pf)


GEOMETRIES = ("s420", "17x9_422", "33x47")


def _options(p, name):
    src = source(name)
    for sf in ((1, 1), (1, 2), (1, 4), (1, 8)):
        for extra in (None, 5):
            for bottom_up, fast_up, fast_dct in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
                p.set(bottomup=bottom_up, fastupsample=fast_up, fastdct=fast_dct)
                p.pixels(src, PF_RGB if extra is None else PF_BGRX, extra, sf)
    p.set(bottomup=0, fastupsample=0, fastdct=0)
    top = p.pixels(src, PF_RGB).copy()
    p.set(bottomup=1)
    w, h, _ = p.size(src)
    assert np.array_equal(p.pixels(src, PF_RGB)[:w * h * 3].reshape(h, w, 3), top[:w * h * 3].reshape(h, w, 3)[::-1])
    p.set(bottomup=0, fastdct=1)
    if name == "s420":                                                  # (the small synthetic frames are too smooth for the methods to differ)
        assert not np.array_equal(p.pixels(src, PF_RGB), top), "FASTDCT changes nothing"


@with_pair
def check_options_s420(p):
    _options(p, "s420")


@with_pair
def check_options_17x9_422(p):
    _options(p, "17x9_422")


@with_pair
def check_options_33x47(p):
    _options(p, "33x47")


# ---- 3. tjDecompress2 --------------------------------------------------------------------------------------------------------------
def _legacy(p, src, width, height, flags, pf=PF_RGB, expect=0):
    w, h, _ = p.size(src)
    size = max(width or w, w) * max(height or h, h) * PIXEL_SIZE[pf] + 64
    a = np.full((size,), FILL, np.uint8)
    b = a.copy()
    ra = p.S.tjDecompress2(p.hs, src, len(src), a.ctypes.data, width, 0, height, pf, flags)
    rb = p.R.tjDecompress2(p.hr, src, len(src), b.ctypes.data, width, 0, height, pf, flags)
    assert ra == expect, "tjDecompress2(%d x %d, flags %d): %d (%s)" % (width, height, flags, ra, err(p.S, p.hs))
    return ra, rb, a, b


@with_pair
def check_legacy(p):
    src = source("s420")
    for flags in (0, FLAG_FASTDCT, FLAG_BOTTOMUP | FLAG_FASTUPSAMPLE):
        for width, height in ((0, 0), (227, 149), (114, 75), (29, 19), (0, 75), (120, 149)):      # full, full, 1/2, 1/8, 1/2 by height, 1/2 by width
            ra, rb, a, b = _legacy(p, src, width, height, flags)
            assert rb == 0 and np.array_equal(a, b), (flags, width, height)
            for prm in (P_BOTTOMUP, P_FASTUPSAMPLE, P_FASTDCT, P_JPEGWIDTH, P_SUBSAMP):
                p.same("tj3Get", prm)
    # 199 x 131 is the 7/8 size: the reference decodes at 7/8, this library names the factor and writes nothing
    ra, rb, a, b = _legacy(p, src, 199, 131, 0, expect=-1)
    assert rb == 0 and "7/8" in err(p.S, p.hs) and (a == FILL).all() and not (b == FILL).all()
    ra, rb, a, b = _legacy(p, src, 10, 10, 0, expect=-1)                # nothing fits
    assert rb == -1 and (a == FILL).all()
    ra, rb, a, b = _legacy(p, src, 0, 0, 0)
    assert rb == 0 and np.array_equal(a, b)


# ---- 4. planar output --------------------------------------------------------------------------------------------------------
def _plane_dims(L, w, h, sub, sf):
    sw, sh = scaled(w, *sf), scaled(h, *sf)
    return [(L.tj3YUVPlaneWidth(c, sw, sub), L.tj3YUVPlaneHeight(c, sh, sub)) for c in range(1 if sub == TJSAMP_GRAY else 3)]


def _yuv(p, name):
    src = source(name)
    w, h, sub = p.size(src)
    for sf in ((1, 1), (1, 2)):
        assert p.same("tj3SetScalingFactor", ScalingFactor(*sf)) == 0
        dims = _plane_dims(p.R, w, h, sub, sf)
        assert dims == _plane_dims(p.S, w, h, sub, sf)
        for pad in (None, 3):
            for fast_dct in (0, 1):
                p.set(fastdct=fast_dct)
                outs = []
                for L, hd in ((p.S, p.hs), (p.R, p.hr)):
                    strides = [pw + (pad or 0) for pw, _ in dims] + [0] * (3 - len(dims))
                    planes = [np.full((st * ph + 16,), FILL, np.uint8) for st, (_, ph) in zip(strides, dims)]
                    ptrs = (C.c_void_p * 3)(*[q.ctypes.data for q in planes])
                    rc = L.tj3DecompressToYUVPlanes8(hd, src, len(src), ptrs, None if pad is None else (C.c_int * 3)(*strides))
                    assert rc == 0, "%s at %s: %s" % (name, sf, err(L, hd))
                    outs.append(planes)
                for c, (a, b) in enumerate(zip(*outs)):
                    assert np.array_equal(a, b), "%s at %d/%d, component %d, strides %s, fast %d" % (name, sf[0], sf[1], c, pad, fast_dct)
        p.set(fastdct=0)
        for align in (1, 4):
            n = p.R.tj3YUVBufSize(scaled(w, *sf), align, scaled(h, *sf), sub)
            assert n == p.S.tj3YUVBufSize(scaled(w, *sf), align, scaled(h, *sf), sub)
            a = np.full((n + 16,), FILL, np.uint8)
            b = a.copy()
            ra, rb = p.S.tj3DecompressToYUV8(p.hs, src, len(src), a.ctypes.data, align), p.R.tj3DecompressToYUV8(p.hr, src, len(src), b.ctypes.data, align)
            assert ra == rb == 0 and np.array_equal(a, b), "%s tj3DecompressToYUV8 align %d at %s" % (name, align, sf)
        a = np.full((p.R.tj3YUVBufSize(w, 4, h, sub) + 16,), FILL, np.uint8)
        b = a.copy()
        req = (0, 0) if sf == (1, 1) else (scaled(w, *sf), scaled(h, *sf))
        ra = p.S.tjDecompressToYUV2(p.hs, src, len(src), a.ctypes.data, req[0], 4, req[1], FLAG_FASTDCT)
        rb = p.R.tjDecompressToYUV2(p.hr, src, len(src), b.ctypes.data, req[0], 4, req[1], FLAG_FASTDCT)
        assert ra == rb == 0 and np.array_equal(a, b), "%s tjDecompressToYUV2 at %s" % (name, sf)
        p.set(fastdct=0)


@with_pair
def check_yuv_s420(p):
    _yuv(p, "s420")
    _yuv(p, "17x9")


@with_pair
def check_yuv_s422(p):
    _yuv(p, "s422")
    _yuv(p, "17x9_422")


@with_pair
def check_yuv_s444(p):
    _yuv(p, "s444")
    _yuv(p, "17x9_444")


@with_pair
def check_yuv_gray(p):
    _yuv(p, "gray")
    _yuv(p, "17x9_gray")


# ---- 5. one handle, many files; two handles in two threads ---------------------------------------------------------------------
@with_pair
def check_one_handle_many_files(p):
    names = ("s420", "17x9", "gray", "s444", "33x47", "rgb", "1x1", "8x8", "noise", "s420")
    first = None
    for k, name in enumerate(names):
        a = p.pixels(source(name), PF_RGB if k % 2 == 0 else PF_BGRX, sf=(1, 2) if k % 3 == 1 else (1, 1))
        if k == 0:
            first = a.copy()
    assert np.array_equal(p.pixels(source("s420"), PF_RGB), first)


def check_two_threads(S, R):
    errors = []

    def work(names):
        try:
            p = Pair(S, R)
            try:
                for _ in range(3):
                    for name in names:
                        p.pixels(source(name), PF_RGB)
            finally:
                p.close()
        except BaseException:
            errors.append(traceback.format_exc())

    for n in ("s420", "s422", "gray", "17x9"):
        source(n)
    ts = [threading.Thread(target=work, args=(names,)) for names in (("s420", "gray", "17x9"), ("s422", "17x9", "s420"))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors[0]


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
@with_pair
def check_refusals(p):
    S, hs = p.S, p.hs
    good = source("s420")

    def refused(rc, word=None):
        assert rc == -1, rc
        text = err(S, hs)
        assert text and text != "No error" and (word is None or word.lower() in text.lower()), text
        p.set(bottomup=0, fastupsample=0, fastdct=0)
        p.pixels(good, PF_RGB)                                           # the same handle still decodes a good file

    prog = progressive()
    refused(S.tj3DecompressHeader(hs, prog, len(prog)), "progressive")
    buf = np.full((227 * 149 * 4 + 64,), FILL, np.uint8)
    refused(S.tj3Decompress8(hs, prog, len(prog), buf.ctypes.data, 0, PF_RGB), "progressive")
    assert (buf == FILL).all()
    refused(S.tj3Decompress8(hs, good, len(good), buf.ctypes.data, 0, PF_CMYK), "CMYK")
    assert (buf == FILL).all()
    refused(S.tj3Decompress12(hs, good, len(good), buf.ctypes.data, 0, PF_RGB), "12-bit")
    assert p.same("tj3DecompressHeader", good, len(good)) == 0
    assert p.same("tj3SetCroppingRegion", Region(0, 0, 0, 0)) == 0
    refused(S.tj3SetCroppingRegion(hs, Region(16, 16, 32, 32)), "partial")
    for prm in (P_JPEGWIDTH, P_PRECISION, P_COLORSPACE, P_PROGRESSIVE, P_LOSSLESS, P_XDENSITY, P_QUALITY, P_NOREALLOC):
        assert p.same("tj3Set", prm, 1) == -1
        refused(-1)
    assert p.same("tj3SetScalingFactor", ScalingFactor(3, 8)) == 0
    refused(S.tj3Decompress8(hs, good, len(good), buf.ctypes.data, 0, PF_RGB), "3/8")
    assert (buf == FILL).all()
    assert p.same("tj3SetScalingFactor", ScalingFactor(1, 1)) == 0
    p.set(maxpixels=1000)
    ra, rb = p.both("tj3Decompress8", good, len(good), buf.ctypes.data, 0, PF_RGB)
    assert ra == rb == -1 and "too large" in err(S, hs) and (buf == FILL).all()
    p.set(maxpixels=0)
    cut = truncated()
    refused(S.tj3Decompress8(hs, cut, len(cut), buf.ctypes.data, 0, PF_RGB))
    assert (buf == FILL).all(), "a damaged file wrote to the destination"
    assert S.tj3GetErrorCode(hs) == 1                                    # TJERR_FATAL
    planes = [np.full((232 * 152,), FILL, np.uint8) for _ in range(3)]
    ptrs = (C.c_void_p * 3)(*[q.ctypes.data for q in planes])
    refused(S.tj3DecompressToYUVPlanes8(hs, cut, len(cut), ptrs, None))
    assert all((q == FILL).all() for q in planes)
    mixed = TC.source("s_mixed")                                         # no TJSAMP
    ra, rb = p.both("tj3DecompressToYUVPlanes8", mixed, len(mixed), ptrs, None)
    assert ra == rb == -1 and "subsampling" in err(S, hs)
    p.pixels(mixed, PF_RGB)
    ra, rb = p.both("tj3DecompressToYUV8", good, len(good), buf.ctypes.data, 3)          # align not a power of two
    assert ra == rb == -1
    ra, rb = p.both("tj3Decompress8", good, len(good), None, 0, PF_RGB)
    assert ra == rb == -1
    ra, rb = p.both("tj3Decompress8", good, len(good), buf.ctypes.data, 0, 12)
    assert ra == rb == -1
    # a compress handle is no decompress handle, and the other way round
    hc = S.tj3Init(TJINIT_COMPRESS)
    assert S.tj3DecompressHeader(hc, good, len(good)) == -1 and "decompression" in err(S, hc)
    S.tj3Destroy(hc)
    hd = S.tjInitDecompress()
    assert hd and S.tj3DecompressHeader(hd, good, len(good)) == 0 and S.tjDestroy(hd) == 0


CHECKS = {
    "headers": check_headers,
    "pixel_formats": check_pixel_formats,
    "options_s420": check_options_s420,
    "options_17x9_422": check_options_17x9_422,
    "options_33x47": check_options_33x47,
    "legacy": check_legacy,
    "yuv_s420": check_yuv_s420,
    "yuv_s422": check_yuv_s422,
    "yuv_s444": check_yuv_s444,
    "yuv_gray": check_yuv_gray,
    "one_handle_many_files": check_one_handle_many_files,
    "two_threads": check_two_threads,
    "refusals": check_refusals,
}

# ---- 7. the switch back to forwarding, in a child process (the variable is read when an instance is made) ------------------------
FORWARD_CHILD = """
import ctypes, sys
L = ctypes.CDLL(sys.argv[1])
L.tj3Init.restype = ctypes.c_void_p
L.tjGetErrorStr.restype = ctypes.c_char_p
h = L.tj3Init(1)
print("NULL" if not h else "HANDLE", L.tjGetErrorStr().decode())
c = L.tj3Init(0)
print("COMPRESS", "ok" if c else "NULL")
"""


def check_forwarding_switch(shim_path):
    import subprocess
    env = dict(os.environ, MOZJPEG_HIP_TJ_DECOMPRESS="0")
    r = subprocess.run([sys.executable, "-c", FORWARD_CHILD, shim_path], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    out = r.stdout.decode().splitlines()
    assert r.returncode == 0 and out[0].startswith("NULL ") and "MOZJPEG_HIP_TJ_DECOMPRESS" in out[0] and out[1] == "COMPRESS ok", (r.returncode, out, r.stderr.decode()[-400:])
    env["MOZJPEG_HIP_TJ_DECOMPRESS"] = "1"
    r = subprocess.run([sys.executable, "-c", FORWARD_CHILD, shim_path], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and r.stdout.decode().startswith("HANDLE"), (r.returncode, r.stdout, r.stderr.decode()[-400:])


def main(shim_path):
    """every check against the library at shim_path; prints {"name": "ok" | traceback}"""
    S, R = load(shim_path), load(TJLIB)
    res = {}
    for name, fn in CHECKS.items():
        try:
            fn(S, R)
            res[name] = "ok"
        except BaseException:
            res[name] = traceback.format_exc()
    print("TJ_DECOMPRESS_RESULTS " + json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1])
