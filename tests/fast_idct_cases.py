"""The case list and helpers of the tests of the fast integer IDCT (k_idct_ifast, djpeg -dct fast), bottom-up rows and raw sample
planes (test_simt_decode_fast.py on the emulator, test_gpu_decode_fast.py on the chip).

Sources are made at test time by the reference's cjpeg (transcode_cases / decode_cases / scale_cases plus a quality-25 and a
quality-100 file).  Expected pixels always come from the reference at test time: oracle/_ref/djpeg -pnm -dct fast [-scale k/8]
for pixels, oracle/_ref/libturbojpeg.so.0's tj3DecompressToYUVPlanes8 for planes; every comparison is exact equality, shape
included."""
import ctypes as C
import functools
import os

import numpy as np

import decode_cases as DC
import oracle_lib as O
import scale_cases as SC
import transcode_cases as TC

TJLIB = os.path.join(O.REF_DIR, "libturbojpeg.so.0")


def have_tools():
    return DC.have_tools() and os.path.exists(TJLIB)


EXTRA = {
    "q25": lambda: TC.cjpeg(TC.testorig(), ["-revert", "-quality", "25"]),
    "q100": lambda: TC.cjpeg(TC.testorig(), ["-revert", "-quality", "100"]),
    "s444": lambda: TC.cjpeg(TC.testorig(), ["-revert", "-sample", "1x1"]),
    "17x9_444": lambda: TC.cjpeg(O.synthetic_frame(17, 9, 5), ["-revert", "-sample", "1x1"]),
    "17x9_1x2": lambda: TC.cjpeg(O.synthetic_frame(17, 9, 5), ["-revert", "-sample", "1x2"]),
    "17x9_gray": lambda: TC.cjpeg(O.synthetic_frame(17, 9, 5), ["-revert", "-grayscale"]),
}
NAMES = ["revert", "q90_2x1_r1", "s1x2", "s_mixed", "gray_r5b", "rgb", "scans3_2x2_r2", "1x1", "8x8", "17x9", "noise_q100", "q25", "q100"]
MODES = ("default", "nosmooth", "grayscale")
CASES = [(s, m) for s in NAMES for m in MODES]
MUST_DIFFER = ("revert", "noise_q100")
SCALED_CASES = [(s, sc) for s in ("revert", "s_mixed", "17x9_2x1") for sc in SC.SCALES]
FLIP_CASES = [(kw, sc) for kw in ("rgb", "gray", "bgrx") for sc in (None, "1/4")]
FLIP_KW = {"rgb": dict(color="rgb"), "gray": dict(color="gray"), "bgrx": dict(color="rgb", layout="bgrx")}
# name -> TurboJPEG's subsampling: 4:2:0, 4:2:2, 4:4:0, 4:4:4, gray at 227x149 and 17x9
PLANE_SOURCES = ["revert", "q90_2x1_r1", "s1x2", "s444", "gray_r5b", "17x9", "17x9_2x1", "17x9_1x2", "17x9_444", "17x9_gray"]
PLANE_CASES = [(s, sc) for s in PLANE_SOURCES for sc in (None, "1/2")]


def case_id(c):
    return "-".join(str(v) for v in c).replace("/", "_")


@functools.lru_cache(maxsize=None)
def source(name):
    return EXTRA[name]() if name in EXTRA else SC.source(name)


@functools.lru_cache(maxsize=None)
def reference(name, mode, scale_arg=None, fast=True):
    args = (["-dct", "fast"] if fast else []) + ([] if scale_arg is None else ["-scale", scale_arg]) + DC.MODES[mode][1]
    status, pix = DC.djpeg_status(source(name), args)
    assert status == 0 and pix is not None, "djpeg %s exits with %d on %s" % (" ".join(args), status, name)
    return pix


def run(M, name, mode="default", **kw):
    out = M.decode([source(name)], **dict(DC.MODES[mode][0], **kw))[0]
    if isinstance(out, Exception):
        raise out
    return out


same = SC.same


# ---- the reference's TurboJPEG, for planes ----------------------------------------------------------------------------------------
class ScalingFactor(C.Structure):
    _fields_ = [("num", C.c_int), ("denom", C.c_int)]


_tj = None


def tj():
    global _tj
    if _tj is None:
        L = C.CDLL(TJLIB)
        L.tj3Init.restype = C.c_void_p
        L.tj3Init.argtypes = [C.c_int]
        L.tj3Destroy.argtypes = [C.c_void_p]
        L.tj3Get.argtypes = [C.c_void_p, C.c_int]
        L.tj3Set.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.tj3GetErrorStr.restype = C.c_char_p
        L.tj3GetErrorStr.argtypes = [C.c_void_p]
        L.tj3DecompressHeader.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        L.tj3SetScalingFactor.argtypes = [C.c_void_p, ScalingFactor]
        L.tj3DecompressToYUVPlanes8.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
        L.tj3YUVPlaneWidth.argtypes = [C.c_int] * 3
        L.tj3YUVPlaneHeight.argtypes = [C.c_int] * 3
        _tj = L
    return _tj


TJINIT_DECOMPRESS, TJPARAM_SUBSAMP, TJPARAM_JPEGWIDTH, TJPARAM_JPEGHEIGHT, TJPARAM_FASTDCT, TJSAMP_GRAY = 1, 4, 5, 6, 10, 3


@functools.lru_cache(maxsize=None)
def reference_planes(name, num, denom, fast=False):
    """the planes of the reference's tj3DecompressToYUVPlanes8 at num/denom (fast: with TJPARAM_FASTDCT), tight strides"""
    L = tj()
    src = source(name)
    h = L.tj3Init(TJINIT_DECOMPRESS)
    try:
        assert L.tj3DecompressHeader(h, src, len(src)) == 0, L.tj3GetErrorStr(h)
        sub, w, ht = (L.tj3Get(h, p) for p in (TJPARAM_SUBSAMP, TJPARAM_JPEGWIDTH, TJPARAM_JPEGHEIGHT))
        assert sub >= 0
        assert L.tj3SetScalingFactor(h, ScalingFactor(num, denom)) == 0
        assert L.tj3Set(h, TJPARAM_FASTDCT, int(fast)) == 0
        sw, sh = -(-w * num // denom), -(-ht * num // denom)
        planes = [np.full((L.tj3YUVPlaneHeight(c, sh, sub), L.tj3YUVPlaneWidth(c, sw, sub)), 0xA5, np.uint8) for c in range(1 if sub == TJSAMP_GRAY else 3)]
        ptrs = (C.c_void_p * 3)(*[p.ctypes.data for p in planes])
        assert L.tj3DecompressToYUVPlanes8(h, src, len(src), ptrs, None) == 0, L.tj3GetErrorStr(h)
        return planes
    finally:
        L.tj3Destroy(h)


# ---- the checks both test files make ------------------------------------------------------------------------------------------------
def check_case(M, name, mode):
    ref = reference(name, mode)
    out = run(M, name, mode, dct="fast")
    assert same(out, ref), "%s against the reference's %s" % (out.shape, ref.shape)
    assert same(run(M, name, mode, dct="int"), DC.djpeg(source(name), DC.MODES[mode][1]))


def check_fast_differs_from_slow(M, name):
    fast, slow = run(M, name, dct="fast"), run(M, name)
    assert fast.shape == slow.shape and not np.array_equal(fast, slow)
    assert not np.array_equal(reference(name, "default"), reference(name, "default", fast=False))


def check_scaled_case(M, name, sc):
    scale, arg, k = SC.SCALES[sc]
    ref = reference(name, "default", arg)
    out = run(M, name, scale=scale, dct="fast")
    assert same(out, ref), "%s against the reference's %s" % (out.shape, ref.shape)


def check_scaled_method_reaches_size_8_only(M):
    """4:2:0 at 1/2: chroma is at size 8 and the method shows; gray at 1/2: no component is, fast == slow"""
    info = M.jpeg_info(source("revert"))
    assert SC.dct_scaled_sizes(info, 4) == [4, 8, 8]
    assert not np.array_equal(run(M, "revert", scale="1/2", dct="fast"), run(M, "revert", scale="1/2"))
    assert same(run(M, "gray_r5b", scale="1/2", dct="fast"), run(M, "gray_r5b", scale="1/2"))
    assert same(reference("gray_r5b", "default", "4/8"), reference("gray_r5b", "default", "4/8", fast=False))


def check_bottom_up(M, kind, sc):
    scale, arg = (None, None) if sc is None else SC.SCALES[sc][:2]
    for dct in ("int", "fast"):
        ref = reference("revert", "grayscale" if kind == "gray" else "default", arg, fast=dct == "fast")
        out = run(M, "revert", scale=scale, dct=dct, bottom_up=True, **FLIP_KW[kind])
        up = run(M, "revert", scale=scale, dct=dct, **FLIP_KW[kind])
        assert same(out, up[::-1])
        if kind == "bgrx":
            DC.check_layout(ref[::-1], out, "bgrx")
        else:
            assert same(out, np.ascontiguousarray(ref[::-1]))


def check_planes(M, name, sc):
    scale, k = (None, 8) if sc is None else (SC.SCALES[sc][0], SC.SCALES[sc][2])
    for dct in (None, "int", "fast"):
        ref = reference_planes(name, 1, 8 // k, dct == "fast")
        out = M.decode_planes([source(name)], scale=scale, dct=dct)[0]
        if isinstance(out, Exception):
            raise out
        assert len(out) == len(ref)
        for c, (a, b) in enumerate(zip(out, ref)):
            assert same(a, b), "component %d: %s against the reference's %s" % (c, a.shape, b.shape)


def check_planes_of_a_file_without_tjsamp(M):
    """2x2,1x1,2x1 has no TJSAMP: the planes still come, of ceil() shapes"""
    src = source("s_mixed")
    info = M.jpeg_info(src)
    w, h = info.image_width, info.image_height
    for scale, k in ((None, 8), ("1/2", 4)):
        out = M.decode_planes([src], scale=scale)[0]
        sw, sh = -(-w * k // 8), -(-h * k // 8)
        pw, ph = -(-sw // 2) * 2, -(-sh // 2) * 2
        assert [p.shape for p in out] == [(ph, pw), (ph // 2, pw // 2), (ph // 2, pw)]
        assert all(p.dtype == np.uint8 for p in out)
    # at full size the luma plane is what the gray picture is made of
    full = M.decode_planes([src])[0]
    assert same(np.ascontiguousarray(full[0][:h, :w]), DC.reference("s_mixed", "grayscale"))


def check_one_encoder_serves_everything(M):
    src = source("revert")
    enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=1)
    slow, fast = DC.reference("revert", "default"), reference("revert", "default")
    for _ in range(2):
        assert same(enc.decode_host([src])[0], slow)
        assert same(enc.decode_host([src], dct="fast")[0], fast)
        planes = enc.decode_host([src], raw_planes=True, scale="1/2")[0]
        for a, b in zip(planes, reference_planes("revert", 1, 2)):
            assert same(a, b)
        assert same(enc.decode_host([src], dct="fast", bottom_up=True)[0], np.ascontiguousarray(fast[::-1]))
        assert same(enc.decode_host([src], dct="int", scale="1/8")[0], SC.reference("revert", "default", "1/8"))
    o = M.DecodeOpts()                                                # a zeroed struct means what it meant: slow, top-down, pixels
    assert (o.dct_method, o.bottom_up, o.raw_planes) == (0, 0, 0)
    assert same(enc.decode_host([src], opts=o)[0], DC.reference("revert", "nosmooth"))
    d = M.DecodeOpts()
    M.lib().mjh_decode_opts_defaults(d)
    assert (d.dct_method, d.bottom_up, d.raw_planes, d.fancy_upsampling) == (0, 0, 0, 1)
    enc.close()


def check_batch(M):
    files = DC.batch_files()
    singles = [M.decode([f], dct="fast")[0] for f in files]
    for f, s in zip(files, singles):
        assert same(s, DC.djpeg(f, ["-dct", "fast"]))
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True), max_batch=3)
    for o, s in zip(enc.decode_host(files, dct="fast"), singles):
        assert same(o, s)
    planes = enc.decode_host(files, raw_planes=True)
    for p, f in zip(planes, files):
        one = M.decode_planes([f])[0]
        assert all(same(a, b) for a, b in zip(p, one))
    enc.close()


def check_refusals(M):
    src = source("revert")
    enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=1)
    full = enc.decode_host([src])[0]
    for v in (2, 7, -1):
        o = SC.raw_opts(M, 1, 1)
        o.dct_method = v
        with SC.pytest_raises(M, M.EINVAL, "dct_method"):
            enc.decode_host([src], opts=o)
        with SC.pytest_raises(M, M.EINVAL, "dct"):
            M.decode([src], dct=v)
    with SC.pytest_raises(M, M.EINVAL, "dct"):
        M.decode([src], dct="float")
    L = M.lib()
    info = M.jpeg_info(src)
    # the pixel accessors after a raw_planes call, the plane accessor after a pixel call
    enc.decode_host([src], raw_planes=True)
    buf = np.zeros((info.image_height, info.image_width, 3), np.uint8)
    assert L.mjh_get_pixels(enc._h, 0, buf.ctypes.data, buf.strides[0]) == M.EINVAL and not buf.any()
    assert L.mjh_get_pixels_device(enc._h, None, None, None) == M.EINVAL
    base, pitch, stride, pw, ph = enc.planes_device(1)
    assert (pw, ph) == (8 * -(-info.image_width // 16), 8 * -(-info.image_height // 16)) and pitch >= pw and stride >= pitch * ph
    one = np.zeros((ph + 1, pw + 1), np.uint8)
    assert L.mjh_get_plane(enc._h, 0, 1, one.ctypes.data, one.strides[0], pw, ph) == M.OK
    for w, h in ((pw + 1, ph), (pw, ph + 1), (0, 1), (1, -1)):
        assert L.mjh_get_plane(enc._h, 0, 1, one.ctypes.data, one.strides[0], w, h) == M.EINVAL
    assert L.mjh_get_plane(enc._h, 0, 3, one.ctypes.data, one.strides[0], 1, 1) == M.EINVAL
    assert L.mjh_get_plane(enc._h, 1, 0, one.ctypes.data, one.strides[0], 1, 1) == M.EINVAL
    assert same(enc.decode_host([src])[0], full)
    assert L.mjh_get_plane(enc._h, 0, 0, one.ctypes.data, one.strides[0], 1, 1) == M.EINVAL
    assert L.mjh_get_planes_device(enc._h, 0, None, None, None, None, None) == M.EINVAL
    enc.close()
