"""Lossless JPEG (SOF3) test material shared by tests/test_simt_lossless.py, tests/test_gpu_lossless.py and the goldens generator
tests/golden/make_lossless_goldens.py: deterministic images, the reference's answer through `oracle/_ref/cjpeg -revert -lossless`
(built by oracle/Makefile), and the parameter sets of this library for the same switches."""
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CJPEG = os.path.join(ROOT, "oracle", "_ref", "cjpeg")


def image(kind, h, w, comps, precision, seed=0):
    """kind: "random" (full range noise), "flat" (one value), "smooth" (gradient + mild noise), "extreme" (columns alternating 0 and
    the maximum: with PSV 1 every difference is +-(2^P - 1), at 16 bits the difference 32768 mod 2^16 of category 16 comes with them)"""
    top = (1 << precision) - 1
    rs = np.random.RandomState(seed)
    shape = (h, w, comps)
    if kind == "random":
        a = rs.randint(0, top + 1, shape)
    elif kind == "flat":
        a = np.full(shape, rs.randint(0, top + 1))
    elif kind == "smooth":
        y, x = np.mgrid[0:h, 0:w]
        base = (x * 7 + y * 3)[..., None] * (top // 1024 + 1) + np.arange(comps) * (top // 5)
        a = np.clip(base + rs.randint(-(top // 64 + 1), top // 64 + 2, shape), 0, top)
    elif kind == "extreme":
        a = np.zeros(shape, np.int64)
        a[:, 1::2] = top
        if precision == 16 and w > 2:
            a[:, 2, 0] = 32768        # 65535 -> 32768: difference -32767; 32768 -> 0 at x = 3: -32768 (category 16)
            a[:, 3, 0] = 0
    else:
        raise ValueError(kind)
    return a.astype(np.uint8 if precision == 8 else np.uint16)


def write_pnm(path, a, precision):
    h, w, c = a.shape
    maxval = (1 << precision) - 1
    with open(path, "wb") as f:
        f.write(b"P%d\n%d %d\n%d\n" % (5 if c == 1 else 6, w, h, maxval))
        f.write(a.astype(">u2" if maxval > 255 else np.uint8).tobytes())


def cjpeg_args(psv, pt, precision, restart=None):
    args = ["-revert", "-lossless", "%d,%d" % (psv, pt)]
    if precision != 8:
        args += ["-precision", str(precision)]
    if restart is not None:
        args += ["-restart", str(restart)]
    return args


def reference(a, psv, pt, precision, restart=None, extra=()):
    """the reference's file, or (returncode, stderr) when it refuses"""
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "in.pnm")
        write_pnm(f, a, precision)
        r = subprocess.run([CJPEG] + cjpeg_args(psv, pt, precision, restart) + list(extra) + [f], capture_output=True)   # (-revert first: it resets every switch in front of it)
    if r.returncode != 0:
        return r.returncode, r.stderr.decode(errors="replace")
    return r.stdout


def params(M, a, psv, pt, precision, restart=None):
    h, w, c = a.shape
    return M.make_params(w, h, revert=True, lossless=(psv, pt), precision=precision, grayin=c == 1, restart=restart)


# the emulator slice: (kind, h, w, comps, precision, psv, pt, restart)
SIMT_CASES = [
    ("random", 1, 1, 3, 8, 1, 0, None),
    ("random", 1, 37, 1, 8, 2, 0, None),
    ("random", 53, 1, 3, 8, 3, 0, None),
    ("smooth", 29, 47, 3, 8, 4, 0, 1),
    ("random", 29, 47, 1, 8, 5, 7, 3),
    ("flat", 17, 23, 3, 8, 6, 1, None),
    ("smooth", 31, 1300, 3, 8, 7, 0, 4),
    ("smooth", 21, 33, 3, 12, 1, 0, None),
    ("random", 21, 33, 1, 12, 6, 11, 2),
    ("extreme", 9, 40, 1, 12, 7, 1, None),
    ("extreme", 11, 41, 3, 16, 1, 0, None),
    ("extreme", 11, 41, 1, 16, 1, 0, 1),
    ("random", 19, 25, 3, 16, 4, 15, None),
    ("smooth", 19, 25, 1, 16, 6, 3, 5),
]


def case_id(c):
    kind, h, w, comps, prec, psv, pt, rst = c
    return "%s-%dx%dx%d-p%d-psv%d-pt%d-r%s" % (kind, w, h, comps, prec, psv, pt, rst)


# ---- the reference's TurboJPEG library (oracle/_ref/libturbojpeg.so.0), tj3 API with TJPARAM_LOSSLESS* ------------------------------
TJLIB = os.path.join(ROOT, "oracle", "_ref", "libturbojpeg.so.0")
TJPARAM_NOREALLOC, TJPARAM_LOSSLESS, TJPARAM_LOSSLESSPSV, TJPARAM_LOSSLESSPT, TJPARAM_RESTARTROWS = 2, 15, 16, 17, 19
TJPF = {"RGB": 0, "BGR": 1, "RGBX": 2, "BGRX": 3, "XBGR": 4, "XRGB": 5, "GRAY": 6}
TJPF_LAYOUT = {"RGB": (3, (0, 1, 2)), "BGR": (3, (2, 1, 0)), "RGBX": (4, (0, 1, 2)), "BGRX": (4, (2, 1, 0)),
               "XBGR": (4, (3, 2, 1)), "XRGB": (4, (1, 2, 3))}
_tj = None


def tj():
    global _tj
    if _tj is None:
        import ctypes as C
        L = C.CDLL(TJLIB)
        L.tj3Init.restype = C.c_void_p
        L.tj3Init.argtypes = [C.c_int]
        L.tj3Set.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.tj3Get.argtypes = [C.c_void_p, C.c_int]
        L.tj3Destroy.argtypes = [C.c_void_p]
        L.tj3Free.argtypes = [C.c_void_p]
        L.tj3GetErrorStr.restype = C.c_char_p
        L.tj3GetErrorStr.argtypes = [C.c_void_p]
        for f in (L.tj3Compress8, L.tj3Compress12, L.tj3Compress16):
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        _tj = L
    return _tj


def tj_compress(a, psv, pt, precision, pixel_format, restart_rows=0, handle=None):
    """one lossless file from the reference's TurboJPEG (setCompDefaults turbojpeg.c:346-355); a: [H, W, samples per pixel]"""
    import ctypes as C
    L = tj()
    h = handle or L.tj3Init(0)
    try:
        for prm, v in ((TJPARAM_LOSSLESS, 1), (TJPARAM_LOSSLESSPSV, psv), (TJPARAM_LOSSLESSPT, pt), (TJPARAM_RESTARTROWS, restart_rows)):
            if L.tj3Set(h, prm, v) != 0:
                raise RuntimeError(L.tj3GetErrorStr(h).decode())
        a = np.ascontiguousarray(a)
        buf, size = C.c_void_p(), C.c_size_t()
        fn = {8: L.tj3Compress8, 12: L.tj3Compress12, 16: L.tj3Compress16}[precision]
        if fn(h, a.ctypes.data, a.shape[1], a.strides[0] // a.itemsize, a.shape[0], TJPF[pixel_format], C.byref(buf), C.byref(size)) != 0:
            raise RuntimeError(L.tj3GetErrorStr(h).decode())
        out = C.string_at(buf, size.value)
        L.tj3Free(buf)
        return out
    finally:
        if handle is None:
            L.tj3Destroy(h)
