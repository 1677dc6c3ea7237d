"""Lossless JPEG through the TurboJPEG-signature library (mozjpeg_amd/libmozjpeg_hip_turbojpeg.so): tj3Set / tj3Get of
TJPARAM_LOSSLESS, TJPARAM_LOSSLESSPSV, TJPARAM_LOSSLESSPT with the reference's ranges (turbojpeg.c:745-758), lossless
tj3Compress8 / tj3Compress12 / tj3Compress16 byte for byte against the reference's libturbojpeg.so.0 (oracle/_ref), and the calls the
reference refuses.  The library runs the real device library: under --simt this file skips itself (the conftest's skip list goes by
file name)."""
import ctypes as C
import os

import numpy as np
import pytest

import mozjpeg_amd as M
import lossless_cases as LC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TJSHIM = os.path.join(ROOT, "mozjpeg_amd", "libmozjpeg_hip_turbojpeg.so")
TJPARAM_QUALITY, TJPARAM_SUBSAMP, TJPARAM_ARITHMETIC = 3, 4, 14


@pytest.fixture(scope="module")
def shim():
    if "simt" in os.path.basename(M.LIB_PATH or ""):
        pytest.skip("the TurboJPEG-signature library is linked to the device library, not to the emulator")
    L = C.CDLL(TJSHIM)
    L.tj3Init.restype = C.c_void_p
    L.tj3Init.argtypes = [C.c_int]
    L.tj3Set.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.tj3Get.argtypes = [C.c_void_p, C.c_int]
    L.tj3Destroy.argtypes = [C.c_void_p]
    L.tj3GetErrorStr.restype = C.c_char_p
    L.tj3GetErrorStr.argtypes = [C.c_void_p]
    for f in (L.tj3Compress8, L.tj3Compress12, L.tj3Compress16):
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    return L


def _compress(L, h, a, prec, fmt):
    buf, size = C.c_void_p(), C.c_size_t()
    fn = {8: L.tj3Compress8, 12: L.tj3Compress12, 16: L.tj3Compress16}[prec]
    a = np.ascontiguousarray(a)
    rc = fn(h, a.ctypes.data, a.shape[1], a.strides[0] // a.itemsize, a.shape[0], LC.TJPF[fmt], C.byref(buf), C.byref(size))
    if rc != 0:
        return None
    out = C.string_at(buf, size.value)
    C.CDLL(None).free(buf)          # (the library hands over malloc'd memory, as tj3Alloc does)
    return out


def _set(L, h, psv, pt, rows=0):
    for prm, v in ((LC.TJPARAM_LOSSLESS, 1), (LC.TJPARAM_LOSSLESSPSV, psv), (LC.TJPARAM_LOSSLESSPT, pt), (LC.TJPARAM_RESTARTROWS, rows)):
        assert L.tj3Set(h, prm, v) == 0


def test_tj_lossless_parameter_ranges(shim):
    h = shim.tj3Init(0)
    ref = LC.tj()
    r = ref.tj3Init(0)
    try:
        for prm, vals in ((LC.TJPARAM_LOSSLESS, (-1, 0, 1, 2)), (LC.TJPARAM_LOSSLESSPSV, (0, 1, 7, 8)), (LC.TJPARAM_LOSSLESSPT, (-1, 0, 15, 16))):
            assert shim.tj3Get(h, prm) == ref.tj3Get(r, prm)           # defaults: 0 / 1 / 0 (turbojpeg.c:560)
            for v in vals:
                assert (shim.tj3Set(h, prm, v) == 0) == (ref.tj3Set(r, prm, v) == 0), (prm, v)
                assert shim.tj3Get(h, prm) == ref.tj3Get(r, prm), (prm, v)
    finally:
        shim.tj3Destroy(h)
        ref.tj3Destroy(r)


@pytest.mark.parametrize("prec", [8, 12, 16])
@pytest.mark.parametrize("fmt", ["RGB", "BGRX", "XRGB", "GRAY"])
def test_tj_lossless_matches_reference(shim, prec, fmt):
    """no TJPARAM_QUALITY / TJPARAM_SUBSAMP set: lossless needs neither (turbojpeg-mp.c:89-92)"""
    px, off = LC.TJPF_LAYOUT.get(fmt, (1, (0,)))
    a = LC.image("smooth", 57, 75, px, prec, seed=prec)
    h = shim.tj3Init(0)
    try:
        for psv, pt, rows in ((1, 0, 0), (4, 1, 2), (7, prec - 1, 0), (6, 0, 5)):
            _set(shim, h, psv, pt, rows)
            got = _compress(shim, h, a, prec, fmt)
            assert got is not None, shim.tj3GetErrorStr(h)
            assert got == LC.tj_compress(a, psv, pt, prec, fmt, rows), (psv, pt, rows)
    finally:
        shim.tj3Destroy(h)


def test_tj_refusals_match_the_reference(shim):
    a8 = LC.image("random", 8, 10, 3, 8)
    a16 = LC.image("random", 8, 10, 3, 16)
    ref = LC.tj()
    for setup, a, prec in (("pt_ge_precision", a8, 8), ("lossy16", a16, 16)):
        results = []
        for L in (shim, ref):
            h = L.tj3Init(0)
            if setup == "lossy16":
                L.tj3Set(h, TJPARAM_QUALITY, 90)
                L.tj3Set(h, TJPARAM_SUBSAMP, 0)
            else:
                _set(L, h, 1, 9)
            buf, size = C.c_void_p(), C.c_size_t()
            fn = L.tj3Compress16 if prec == 16 else L.tj3Compress8
            results.append(fn(h, a.ctypes.data, a.shape[1], a.shape[1] * 3, a.shape[0], LC.TJPF["RGB"], C.byref(buf), C.byref(size)))
            L.tj3Destroy(h)
        assert results[0] != 0 and results[1] != 0, (setup, results)


def test_tj_lossless_ignores_arithmetic(shim):
    """setCompDefaults returns in front of arith_code / optimize / progressive in lossless mode (turbojpeg.c:346-385)"""
    a = LC.image("smooth", 20, 30, 3, 8)
    h = shim.tj3Init(0)
    try:
        _set(shim, h, 2, 0)
        assert shim.tj3Set(h, TJPARAM_ARITHMETIC, 1) == 0
        assert _compress(shim, h, a, 8, "RGB") == LC.tj_compress(a, 2, 0, 8, "RGB")
    finally:
        shim.tj3Destroy(h)
