"""CPU suite: the fast integer IDCT (mjh_decode_opts.dct_method 1, djpeg -dct fast: k_idct_ifast of mjh_idct.hip), bottom-up rows
and raw sample planes, with the kernels executed by the lock-step wave64 emulator (tools/simt, SIMT_STRICT), whose device buffers
end at unmapped pages.  Expected pixels come from the reference's djpeg -dct fast, expected planes from its TurboJPEG library, at
test time; every comparison is exact equality, the array shape included (tests/fast_idct_cases.py)."""
import os
import sys

import numpy as np
import pytest

import mozjpeg_amd as M
import decode_cases as DC
import fast_idct_cases as FC
import scale_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "simt"))

pytestmark = pytest.mark.skipif(not FC.have_tools(), reason="reference cjpeg / djpeg / libturbojpeg not built (oracle/_ref)")


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


@pytest.mark.parametrize("src,mode", FC.CASES, ids=[FC.case_id(c) for c in FC.CASES])
def test_fast_decode_matches_djpeg(simt, src, mode):
    FC.check_case(M, src, mode)


@pytest.mark.parametrize("src", FC.MUST_DIFFER)
def test_fast_and_slow_pictures_differ(simt, src):
    FC.check_fast_differs_from_slow(M, src)


@pytest.mark.parametrize("src,sc", FC.SCALED_CASES, ids=[FC.case_id(c) for c in FC.SCALED_CASES])
def test_fast_scaled_decode_matches_djpeg(simt, src, sc):
    FC.check_scaled_case(M, src, sc)


def test_scaled_method_reaches_size_8_only(simt):
    FC.check_scaled_method_reaches_size_8_only(M)


@pytest.mark.parametrize("kind,sc", FC.FLIP_CASES, ids=[FC.case_id(c) for c in FC.FLIP_CASES])
def test_bottom_up(simt, kind, sc):
    FC.check_bottom_up(M, kind, sc)


@pytest.mark.parametrize("src,sc", FC.PLANE_CASES, ids=[FC.case_id(c) for c in FC.PLANE_CASES])
def test_planes_match_turbojpeg(simt, src, sc):
    FC.check_planes(M, src, sc)


def test_planes_of_a_file_without_tjsamp(simt):
    FC.check_planes_of_a_file_without_tjsamp(M)


def test_one_encoder_serves_everything(simt):
    FC.check_one_encoder_serves_everything(M)


def test_batch_equals_single_files(simt):
    FC.check_batch(M)


def test_refusals(simt):
    FC.check_refusals(M)


# ---- hostile input, emulator only -----------------------------------------------------------------------------------------------------
def test_absurd_quantization_under_the_fast_method(simt):
    """every quantization step 65535: the reference's int sums overflow (undefined behaviour there, a wrap here), so the pixels are
    not compared; the call completes with a picture of the right shape and faults nowhere.  Under dct="int" nothing changes."""
    src = SC.absurd_quant()
    info = M.jpeg_info(src)
    for scale, k in ((None, 8), ("1/2", 4), ("1/8", 1)):
        out = M.decode([src], dct="fast", scale=scale)[0]
        assert isinstance(out, np.ndarray) and out.dtype == np.uint8
        assert out.shape == (-(-info.image_height * k // 8), -(-info.image_width * k // 8), 3)
    assert SC.same(M.decode([src], dct="int")[0], DC.djpeg(src))
    assert SC.same(M.decode([src])[0], DC.djpeg(src))
    planes = M.decode_planes([src], dct="fast")[0]
    assert len(planes) == 3


def test_truncated_file_under_the_fast_method(simt):
    src = FC.source("revert")
    info = M.jpeg_info(src)
    a, n = info.scans[0].data_offset, info.scans[0].data_size
    cut = src[:a + n // 2]
    slow, fast = M.decode([cut])[0], M.decode([cut], dct="fast")[0]
    assert isinstance(slow, M.MjhError) and isinstance(fast, M.MjhError)
    assert (fast.code, str(fast)) == (slow.code, str(slow)) and fast.code == M.EINVAL
    planes = M.decode_planes([cut], dct="fast")[0]
    assert isinstance(planes, M.MjhError) and planes.code == M.EINVAL
    assert SC.same(M.decode([src], dct="fast")[0], FC.reference("revert", "default"))
