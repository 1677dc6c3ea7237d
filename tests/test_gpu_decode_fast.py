"""GPU (-m gpu): the fast integer IDCT on the chip (mjh_decode_opts.dct_method 1, djpeg -dct fast: k_idct_ifast of mjh_idct.hip),
bottom-up rows in k_upcolor and raw sample planes.  Expected pixels come from the reference's djpeg -dct fast, expected planes
from its TurboJPEG library, at test time; every comparison is exact equality, the array shape included
(tests/fast_idct_cases.py).  The hostile-input cases run on the emulator only (test_simt_decode_fast.py)."""
import numpy as np
import pytest

import mozjpeg_amd as M
import decode_cases as DC
import fast_idct_cases as FC

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not FC.have_tools(), reason="reference cjpeg / djpeg / libturbojpeg not built (oracle/_ref)")]


@pytest.mark.parametrize("src,mode", FC.CASES, ids=[FC.case_id(c) for c in FC.CASES])
def test_fast_decode_matches_djpeg(src, mode):
    FC.check_case(M, src, mode)


@pytest.mark.parametrize("src", FC.MUST_DIFFER)
def test_fast_and_slow_pictures_differ(src):
    FC.check_fast_differs_from_slow(M, src)


@pytest.mark.parametrize("src,sc", FC.SCALED_CASES, ids=[FC.case_id(c) for c in FC.SCALED_CASES])
def test_fast_scaled_decode_matches_djpeg(src, sc):
    FC.check_scaled_case(M, src, sc)


def test_scaled_method_reaches_size_8_only():
    FC.check_scaled_method_reaches_size_8_only(M)


@pytest.mark.parametrize("kind,sc", FC.FLIP_CASES, ids=[FC.case_id(c) for c in FC.FLIP_CASES])
def test_bottom_up(kind, sc):
    FC.check_bottom_up(M, kind, sc)


@pytest.mark.parametrize("src,sc", FC.PLANE_CASES, ids=[FC.case_id(c) for c in FC.PLANE_CASES])
def test_planes_match_turbojpeg(src, sc):
    FC.check_planes(M, src, sc)


def test_planes_of_a_file_without_tjsamp():
    FC.check_planes_of_a_file_without_tjsamp(M)


def test_one_encoder_serves_everything():
    FC.check_one_encoder_serves_everything(M)


def test_batch_equals_single_files():
    FC.check_batch(M)


def test_refusals():
    FC.check_refusals(M)


class _DeviceView:
    """a device buffer of the encoder as an object torch can wrap without a copy"""

    def __init__(self, ptr, shape, strides):
        self.__cuda_array_interface__ = dict(shape=shape, strides=strides, typestr="|u1", data=(ptr, False), version=2)


def test_torch_views_of_bottom_up_pixels_and_planes():
    """callers who stay on the device: the flipped rows are in mjh_get_pixels_device's buffer, the planes in mjh_get_planes_device's"""
    import torch
    files = DC.batch_files()
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True), max_batch=3)
    enc.submit_decode(files, dct="fast", bottom_up=True)
    enc.wait_decode()
    ptr, pitch, stride, st = enc.pixels_device()
    h, w = st["height"], st["width"]
    got = torch.as_tensor(_DeviceView(ptr, (3, h, w, 3), (stride, pitch, 3, 1)), device="cuda:0").cpu().numpy()
    for i, f in enumerate(files):
        assert np.array_equal(got[i], DC.djpeg(f, ["-dct", "fast"])[::-1])
    host = enc.decode_host(files, raw_planes=True, scale="1/2")
    enc.wait_decode()
    for c in range(3):
        ptr, pitch, stride, pw, ph = enc.planes_device(c)
        got = torch.as_tensor(_DeviceView(ptr, (3, ph, pw), (stride, pitch, 1)), device="cuda:0").cpu().numpy()
        for i in range(3):
            a = host[i][c]
            assert np.array_equal(got[i, :a.shape[0], :a.shape[1]], a)
    enc.close()
