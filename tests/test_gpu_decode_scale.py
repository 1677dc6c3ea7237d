"""GPU (-m gpu): decoding JPEG files at reduced size on the chip (mjh_decode_host with scale_num / scale_denom, djpeg -scale 1/2,
1/4, 1/8: k_idct_scaled of mjh_idct.hip, then k_upcolor on the reduced planes).  Every expected pixel comes from the reference's
djpeg -scale at test time and is compared for exact equality, the array shape included (tests/scale_cases.py).  The
untrusted-input cases run on the emulator only (test_simt_decode_scale.py)."""
import numpy as np
import pytest

import mozjpeg_amd as M
import oracle_lib as O
import decode_cases as DC
import scale_cases as SC
import transcode_cases as TC

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not SC.have_tools(), reason="reference cjpeg / jpegtran / djpeg not built (oracle/_ref)")]


@pytest.mark.parametrize("src,mode,sc", SC.CASES, ids=[SC.case_id(c) for c in SC.CASES])
def test_scaled_decode_matches_djpeg(src, mode, sc):
    SC.check_case(M, src, mode, sc)


@pytest.mark.parametrize("src,layout,sc", SC.LAYOUT_CASES, ids=[SC.case_id(c) for c in SC.LAYOUT_CASES])
def test_scaled_four_byte_layout(src, layout, sc):
    SC.check_layout_case(M, src, layout, sc)


@pytest.mark.parametrize("src,frac", SC.FRACTION_CASES, ids=[SC.case_id(c) for c in SC.FRACTION_CASES])
def test_fraction_is_resolved_as_djpeg_does(src, frac):
    SC.check_fraction(M, src, frac)


def test_every_transform_size_is_reached():
    SC.check_every_transform_size_is_reached(M)


def test_one_encoder_serves_every_scale():
    SC.check_one_encoder_serves_every_scale(M)


def test_mixed_batch_with_a_damaged_file():
    SC.check_mixed_batch(M)


def test_refusals():
    SC.check_refusals(M)


class _DeviceView:
    """the encoder's pixel buffer as an object torch can wrap without a copy"""

    def __init__(self, ptr, shape, strides):
        self.__cuda_array_interface__ = dict(shape=shape, strides=strides, typestr="|u1", data=(ptr, False), version=2)


@pytest.mark.parametrize("sc", list(SC.SCALES))
@pytest.mark.parametrize("kw", [dict(), dict(layout="bgrx"), dict(color="gray")], ids=["rgb", "bgrx", "gray"])
def test_device_buffer_addresses_the_scaled_image(kw, sc):
    """mjh_get_pixels_device against mjh_get_pixels: pitch and stride of the scaled rows, padded by the full-size rules"""
    import torch
    scale, arg, k = SC.SCALES[sc]
    files = DC.batch_files()
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True), max_batch=3)
    host = enc.decode_host(files, scale=scale, **kw)
    enc.submit_decode(files, scale=scale, **kw)
    enc.wait_decode()
    ptr, pitch, stride, st = enc.pixels_device()
    h, w, px = st["height"], st["width"], st["pixel_size"]
    info = M.jpeg_info(files[0])
    assert (h, w) == (-(-info.image_height * k // 8), -(-info.image_width * k // 8))
    assert pitch == (px * ((w + 3) & ~3) + 15) & ~15 and stride == pitch * h
    t = torch.as_tensor(_DeviceView(ptr, (3, h, w, px), (stride, pitch, px, 1)), device="cuda:0")
    got = t.cpu().numpy()
    for i in range(3):
        assert np.array_equal(got[i] if px > 1 else got[i, :, :, 0], host[i])
        if not kw:
            assert SC.same(host[i], DC.djpeg(files[i], ["-scale", arg]))
    enc.close()


def test_full_size_batch_at_every_scale():
    """4 distinct 4K 4:2:0 q75 files in one call at 1/2, 1/4 and 1/8, then at full size on the same encoder"""
    files = [TC.cjpeg(O.synthetic_frame(3840, 2160, seed=100 + i), ["-revert", "-quality", "75", "-sample", "2x2"]) for i in range(4)]
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True), max_batch=4)
    for sc, (scale, arg, k) in SC.SCALES.items():
        outs = enc.decode_host(files, scale=scale)
        for i, (f, o) in enumerate(zip(files, outs)):
            assert SC.same(o, DC.djpeg(f, ["-scale", arg])), "file %d at %s" % (i, sc)
    outs = enc.decode_host(files)
    for i, (f, o) in enumerate(zip(files, outs)):
        assert SC.same(o, DC.djpeg(f)), "file %d at full size" % i
    enc.close()
