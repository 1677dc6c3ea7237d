"""GPU (-m gpu): decoding JPEG files to pixels on the chip (mjh_decode_host: the Huffman decoder of mjh_decode.hip, then the pixel kernels
of mjh_idct.hip).  Every expected pixel comes from the reference's djpeg (oracle/_ref/djpeg -pnm + switches) at test time and is compared
for exact equality.  The untrusted-input cases (truncation, bit flips) run on the emulator only (test_simt_decode.py)."""
import random

import numpy as np
import pytest

import mozjpeg_amd as M
import oracle_lib as O
import decode_cases as DC
import transcode_cases as TC

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not DC.have_tools(), reason="reference cjpeg / jpegtran / djpeg not built (oracle/_ref)")]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("src,mode", DC.ALL_PAIRS, ids=["%s-%s" % p for p in DC.ALL_PAIRS])
def test_decode_matches_djpeg(src, mode):
    ref = DC.reference(src, mode)
    out = DC.run_pair(M, src, mode)
    assert same(out, ref), "%s, the reference %s" % (out.shape, ref.shape)


def test_every_upsampler_is_reached():
    used = set()
    for src, mode in DC.ALL_PAIRS:
        used |= DC.upsamplers(M.jpeg_info(DC.source(src)), mode, M.CS_GRAYSCALE, M.CS_YCBCR)
    assert used == DC.ALL_UPSAMPLERS, "not reached: %s" % sorted(DC.ALL_UPSAMPLERS - used)


@pytest.mark.parametrize("src", ["revert", "rgb", "gray_r5b", "17x9"])
def test_extended_layouts(src):
    rgb = DC.reference(src, "rgb")
    for layout in DC.LAYOUT_ORDER:
        out = M.decode([DC.source(src)], color="rgb", layout=layout)[0]
        DC.check_layout(rgb, out, layout)


def test_range_limit_wrap():
    src = DC.wrap_source()
    for mode in DC.MODES:
        status, ref = DC.djpeg_status(src, DC.MODES[mode][1])
        assert status == 0, "djpeg exits with %d on the patched file" % status
        enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=1)
        out = enc.decode_host([src], **DC.MODES[mode][0])[0]
        wrapped = DC.wrapped_samples(M, enc, src)
        enc.close()
        assert wrapped > 0, "no sample of the file leaves the clamp region: the case proves nothing"
        assert same(out, ref), mode


SUBSEQ_SOURCES = ["revert", "q90_2x1_r1", "gray_r5b", "scans3_2x2_r2", "rgb", "oracle_baseline", "s_mixed", "noise_q100", "17x9"]


@pytest.mark.parametrize("S", [0, None])
def test_subsequence_length_changes_nothing(monkeypatch, S):
    if S is None:
        monkeypatch.delenv("MJH_DECODE_SUBSEQ", raising=False)
    else:
        monkeypatch.setenv("MJH_DECODE_SUBSEQ", str(S))
    for src in SUBSEQ_SOURCES:
        enc = M.Encoder(M.params_from_jpeg(DC.source(src), revert=True), max_batch=1)
        out = enc.decode_host([DC.source(src)])[0]
        st = enc.transcode_stats()
        enc.close()
        if S is not None:
            assert st["subseq"] == S
        assert same(out, DC.reference(src, "default")), "%s S=%s" % (src, S)


@pytest.mark.parametrize("mode", ["default", "nosmooth"])
def test_batch_of_different_files(mode):
    files = DC.batch_files()
    kw, args = DC.MODES[mode]
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True), max_batch=3)
    outs = enc.decode_host(files, **kw)
    for f, o in zip(files, outs):
        assert same(o, DC.djpeg(f, args))
        assert same(o, enc.decode_host([f], **kw)[0])
    enc.close()


def test_decode_keeps_input_order():
    names = ["revert", "gray_r5b", "8x8", "revert_opt", "rgb", "17x9", "jfif102", "s1x2", "1x1", "noise_q100", "scans3_2x2_r2", "revert",
             "s4x1", "s_h1v2_h2v1", "33x47"]
    random.Random(5).shuffle(names)
    for mode in ("default", "grayscale"):
        outs = M.decode([DC.source(s) for s in names], max_batch=4, **DC.MODES[mode][0])
        for s, o in zip(names, outs):
            assert same(o, DC.reference(s, mode)), "%s %s" % (s, mode)


@pytest.mark.parametrize("what", list(TC.REFUSALS))
def test_refused_sources(what):
    args, word = TC.REFUSALS[what]
    src = TC.cjpeg(TC.testorig(), args)
    r = M.decode([src, TC.source("revert")])
    assert isinstance(r[0], M.MjhError) and r[0].code == M.EUNSUPPORTED and word in str(r[0])
    assert same(r[1], DC.reference("revert", "default"))


def test_transform_with_decode_and_bad_options_are_refused():
    """on fresh encoders and after a batch with a damaged file: the refusal is the call's own, whatever ran before"""
    src = TC.source("revert")
    enc = M.Encoder(M.params_from_jpeg(src, revert=True, transform="flip_h"), max_batch=1)
    with pytest.raises(M.MjhError) as ei:
        enc.decode_host([src])
    assert ei.value.code == M.EUNSUPPORTED
    enc.close()
    M._decode_encoders.clear()
    for kw in (dict(color=7), dict(pixel_size=2), dict(color="gray", pixel_size=3)):
        with pytest.raises(M.MjhError) as ei:
            M.decode([src], **kw)
        assert ei.value.code == M.EINVAL, kw
    info = M.jpeg_info(src)
    a, n = info.scans[0].data_offset, info.scans[0].data_size
    bad = src[:a + n // 2] + src[a + n // 2 + 40:]
    for damaged_first in (False, True):
        enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=2)
        if damaged_first:
            res = enc.decode_host([src, bad], errors="return")
            assert res[0] is None and isinstance(res[1], M.MjhError)
            with pytest.raises(M.MjhError):
                enc.wait_decode()
        o = M.DecodeOpts()
        M.lib().mjh_decode_opts_defaults(o)
        o.pixel_size = 2                                # (past the binding's own check: what a C caller could pass)
        for errors in ("raise", "return"):
            with pytest.raises(M.MjhError) as ei:
                enc.decode_host([src], errors=errors, opts=o)
            assert ei.value.code == M.EINVAL and "pixel_size" in str(ei.value)
        assert same(enc.decode_host([src])[0], DC.reference("revert", "default"))
        enc.close()


class _DeviceView:
    """the encoder's pixel buffer as an object torch can wrap without a copy"""

    def __init__(self, ptr, shape, strides):
        self.__cuda_array_interface__ = dict(shape=shape, strides=strides, typestr="|u1", data=(ptr, False), version=2)


@pytest.mark.parametrize("kw", [dict(), dict(layout="bgrx"), dict(color="gray")], ids=["rgb", "bgrx", "gray"])
def test_device_buffer_through_torch(kw):
    import torch
    files = DC.batch_files()
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True), max_batch=3)
    host = enc.decode_host(files, **kw)
    enc.submit_decode(files, **kw)                      # once more, without touching the host path: wait, then read the device buffer
    enc.wait_decode()
    ptr, pitch, stride, st = enc.pixels_device()
    h, w, px = st["height"], st["width"], st["pixel_size"]
    assert pitch >= w * px and stride >= pitch * h
    t = torch.as_tensor(_DeviceView(ptr, (3, h, w, px), (stride, pitch, px, 1)), device="cuda:0")
    assert t.is_cuda and t.data_ptr() == ptr
    got = t.cpu().numpy()
    for i in range(3):
        assert np.array_equal(got[i] if px > 1 else got[i, :, :, 0], host[i])
    enc.close()


def test_full_size_batch():
    """8 distinct 4K 4:2:0 q75 files in one call, with and without fancy upsampling"""
    files = [TC.cjpeg(O.synthetic_frame(3840, 2160, seed=100 + i), ["-revert", "-quality", "75", "-sample", "2x2"]) for i in range(8)]
    assert len(set(files)) == 8
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True), max_batch=8)
    for mode in ("default", "nosmooth"):
        kw, args = DC.MODES[mode]
        outs = enc.decode_host(files, **kw)
        for i, (f, o) in enumerate(zip(files, outs)):
            assert same(o, DC.djpeg(f, args)), "file %d, %s" % (i, mode)
    enc.close()


def test_many_small_files_in_one_call():
    """256 files of 320 x 240 in one call"""
    w, h = 320, 240
    big = O.synthetic_frame(1280, 960, seed=9)
    rng = random.Random(w)
    files = []
    for i in range(256):
        x, y = rng.randrange(0, 1280 - w), rng.randrange(0, 960 - h)
        files.append(TC.cjpeg(big[y:y + h, x:x + w], ["-revert", "-quality", "75", "-sample", "2x2"] + (["-restart", "1"] if i % 7 == 3 else [])))
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True), max_batch=256)
    outs = enc.decode_host(files)
    enc.close()
    for i, (f, o) in enumerate(zip(files, outs)):
        assert same(o, DC.djpeg(f)), "file %d" % i
