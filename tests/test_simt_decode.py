"""CPU suite: decoding JPEG files to pixels (mjh_decode_host) with the Huffman decoder kernels of mjh_decode.hip and the pixel kernels of
mjh_idct.hip executed by the lock-step wave64 emulator (tools/simt, SIMT_STRICT).  Every expected pixel comes from the reference's
djpeg (oracle/_ref/djpeg -pnm + switches) at test time and is compared for exact equality; sources are made at test time as well
(tests/decode_cases.py)."""
import os
import random
import sys

import numpy as np
import pytest

import mozjpeg_amd as M
import decode_cases as DC
import transcode_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "simt"))

pytestmark = pytest.mark.skipif(not DC.have_tools(), reason="reference cjpeg / jpegtran / djpeg not built (oracle/_ref)")


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


@pytest.fixture
def subseq(monkeypatch):
    def set_(s):
        if s is None:
            monkeypatch.delenv("MJH_DECODE_SUBSEQ", raising=False)
        else:
            monkeypatch.setenv("MJH_DECODE_SUBSEQ", str(s))
    return set_


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


# ---- 1. pixels == djpeg's, every source under every mode ----------------------------------------------------------------------
@pytest.mark.parametrize("src,mode", DC.ALL_PAIRS, ids=["%s-%s" % p for p in DC.ALL_PAIRS])
def test_decode_matches_djpeg(simt, src, mode):
    ref = DC.reference(src, mode)
    out = DC.run_pair(M, src, mode)
    assert same(out, ref), "%s, the reference %s" % (out.shape, ref.shape)


def test_every_upsampler_is_reached(simt):
    used = set()
    for src, mode in DC.ALL_PAIRS:
        used |= DC.upsamplers(M.jpeg_info(DC.source(src)), mode, M.CS_GRAYSCALE, M.CS_YCBCR)
    assert used == DC.ALL_UPSAMPLERS, "not reached: %s" % sorted(DC.ALL_UPSAMPLERS - used)
    # the small images take the plain functions under fancy upsampling (downsampled_width <= 2)
    assert "h2v2_upsample" in DC.upsamplers(M.jpeg_info(DC.source("1x1")), "default")


# ---- 2. extended pixel layouts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", ["revert", "rgb", "gray_r5b", "17x9"])
def test_extended_layouts(simt, src):
    rgb = DC.reference(src, "rgb")
    for layout in DC.LAYOUT_ORDER:
        out = M.decode([DC.source(src)], color="rgb", layout=layout)[0]
        DC.check_layout(rgb, out, layout)


# ---- 3. the wrap of the range-limit table -------------------------------------------------------------------------------------
def test_range_limit_wrap(simt):
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


# ---- 4. subsequence lengths ---------------------------------------------------------------------------------------------------
SUBSEQ_SOURCES = ["revert", "q90_2x1_r1", "gray_r5b", "scans3_2x2_r2", "rgb", "oracle_baseline", "s_mixed", "noise_q100", "17x9"]


@pytest.mark.parametrize("S", [0, 16, 64])
def test_subsequence_length_changes_nothing(simt, subseq, S):
    subseq(S)
    for src in SUBSEQ_SOURCES:
        enc = M.Encoder(M.params_from_jpeg(DC.source(src), revert=True), max_batch=1)
        out = enc.decode_host([DC.source(src)])[0]
        st = enc.transcode_stats()
        enc.close()
        assert st["subseq"] == S
        assert same(out, DC.reference(src, "default")), "%s S=%d" % (src, S)


# ---- 5. batches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "nosmooth"])
def test_batch_of_different_files(simt, mode):
    files = DC.batch_files()
    kw, args = DC.MODES[mode]
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True), max_batch=3)
    outs = enc.decode_host(files, **kw)
    for f, o in zip(files, outs):
        assert same(o, DC.djpeg(f, args))
        assert same(o, enc.decode_host([f], **kw)[0])
    enc.close()


def test_decode_keeps_input_order(simt):
    names = ["revert", "gray_r5b", "8x8", "revert_opt", "rgb", "17x9", "jfif102", "s1x2", "1x1", "noise_q100", "scans3_2x2_r2", "revert",
             "s4x1", "s_h1v2_h2v1", "33x47"]
    random.Random(5).shuffle(names)
    for mode in ("default", "grayscale"):
        outs = M.decode([DC.source(s) for s in names], max_batch=4, **DC.MODES[mode][0])
        for s, o in zip(names, outs):
            assert same(o, DC.reference(s, mode)), "%s %s" % (s, mode)


# ---- 6. untrusted input (the emulator's device buffers end at unmapped pages) -----------------------------------------------------
def test_truncated_files_fail(simt):
    src = TC.source("revert")
    info = M.jpeg_info(src)
    a, n = info.scans[0].data_offset, info.scans[0].data_size
    enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=1)
    cuts = list(range(a, a + n, 97))
    assert len(cuts) > 20
    for cut in cuts:
        with pytest.raises(M.MjhError) as ei:
            enc.decode_host([src[:cut]])
        assert ei.value.code == M.EINVAL
    for cut in cuts[1::4]:
        with pytest.raises(M.MjhError) as ei:
            enc.decode_host([src[:cut] + b"\xff\xd9"])
        assert ei.value.code == M.EINVAL
    assert same(enc.decode_host([src])[0], DC.reference("revert", "default"))
    enc.close()


def test_bit_flips_decode_as_the_reference_or_fail(simt):
    """the 200 seeded flips of test_simt_transcode.py (same seed, same source).  Measured on the emulator: 170 decode to djpeg's
    pixels and 30 fail, and these 30 are the files mjh_transcode_host fails as well (the decoder and its statuses are shared) and
    the only ones on which the reference's djpeg and jpegtran warn (28) or stop (2)."""
    src = TC.source("revert")
    info = M.jpeg_info(src)
    a, n = info.scans[0].data_offset, info.scans[0].data_size
    rng = random.Random(20240607)
    enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=1)
    equal = failed = 0
    for _ in range(200):
        pos, bit = a + rng.randrange(n), rng.randrange(8)
        bad = bytearray(src)
        bad[pos] ^= 1 << bit
        bad = bytes(bad)
        status, ref = DC.djpeg_status(bad)
        try:
            out = enc.decode_host([bad])[0]
        except M.MjhError as exc:
            assert exc.code == M.EINVAL
            failed += 1
            continue
        if status == 0:
            assert same(out, ref), "flip of bit %d at %d: pixels that differ from the reference's" % (bit, pos)
            equal += 1
    print("bit flips: %d equal, %d failed" % (equal, failed))
    assert equal >= 100, "%d of 200 flips gave the reference's pixels, %d failed" % (equal, failed)
    assert same(enc.decode_host([src])[0], DC.reference("revert", "default"))
    enc.close()


def test_damaged_file_in_a_batch(simt):
    src = TC.source("revert")
    info = M.jpeg_info(src)
    a, n = info.scans[0].data_offset, info.scans[0].data_size
    bad = src[:a + n // 2] + src[a + n // 2 + 40:]                # 40 bytes of entropy data missing, every marker in place
    good2 = TC.source("revert_opt")
    ref = [DC.reference("revert", "default"), None, DC.reference("revert_opt", "default")]
    enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=3)
    with pytest.raises(M.MjhError) as ei:
        enc.decode_host([src, bad, good2])
    assert ei.value.code == M.EINVAL and "file 1" in str(ei.value)
    assert [enc.transcode_status(i)[0] for i in range(3)] == [M.OK, M.EINVAL, M.OK]
    assert "Corrupt" in enc.transcode_status(1)[1]
    outs = enc.decode_host([src, good2])                          # the encoder stays usable
    assert same(outs[0], ref[0]) and same(outs[1], ref[2])
    enc.close()
    out = M.decode([src, bad, good2])
    assert same(out[0], ref[0]) and same(out[2], ref[2])
    assert isinstance(out[1], M.MjhError) and out[1].code == M.EINVAL


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", list(TC.REFUSALS))
def test_refused_sources(simt, what):
    args, word = TC.REFUSALS[what]
    src = TC.cjpeg(TC.testorig(), args)
    r = M.decode([src, TC.source("revert")])
    assert isinstance(r[0], M.MjhError) and r[0].code == M.EUNSUPPORTED and word in str(r[0])
    assert same(r[1], DC.reference("revert", "default"))


def test_transform_with_decode_is_refused(simt):
    src = TC.source("revert")
    enc = M.Encoder(M.params_from_jpeg(src, revert=True, transform="flip_h"), max_batch=1)
    with pytest.raises(M.MjhError) as ei:
        enc.decode_host([src])
    assert ei.value.code == M.EUNSUPPORTED and "transform" in str(ei.value)
    enc.close()


BAD_OPTIONS = (dict(color=7), dict(color=3), dict(pixel_size=2), dict(pixel_size=5), dict(color="gray", pixel_size=3),
               dict(pixel_size=3, rgb_offset=(0, 1, 3)), dict(pixel_size=4, rgb_offset=(1, 1, 2)))


def _raw_opts(kw):
    """the DecodeOpts of kw WITHOUT the binding's own validation: what a C caller could pass"""
    o = M.DecodeOpts()
    M.lib().mjh_decode_opts_defaults(o)
    color = kw.get("color")
    o.out_color_space = {None: 0, "gray": M.CS_GRAYSCALE}.get(color, color)
    o.pixel_size = kw.get("pixel_size", 0)
    if "rgb_offset" in kw:
        o.rgb_offset[:] = kw["rgb_offset"]
    return o


def test_bad_options(simt):
    """refused by decode() before any encoder exists, and by the library whatever the encoder did before: fresh, after a good
    batch, after a batch with a damaged file (whose status must not come back for the refused call)"""
    src = TC.source("revert")
    M._decode_encoders.clear()
    for kw in BAD_OPTIONS:
        with pytest.raises(M.MjhError) as ei:
            M.decode([src], **kw)
        assert ei.value.code == M.EINVAL, kw
    with pytest.raises(M.MjhError) as ei:
        M.decode([src], layout="cmyk")
    assert ei.value.code == M.EINVAL
    assert not M._decode_encoders                       # nothing was grouped, no encoder made
    info = M.jpeg_info(src)
    a, n = info.scans[0].data_offset, info.scans[0].data_size
    bad = src[:a + n // 2] + src[a + n // 2 + 40:]
    for history in ("fresh", "good", "damaged"):
        enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=2)
        if history == "good":
            enc.decode_host([src])
        elif history == "damaged":
            res = enc.decode_host([src, bad], errors="return")
            assert res[0] is None and isinstance(res[1], M.MjhError)
        for kw in BAD_OPTIONS:
            for errors in ("raise", "return"):
                with pytest.raises(M.MjhError) as ei:
                    enc.decode_host([src], errors=errors, opts=_raw_opts(kw))
                assert ei.value.code == M.EINVAL and "Corrupt" not in str(ei.value), (history, kw)
                assert ("color_space" in str(ei.value)) or ("pixel_size" in str(ei.value)) or ("rgb_offset" in str(ei.value)), str(ei.value)
            assert M.lib().mjh_transcode_batch_size(enc._h) == 0
            assert enc.transcode_status(0)[0] == M.EINVAL      # no per-file status of the earlier batch is left
        assert same(enc.decode_host([src])[0], DC.reference("revert", "default"))
        enc.close()


def test_refused_call_leaves_no_status_of_an_earlier_batch(simt):
    """a transform set on an encoder that decoded a damaged batch before; a transcode call refused in the marker walk on an encoder
    that decoded before"""
    src = TC.source("revert")
    info = M.jpeg_info(src)
    a, n = info.scans[0].data_offset, info.scans[0].data_size
    bad = src[:a + n // 2] + src[a + n // 2 + 40:]
    enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=2)
    res = enc.decode_host([bad, src], errors="return")
    assert isinstance(res[0], M.MjhError) and res[1] is None
    enc.set_transform(transform="flip_h")
    for errors in ("raise", "return"):
        with pytest.raises(M.MjhError) as ei:
            enc.decode_host([src, src], errors=errors)
        assert ei.value.code == M.EUNSUPPORTED and "transform" in str(ei.value)
    enc.set_transform(None)
    # the marker walk refuses file 1 (other sampling factors): file 0 is fine, and is not given the old decode batch's status
    res = enc.transcode_host([src, TC.source("q90_2x1_r1")], errors="return")
    assert res[0] is None and isinstance(res[1], M.MjhError) and "sampling factors" in str(res[1])
    assert enc.transcode_status(0)[0] == M.OK
    with pytest.raises(M.MjhError):
        enc.wait_decode()                               # the last batch of files was not a decode
    outs = enc.decode_host([src, src])
    enc.wait_decode()
    assert same(outs[0], DC.reference("revert", "default"))
    enc.close()
