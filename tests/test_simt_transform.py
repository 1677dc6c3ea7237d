"""CPU suite: lossless transforms (rotate, flip, transpose, transverse, trim, perfect, crop, grayscale) in the re-compression
path, with the decoder kernels of mozjpeg_amd/csrc/mjh_decode.hip executed by the lock-step wave64 emulator (tools/simt,
SIMT_STRICT).  Every expected byte comes from the reference's jpegtran (oracle/_ref/jpegtran -copy none + switches) at test time."""
import os
import random
import sys

import numpy as np
import pytest

import mozjpeg_amd as M
import oracle_lib as O
import transcode_cases as TC
import transform_cases as XC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "simt"))

pytestmark = pytest.mark.skipif(not TC.have_tools(), reason="reference cjpeg / jpegtran not built (oracle/_ref)")


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


# ---- 1. bytes == reference: every operation, with and without trim ------------------------------------------------------------------
@pytest.mark.parametrize("src,sw,op,trim", XC.OP_CASES, ids=["%s-%s-%s%s" % (s, w, o, "-trim" if t else "") for s, w, o, t in XC.OP_CASES])
def test_operation_matches_jpegtran(simt, src, sw, op, trim):
    ref = XC.reference(src, sw, transform=op, trim=trim)
    out = XC.run(M, TC.source(src), sw, transform=op, trim=trim)
    assert XC.frame(M, out) == XC.frame(M, ref)
    assert out == ref, "%d bytes, the reference %d" % (len(out), len(ref))


def test_sizes_and_factors_the_reference_writes(simt):
    """the sizes the issue quotes for the 227x149 source, and the swapped factors of the 2x1 one"""
    want = {("rot90", False): (149, 227), ("rot90", True): (144, 227), ("flip_h", True): (224, 149), ("transverse", True): (144, 224),
            ("rot270", True): (149, 224)}
    for (op, trim), size in want.items():
        for jpeg in (XC.reference("revert", "revert", transform=op, trim=trim), XC.run(M, TC.source("revert"), "revert", transform=op, trim=trim)):
            assert XC.frame(M, jpeg)[:2] == size, (op, trim)
    p = M.params_from_jpeg(TC.source("q90_2x1_r1"), revert=True, transform="rot90")
    assert (p.h_samp_factor[0], p.v_samp_factor[0]) == (1, 2) and (p.image_width, p.image_height) == (149, 227)
    src_q = M.params_from_jpeg(TC.source("q90_2x1_r1"), revert=True)
    for t in set(p.quant_tbl_no[c] for c in range(3)):
        assert np.array_equal(np.array(p.quantval[t]).reshape(8, 8), np.array(src_q.quantval[t]).reshape(8, 8).T)
    assert XC.frame(M, XC.reference("q90_2x1_r1", "revert", transform="rot90"))[3][0] == (1, 2)


# ---- 2. crop ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,op,crop,size", XC.CROP_CASES, ids=["%s-%s-%s" % (s, o, c) for s, o, c, _ in XC.CROP_CASES])
def test_crop_matches_jpegtran(simt, src, op, crop, size):
    for sw in ("revert", "revert_opt"):
        ref = XC.reference(src, sw, transform=op, crop=crop)
        if size is not None:
            assert XC.frame(M, ref)[:2] == size
        assert XC.run(M, TC.source(src), sw, transform=op, crop=crop) == ref, sw


def test_crop_outside_the_image_is_refused(simt):
    status, _ = XC.reference_status("revert", "revert", crop="100x80+300+0")
    assert status == 1
    with pytest.raises(M.MjhError) as ei:
        M.params_from_jpeg(TC.source("revert"), revert=True, crop="100x80+300+0")
    assert ei.value.code == M.EINVAL and "Invalid crop request" in str(ei.value)


# ---- 3. grayscale -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", ["revert", "q90_2x1_r1", "scans3_2x2_r2", "gray_r5b"])
@pytest.mark.parametrize("op", [None, "rot270"])
def test_grayscale_matches_jpegtran(simt, src, op):
    for sw in ("revert", "revert_opt", "fastcrush_progressive"):
        ref = XC.reference(src, sw, transform=op, grayscale=True)
        w, h, nc, samp = XC.frame(M, ref)
        assert nc == 1 and samp == ((1, 1),) and (w, h) == ((149, 227) if op else (227, 149))
        assert XC.run(M, TC.source(src), sw, transform=op, grayscale=True) == ref, sw
    assert XC.run(M, TC.source(src), "revert", transform=op, grayscale=True, trim=True) == XC.reference(src, "revert", transform=op, grayscale=True, trim=True)


def test_grayscale_of_rgb_is_refused(simt):
    status, _ = XC.reference_status("rgb", "revert", grayscale=True)
    assert status == 1
    with pytest.raises(M.MjhError) as ei:
        M.params_from_jpeg(TC.source("rgb"), revert=True, grayscale=True)
    assert ei.value.code == M.EUNSUPPORTED and "JERR_CONVERSION_NOTIMPL" in str(ei.value)


# ---- 4. perfect ---------------------------------------------------------------------------------------------------------------
def test_perfect(simt):
    status, _ = XC.reference_status("revert", "revert", transform="rot90", perfect=True)
    assert status == 1
    with pytest.raises(M.MjhError) as ei:
        M.params_from_jpeg(TC.source("revert"), revert=True, transform="rot90", perfect=True)
    assert ei.value.code == M.EINVAL and "not perfect" in str(ei.value)
    r = M.recompress([TC.source("revert")], revert=True, transform="rot90", perfect=True)[0]
    assert isinstance(r, M.MjhError) and r.code == M.EINVAL
    ref = XC.reference("revert", "revert", transform="transpose", perfect=True)
    assert XC.frame(M, ref)[:2] == (149, 227)
    assert XC.run(M, TC.source("revert"), "revert", transform="transpose", perfect=True) == ref
    ref = XC.reference("noise_q100", "revert_opt", transform="rot90", perfect=True)
    assert XC.frame(M, ref)[:2] == (48, 64)
    assert XC.run(M, TC.source("noise_q100"), "revert_opt", transform="rot90", perfect=True) == ref


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(simt):
    src = TC.source("revert")
    status, out = XC.reference_status("revert", "revert", crop="300x80+0+0")
    assert status == 0 and XC.frame(M, out)[:2] == (300, 80)              # the reference extends; this project does not
    with pytest.raises(M.MjhError) as ei:
        M.params_from_jpeg(src, revert=True, crop="300x80+0+0")
    assert ei.value.code == M.EUNSUPPORTED and "crop extension" in str(ei.value)
    status, out = XC.reference_status("revert", "revert", crop="100x80f+17+9")
    assert status == 0 and XC.frame(M, out)[:2] == (101, 80)
    with pytest.raises(M.MjhError) as ei:
        M.params_from_jpeg(src, revert=True, crop="100x80f+17+9")
    assert ei.value.code == M.EUNSUPPORTED and "suffix" in str(ei.value)
    status, _ = XC.reference_status("revert", "revert", crop="100xx")
    assert status != 0
    with pytest.raises(M.MjhError) as ei:
        M.params_from_jpeg(src, revert=True, crop="100xx")
    assert ei.value.code == M.EINVAL and "bogus -crop argument" in str(ei.value)
    with pytest.raises(M.MjhError) as ei:
        M.params_from_jpeg(src, revert=True, transform="rot45")
    assert ei.value.code == M.EINVAL
    r = M.recompress([src], revert=True, crop="300x80+0+0")[0]
    assert isinstance(r, M.MjhError) and r.code == M.EUNSUPPORTED


def test_crop_string_states(simt):
    """the fields mjh_transform_parse_crop leaves, with their UNSET / POS / NEG states (jtransform_parse_crop_spec)"""
    def fields(spec):
        t = M.transform_spec(crop=spec)
        return (t.crop, (t.crop_width, t.crop_width_set), (t.crop_height, t.crop_height_set), (t.crop_xoffset, t.crop_xoffset_set),
                (t.crop_yoffset, t.crop_yoffset_set))
    assert fields("100x80+17+9") == (1, (100, 1), (80, 1), (17, 1), (9, 1))
    assert fields("100x80-20-30") == (1, (100, 1), (80, 1), (20, 2), (30, 2))
    assert fields("+16+16") == (1, (0, 0), (0, 0), (16, 1), (16, 1))
    assert fields("x80") == (1, (0, 0), (80, 1), (0, 0), (0, 0))
    assert fields("100") == (1, (100, 1), (0, 0), (0, 0), (0, 0))
    assert fields("100Fx80r-5") == (1, (100, 3), (80, 4), (5, 2), (0, 0))
    for bad in ("100xx", "100x", "+", "100x80+1+2+3", "a", "100 x80"):
        with pytest.raises(M.MjhError) as ei:
            M.transform_spec(crop=bad)
        assert ei.value.code == M.EINVAL, bad
    assert M.transform_spec() is None and M.transform_spec(transform=None, trim=False) is None


# ---- 6. batches ---------------------------------------------------------------------------------------------------------------
def _batch_files():
    img = TC.testorig()
    a = TC.patch_jfif(TC.cjpeg(img, ["-revert"]), 1, 2, 1, 72, 72)
    b = TC.cjpeg(img[::-1].copy(), ["-revert", "-optimize", "-restart", "1"])
    c = TC.patch_jfif(TC.cjpeg(np.roll(img, 40, axis=1), ["-revert", "-optimize", "-restart", "7B"]), 1, 1, 2, 300, 150)
    return [a, b, c]


@pytest.mark.parametrize("sw", ["revert_opt", "fastcrush_progressive"])
def test_batch_of_different_files(simt, sw):
    files = _batch_files()
    kw, args = TC.SWITCHES[sw]
    enc = M.Encoder(M.params_from_jpeg(files[0], transform="rot90", trim=True, **kw), max_batch=3)
    outs = enc.transcode_host(files)
    for f, o in zip(files, outs):
        assert o == O.ref_jpegtran(f, ["-copy", "none", "-rotate", "90", "-trim"] + args)
        assert o == enc.transcode_host([f])[0]
    assert outs[0][11:18] == bytes([1, 2, 1, 0, 72, 0, 72]) and outs[2][11:18] == bytes([1, 1, 2, 1, 44, 0, 150])
    enc.close()


def test_file_of_another_size_in_a_batch_is_named(simt):
    src = TC.source("revert")
    other = TC.cjpeg(TC.testorig()[:, :225], ["-revert"])                   # 225x149: trims to the same 144x224 as 227x149
    enc = M.Encoder(M.params_from_jpeg(src, revert=True, transform="transverse", trim=True), max_batch=3)
    assert M.params_from_jpeg(other, revert=True, transform="transverse", trim=True).image_height == enc.params.image_height == 224
    with pytest.raises(M.MjhError) as ei:
        enc.transcode_host([src, other, src])
    assert ei.value.code == M.EINVAL and "file 1" in str(ei.value) and "image size" in str(ei.value)
    small = TC.source("17x9")
    with pytest.raises(M.MjhError) as ei:
        enc.transcode_host([src, src, small])
    assert ei.value.code == M.EINVAL and "file 2" in str(ei.value) and "image size" in str(ei.value)
    with pytest.raises(M.MjhError) as ei:
        enc.transcode_host([src, TC.source("q90_2x1_r1")])
    assert ei.value.code == M.EINVAL and "file 1" in str(ei.value)
    ref = XC.reference("revert", "revert", transform="transverse", trim=True)
    assert enc.transcode_host([src, src]) == [ref, ref]                      # the encoder stays usable
    # the other source alone defines the call's geometry: same encoder, same destination
    assert enc.transcode_host([other])[0] == O.ref_jpegtran(other, ["-copy", "none", "-transverse", "-trim", "-revert"])
    enc.close()


def test_recompress_keeps_input_order_and_never_returns_the_source(simt):
    names = ["revert", "gray_r5b", "8x8", "revert_opt", "rgb", "17x9", "jfif102", "s1x2", "1x1", "noise_q100", "scans3_2x2_r2", "revert",
             "cjpeg_baseline"]
    random.Random(6).shuffle(names)
    for sw in ("revert_opt", "fastcrush_progressive"):
        outs = M.recompress([TC.source(s) for s in names], max_batch=4, transform="rot90", **TC.SWITCHES[sw][0])
        for s, o in zip(names, outs):
            assert o == XC.reference(s, sw, transform="rot90"), "%s %s" % (s, sw)
            assert o != TC.source(s)


def test_prefer_smallest_is_off_under_a_transform(simt):
    """cjpeg_baseline: the source recompress() hands back under the default switches (test_simt_transcode.py); with trim, crop or
    grayscale -- which leave a 224x144 / same-size image -- the re-coded file comes back although the source is no larger"""
    src = TC.source("cjpeg_baseline")
    assert M.recompress([src])[0] == src
    for xf in (dict(crop="227x149+0+0"), dict(grayscale=True), dict(transform="flip_h")):
        status, ref = TC.jpegtran_status(src, ["-copy", "none"] + XC.jpegtran_args(**xf))
        assert status == 0
        out = M.recompress([src], **xf)[0]
        assert out != src
        assert out == ref, xf


# ---- 7. subsequence lengths ---------------------------------------------------------------------------------------------------
SUBSEQ_CASES = [("revert", "revert_opt", dict(transform="rot90")), ("q90_2x1_r1", "revert", dict(transform="transverse", trim=True)),
                ("gray_r5b", "revert_opt", dict(transform="rot270")), ("scans3_2x2_r2", "revert", dict(transform="flip_h", grayscale=True)),
                ("s_mixed", "revert_opt", dict(transform="rot180", crop="100x80+20+30")), ("noise_q100", "revert_opt", dict(transform="flip_v"))]


@pytest.mark.parametrize("S", [0, 16, None])
def test_subsequence_length_changes_nothing(simt, monkeypatch, S):
    if S is None:
        monkeypatch.delenv("MJH_DECODE_SUBSEQ", raising=False)
    else:
        monkeypatch.setenv("MJH_DECODE_SUBSEQ", str(S))
    for src, sw, xf in SUBSEQ_CASES:
        enc = M.Encoder(M.params_from_jpeg(TC.source(src), **TC.SWITCHES[sw][0], **xf), max_batch=1)
        out = enc.transcode_host([TC.source(src)])[0]
        st = enc.transcode_stats()
        enc.close()
        if S is not None:
            assert st["subseq"] == S
        assert out == XC.reference(src, sw, **xf), "%s %s %s S=%s" % (src, sw, xf, S)


# ---- 8. untrusted input (the emulator's device buffers end at unmapped pages) ---------------------------------------------------
@pytest.mark.parametrize("xf", [dict(transform="rot90"), dict(crop="100x80+17+9"), dict(transform="transverse", trim=True, grayscale=True)],
                         ids=["rot90", "crop", "transverse-trim-gray"])
def test_truncated_and_flipped_files(simt, xf):
    src = TC.source("revert")
    info = M.jpeg_info(src)
    a, n = info.scans[0].data_offset, info.scans[0].data_size
    args = ["-copy", "none"] + XC.jpegtran_args(**xf) + ["-revert", "-optimize"]
    good = XC.reference("revert", "revert_opt", **xf)
    enc = M.Encoder(M.params_from_jpeg(src, revert=True, optimize=True, **xf), max_batch=3)
    cuts = list(range(a, a + n, 211))
    assert len(cuts) > 10
    for cut in cuts:
        with pytest.raises(M.MjhError) as ei:
            enc.transcode_host([src[:cut]])
        assert ei.value.code == M.EINVAL
    for cut in cuts[1::3]:
        with pytest.raises(M.MjhError) as ei:
            enc.transcode_host([src[:cut] + b"\xff\xd9"])
        assert ei.value.code == M.EINVAL
    rng = random.Random(20240608)
    equal = failed = 0
    for _ in range(120):
        pos, bit = a + rng.randrange(n), rng.randrange(8)
        bad = bytearray(src)
        bad[pos] ^= 1 << bit
        bad = bytes(bad)
        status, ref = TC.jpegtran_status(bad, args)
        try:
            out = enc.transcode_host([bad])[0]
        except M.MjhError as exc:
            assert exc.code == M.EINVAL
            failed += 1
            continue
        if status == 0:
            assert out == ref, "flip of bit %d at %d: a file that differs from the reference's" % (bit, pos)
            equal += 1
    assert equal >= 50, "%d of 120 flips gave the reference's bytes, %d failed" % (equal, failed)
    # a damaged file in a batch is reported per file, the others are unaffected
    bad = src[:a + n // 2] + src[a + n // 2 + 40:]
    with pytest.raises(M.MjhError) as ei:
        enc.transcode_host([src, bad, src])
    assert ei.value.code == M.EINVAL and "file 1" in str(ei.value)
    assert [enc.transcode_status(i)[0] for i in range(3)] == [M.OK, M.EINVAL, M.OK]
    assert enc.transcode_host([src, src]) == [good, good]
    enc.close()


# ---- 9. no transform is today's path --------------------------------------------------------------------------------------------
def test_no_transform_is_todays_path(simt):
    for name in ("revert", "gray_r5b", "scans3_2x2_r2"):
        src = TC.source(name)
        for kw in (dict(revert=True), dict(revert=True, optimize=True), dict()):
            a, b = M.params_from_jpeg(src, **kw), M.params_from_jpeg(src, transform=None, **kw)
            c = M.params_from_jpeg(src, transform=None, trim=False, perfect=False, crop=None, grayscale=False, **kw)
            assert bytes(a) == bytes(b) == bytes(c)
            assert getattr(b, "transform", None) is None
        ea, eb = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=1), M.Encoder(M.params_from_jpeg(src, revert=True, transform=None), max_batch=1)
        assert ea.transcode_host([src]) == eb.transcode_host([src]) == [TC.reference(name, "revert")]
        # a transform set and taken away again leaves the encoder where it was
        eb.set_transform("rot180")
        eb.set_transform(None)
        assert eb.transcode_host([src]) == [TC.reference(name, "revert")]
        ea.close()
        eb.close()
