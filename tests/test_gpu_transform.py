"""Lossless transforms in the re-compression path on the chip (-m gpu): the cases of test_simt_transform.py that compare bytes
with the reference's jpegtran, plus full-size batches.  Reads only the tree and oracle/_ref."""
import random

import numpy as np
import pytest

import mozjpeg_amd as M
import oracle_lib as O
import transcode_cases as TC
import transform_cases as XC

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not TC.have_tools(), reason="reference cjpeg / jpegtran not built (oracle/_ref)")]


@pytest.mark.parametrize("src,sw,op,trim", XC.OP_CASES, ids=["%s-%s-%s%s" % (s, w, o, "-trim" if t else "") for s, w, o, t in XC.OP_CASES])
def test_operation_matches_jpegtran(src, sw, op, trim):
    ref = XC.reference(src, sw, transform=op, trim=trim)
    out = XC.run(M, TC.source(src), sw, transform=op, trim=trim)
    assert out == ref, "%d bytes, the reference %d" % (len(out), len(ref))


@pytest.mark.parametrize("src,op,crop,size", XC.CROP_CASES, ids=["%s-%s-%s" % (s, o, c) for s, o, c, _ in XC.CROP_CASES])
def test_crop_matches_jpegtran(src, op, crop, size):
    for sw in ("revert", "revert_opt"):
        ref = XC.reference(src, sw, transform=op, crop=crop)
        if size is not None:
            assert XC.frame(M, ref)[:2] == size
        assert XC.run(M, TC.source(src), sw, transform=op, crop=crop) == ref, sw


@pytest.mark.parametrize("src", ["revert", "q90_2x1_r1", "scans3_2x2_r2", "gray_r5b"])
@pytest.mark.parametrize("op", [None, "rot270"])
def test_grayscale_matches_jpegtran(src, op):
    for sw in ("revert", "revert_opt", "fastcrush_progressive"):
        ref = XC.reference(src, sw, transform=op, grayscale=True)
        assert XC.frame(M, ref)[2:] == (1, ((1, 1),))
        assert XC.run(M, TC.source(src), sw, transform=op, grayscale=True) == ref, sw


def test_perfect_and_refusals():
    src = TC.source("revert")
    for kw, code, word in ((dict(transform="rot90", perfect=True), M.EINVAL, "not perfect"), (dict(crop="300x80+0+0"), M.EUNSUPPORTED, "crop extension"),
                           (dict(crop="100x80f+17+9"), M.EUNSUPPORTED, "suffix"), (dict(crop="100xx"), M.EINVAL, "bogus -crop argument"),
                           (dict(crop="100x80+300+0"), M.EINVAL, "Invalid crop request")):
        with pytest.raises(M.MjhError) as ei:
            M.params_from_jpeg(src, revert=True, **kw)
        assert ei.value.code == code and word in str(ei.value)
    with pytest.raises(M.MjhError) as ei:
        M.params_from_jpeg(TC.source("rgb"), revert=True, grayscale=True)
    assert ei.value.code == M.EUNSUPPORTED
    assert XC.run(M, src, "revert", transform="transpose", perfect=True) == XC.reference("revert", "revert", transform="transpose", perfect=True)
    assert XC.run(M, TC.source("noise_q100"), "revert_opt", transform="rot90", perfect=True) == \
        XC.reference("noise_q100", "revert_opt", transform="rot90", perfect=True)


@pytest.mark.parametrize("sw", ["revert_opt", "fastcrush_progressive"])
def test_batch_of_different_files(sw):
    img = TC.testorig()
    files = [TC.patch_jfif(TC.cjpeg(img, ["-revert"]), 1, 2, 1, 72, 72),
             TC.cjpeg(img[::-1].copy(), ["-revert", "-optimize", "-restart", "1"]),
             TC.patch_jfif(TC.cjpeg(np.roll(img, 40, axis=1), ["-revert", "-optimize", "-restart", "7B"]), 1, 1, 2, 300, 150)]
    kw, args = TC.SWITCHES[sw]
    enc = M.Encoder(M.params_from_jpeg(files[0], transform="rot90", trim=True, **kw), max_batch=3)
    outs = enc.transcode_host(files)
    for f, o in zip(files, outs):
        assert o == O.ref_jpegtran(f, ["-copy", "none", "-rotate", "90", "-trim"] + args)
        assert o == enc.transcode_host([f])[0]
    with pytest.raises(M.MjhError) as ei:
        enc.transcode_host([files[0], TC.cjpeg(img[:, :225], ["-revert"])])
    assert ei.value.code == M.EINVAL and "file 1" in str(ei.value) and "image size" in str(ei.value)
    enc.close()


def test_recompress_keeps_input_order_and_never_returns_the_source():
    names = ["revert", "gray_r5b", "8x8", "revert_opt", "rgb", "17x9", "jfif102", "s1x2", "1x1", "noise_q100", "scans3_2x2_r2", "revert",
             "cjpeg_baseline"]
    random.Random(6).shuffle(names)
    for sw in ("revert_opt", "default"):
        outs = M.recompress([TC.source(s) for s in names], max_batch=4, transform="rot90", **TC.SWITCHES[sw][0])
        for s, o in zip(names, outs):
            assert o == XC.reference(s, sw, transform="rot90"), "%s %s" % (s, sw)
            assert o != TC.source(s)


SUBSEQ_CASES = [("revert", "revert_opt", dict(transform="rot90")), ("q90_2x1_r1", "revert", dict(transform="transverse", trim=True)),
                ("gray_r5b", "revert_opt", dict(transform="rot270")), ("scans3_2x2_r2", "revert", dict(transform="flip_h", grayscale=True)),
                ("s_mixed", "revert_opt", dict(transform="rot180", crop="100x80+20+30")), ("noise_q100", "revert_opt", dict(transform="flip_v"))]


@pytest.mark.parametrize("S", [0, None])
def test_subsequence_length_changes_nothing(monkeypatch, S):
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


def test_no_transform_is_todays_path():
    src = TC.source("revert")
    a, b = M.params_from_jpeg(src, revert=True), M.params_from_jpeg(src, revert=True, transform=None)
    assert bytes(a) == bytes(b)
    ea, eb = M.Encoder(a, max_batch=1), M.Encoder(b, max_batch=1)
    assert ea.transcode_host([src]) == eb.transcode_host([src]) == [TC.reference("revert", "revert")]
    ea.close()
    eb.close()


# ---- full size ------------------------------------------------------------------------------------------------------------------
def _full_size(w, h, cases):
    files = [TC.cjpeg(O.synthetic_frame(w, h, seed=100 + i), ["-revert", "-quality", "75", "-sample", "2x2"]) for i in range(8)]
    assert len(set(files)) == 8
    for xf in cases:
        enc = M.Encoder(M.params_from_jpeg(files[0], revert=True, optimize=True, **xf), max_batch=8)
        outs = enc.transcode_host(files)
        enc.close()
        args = ["-copy", "none"] + XC.jpegtran_args(**xf) + ["-revert", "-optimize"]
        for i, (f, o) in enumerate(zip(files, outs)):
            ref = O.ref_jpegtran(f, args)
            assert o == ref, "file %d, %s: %d bytes, the reference %d" % (i, xf, len(o), len(ref))


def test_full_size_batch():
    """8 distinct 4K 4:2:0 q75 files in one call under rot90 and under flip_h (3840x2160: no partial iMCU, 2160 = 135 iMCUs)"""
    _full_size(3840, 2160, [dict(transform="rot90"), dict(transform="flip_h")])


def test_full_size_batch_with_edges():
    """the same at 3838x2158: a partial iMCU on both sides, kept in place without trim and cut off with it"""
    _full_size(3838, 2158, [dict(transform="rot90"), dict(transform="rot90", trim=True), dict(transform="flip_h"), dict(transform="flip_h", trim=True)])


def test_many_small_files_in_one_call():
    """256 files of 320x240 in one call under transpose"""
    big = O.synthetic_frame(1280, 960, seed=9)
    rng = random.Random(320)
    files = []
    for i in range(256):
        x, y = rng.randrange(0, 1280 - 320), rng.randrange(0, 960 - 240)
        files.append(TC.cjpeg(big[y:y + 240, x:x + 320], ["-revert", "-quality", "75", "-sample", "2x2"] + (["-restart", "1"] if i % 7 == 3 else [])))
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True, optimize=True, transform="transpose"), max_batch=256)
    outs = enc.transcode_host(files)
    enc.close()
    for i, (f, o) in enumerate(zip(files, outs)):
        assert o == O.ref_jpegtran(f, ["-copy", "none", "-transpose", "-revert", "-optimize"]), "file %d" % i
