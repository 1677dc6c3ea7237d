"""GPU (-m gpu): re-compression of existing JPEG files on the chip (mjh_transcode_host: the Huffman decoder of mjh_decode.hip in front of
the entropy-coding passes).  Every expected byte comes from the reference's jpegtran (oracle/_ref/jpegtran -copy none + switches)
at test time.  The untrusted-input cases (truncation, bit flips) run on the emulator only (test_simt_transcode.py)."""
import random

import numpy as np
import pytest

import mozjpeg_amd as M
import oracle_lib as O
import transcode_cases as TC

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not TC.have_tools(), reason="reference cjpeg / jpegtran not built (oracle/_ref)")]


@pytest.mark.parametrize("src,sw", TC.ALL_PAIRS, ids=["%s-%s" % p for p in TC.ALL_PAIRS])
def test_transcode_matches_jpegtran(src, sw):
    ref = TC.reference(src, sw)
    out = TC.run_pair(M, src, sw)
    assert out == ref, "%d bytes, the reference %d" % (len(out), len(ref))


def test_default_switches_recode_branch_is_taken():
    for name in ("revert", "q90_2x1_r1", "gray_r5b", "noise_q100"):
        src, ref = TC.source(name), TC.reference(name, "default")
        assert ref != src, "%s: the reference gave the source back" % name
        enc = M.Encoder(M.params_from_jpeg(src), max_batch=1)
        assert enc.transcode_host([src])[0] == ref
        enc.close()


SUBSEQ_PAIRS = [("revert", "revert_opt"), ("q90_2x1_r1", "revert"), ("gray_r5b", "revert_opt"), ("scans3_2x2_r2", "revert"),
                ("rgb", "revert_opt"), ("oracle_baseline", "revert"), ("s_mixed", "revert_opt"), ("noise_q100", "revert_opt"), ("17x9", "revert")]


@pytest.mark.parametrize("S", [0, None])
def test_subsequence_length_changes_nothing(monkeypatch, S):
    if S is None:
        monkeypatch.delenv("MJH_DECODE_SUBSEQ", raising=False)
    else:
        monkeypatch.setenv("MJH_DECODE_SUBSEQ", str(S))
    for src, sw in SUBSEQ_PAIRS:
        enc = M.Encoder(M.params_from_jpeg(TC.source(src), **TC.SWITCHES[sw][0]), max_batch=1)
        out = enc.transcode_host([TC.source(src)])[0]
        st = enc.transcode_stats()
        enc.close()
        if S is not None:
            assert st["subseq"] == S
        assert out == TC.reference(src, sw), "%s %s S=%s" % (src, sw, S)


@pytest.mark.parametrize("sw", ["revert_opt", "fastcrush_progressive"])
def test_batch_of_different_files(sw):
    img = TC.testorig()
    files = [TC.patch_jfif(TC.cjpeg(img, ["-revert"]), 1, 2, 1, 72, 72),
             TC.cjpeg(img[::-1].copy(), ["-revert", "-optimize", "-restart", "1"]),
             TC.patch_jfif(TC.cjpeg(np.roll(img, 40, axis=1), ["-revert", "-optimize", "-restart", "7B"]), 1, 1, 2, 300, 150)]
    kw, args = TC.SWITCHES[sw]
    enc = M.Encoder(M.params_from_jpeg(files[0], **kw), max_batch=3)
    outs = enc.transcode_host(files)
    for f, o in zip(files, outs):
        assert o == O.ref_jpegtran(f, ["-copy", "none"] + args)
        assert o == enc.transcode_host([f])[0]
    enc.close()


def test_recompress_keeps_input_order():
    names = ["revert", "gray_r5b", "8x8", "revert_opt", "rgb", "17x9", "jfif102", "s1x2", "1x1", "noise_q100", "scans3_2x2_r2", "revert"]
    random.Random(5).shuffle(names)
    for sw in ("revert_opt", "default"):
        outs = M.recompress([TC.source(s) for s in names], max_batch=4, **TC.SWITCHES[sw][0])
        for s, o in zip(names, outs):
            assert o == TC.reference(s, sw), "%s %s" % (s, sw)


def test_full_size_batch():
    """8 distinct 4K 4:2:0 q75 sequential files without restart markers in one call"""
    files = [TC.cjpeg(O.synthetic_frame(3840, 2160, seed=100 + i), ["-revert", "-quality", "75", "-sample", "2x2"]) for i in range(8)]
    assert len(set(files)) == 8
    for sw in ("revert_opt", "default"):
        kw, args = TC.SWITCHES[sw]
        enc = M.Encoder(M.params_from_jpeg(files[0], **kw), max_batch=8)
        outs = enc.transcode_host(files)
        st = enc.transcode_stats()
        enc.close()
        print("4K batch, %s: subsequences of %d bytes, %d synchronisation rounds, %d host synchronisations" % (sw, st["subseq"], st["rounds"], st["host_syncs"]))
        for i, (f, o) in enumerate(zip(files, outs)):
            ref = O.ref_jpegtran(f, ["-copy", "none"] + args)
            assert ref != f
            assert o == ref, "file %d, %s: %d bytes, the reference %d" % (i, sw, len(o), len(ref))


@pytest.mark.parametrize("size", [(64, 64), (320, 240)])
def test_many_small_files_in_one_call(size):
    """256 files of one signature in one call"""
    w, h = size
    big = O.synthetic_frame(1280, 960, seed=9)
    rng = random.Random(w)
    files = []
    for i in range(256):
        x, y = rng.randrange(0, 1280 - w), rng.randrange(0, 960 - h)
        files.append(TC.cjpeg(big[y:y + h, x:x + w], ["-revert", "-quality", "75", "-sample", "2x2"] + (["-restart", "1"] if i % 7 == 3 else [])))
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True, optimize=True), max_batch=256)
    outs = enc.transcode_host(files)
    enc.close()
    for i, (f, o) in enumerate(zip(files, outs)):
        assert o == O.ref_jpegtran(f, ["-copy", "none", "-revert", "-optimize"]), "file %d" % i
