"""CPU suite: re-compression of existing JPEG files (mjh_transcode_host) with the decoder kernels of mozjpeg_amd/csrc/mjh_decode.hip
executed by the lock-step wave64 emulator (tools/simt, SIMT_STRICT).  Every expected byte comes from the reference's jpegtran
(oracle/_ref/jpegtran -copy none + switches) at test time; sources are made at test time as well (tests/transcode_cases.py)."""
import os
import random
import sys

import numpy as np
import pytest

import mozjpeg_amd as M
import oracle_lib as O
import transcode_cases as TC

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


@pytest.fixture
def subseq(monkeypatch):
    def set_(s):
        if s is None:
            monkeypatch.delenv("MJH_DECODE_SUBSEQ", raising=False)
        else:
            monkeypatch.setenv("MJH_DECODE_SUBSEQ", str(s))
    return set_


# ---- 1. bytes == reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,sw", TC.ALL_PAIRS, ids=["%s-%s" % p for p in TC.ALL_PAIRS])
def test_transcode_matches_jpegtran(simt, src, sw):
    ref = TC.reference(src, sw)
    out = TC.run_pair(M, src, sw)
    assert out == ref, "%d bytes, the reference %d" % (len(out), len(ref))


def test_default_switches_recode_branch_is_taken(simt):
    """the Encoder-level comparison of the default switches, on sources whose reference result is NOT the source given back"""
    used = 0
    for name in ("revert", "q90_2x1_r1", "gray_r5b", "noise_q100"):
        src, ref = TC.source(name), TC.reference(name, "default")
        assert ref != src, "%s: the reference gave the source back" % name
        enc = M.Encoder(M.params_from_jpeg(src), max_batch=1)
        assert enc.transcode_host([src])[0] == ref
        enc.close()
        used += 1
    assert used == 4
    # and the other branch: a source the reference's jpegtran gives back unchanged comes back unchanged from recompress()
    src = TC.source("cjpeg_baseline")
    assert TC.reference("cjpeg_baseline", "default") == src
    assert M.recompress([src])[0] == src


# ---- 2. decoded coefficients == the coefficients the source was made from -----------------------------------------------------
def test_decoded_coefficients_equal_the_encoders(simt):
    data, taps, p = TC.oracle_source()
    enc = M.Encoder(M.params_from_jpeg(data, revert=True), max_batch=1)
    enc.set_debug_taps(True)
    enc.transcode_host([data])
    gs, _, _ = O.geometry(p)
    for ci, g in enumerate(gs):
        got = enc.read_tap(M.TAP_COEF_Q, 0, ci)                           # [64 zig-zag][blocks]
        want = taps[("coef_q", ci)][:g.hib, :g.wib].reshape(-1, 64)      # natural order
        zz = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                       28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                       54, 47, 55, 62, 63])
        assert np.array_equal(got.T, want[:, zz]), "component %d" % ci
    enc.close()


# ---- 3. subsequence lengths ---------------------------------------------------------------------------------------------------
SUBSEQ_PAIRS = [("revert", "revert_opt"), ("q90_2x1_r1", "revert"), ("gray_r5b", "revert_opt"), ("scans3_2x2_r2", "revert"),
                ("rgb", "revert_opt"), ("oracle_baseline", "revert"), ("s_mixed", "revert_opt"), ("noise_q100", "revert_opt"), ("17x9", "revert")]


@pytest.mark.parametrize("S", [0, 16, 64])
def test_subsequence_length_changes_nothing(simt, subseq, S):
    subseq(S)
    for src, sw in SUBSEQ_PAIRS:
        enc = M.Encoder(M.params_from_jpeg(TC.source(src), **TC.SWITCHES[sw][0]), max_batch=1)
        out = enc.transcode_host([TC.source(src)])[0]
        st = enc.transcode_stats()
        enc.close()
        assert st["subseq"] == S
        assert out == TC.reference(src, sw), "%s %s S=%d" % (src, sw, S)
        if S == 16 and len(TC.source(src)) > 2000:
            assert st["rounds"] >= 3
        if S == 0:
            assert st["rounds"] == 0


def test_subsequence_starts_inside_stuffing_and_restarts(simt):
    """S = 16 on the q100 noise and the -restart 1 files: subsequences begin inside code words, on the zero of a stuffed FF 00 and right
    behind RSTn markers -- the premise of test 3, checked on the bytes"""
    src = TC.source("noise_q100")
    info = M.jpeg_info(src)
    a = info.scans[0].data_offset
    ent = src[a:a + info.scans[0].data_size]
    assert any(ent[i] == 0 and ent[i - 1] == 0xFF for i in range(16, len(ent), 16)), "no subsequence starts on a stuffed zero"
    assert M.jpeg_info(TC.source("q90_2x1_r1")).scans[0].restart_interval == 15


# ---- 4. one batch, different tables / restart intervals / densities ---------------------------------------------------------------
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
    enc = M.Encoder(M.params_from_jpeg(files[0], **kw), max_batch=3)
    outs = enc.transcode_host(files)
    for f, o in zip(files, outs):
        assert o == O.ref_jpegtran(f, ["-copy", "none"] + args)
        assert o == enc.transcode_host([f])[0]
    assert outs[0][11:18] == bytes([1, 2, 1, 0, 72, 0, 72]) and outs[2][11:18] == bytes([1, 1, 2, 1, 44, 0, 150])
    enc.close()


@pytest.mark.parametrize("S", [16, None])
def test_fill_bytes_and_a_scan_of_two_components(simt, subseq, S):
    """0xFF fill bytes in front of RSTn and of the markers that end a scan; a script whose second scan interleaves Cb and Cr, with
    restart intervals that differ between the scans"""
    subseq(S)
    two = TC.cjpeg(TC.testorig(), ["-revert", "-sample", "2x1", "-restart", "3"], script="0: 0 63 0 0;\n1 2: 0 63 0 0;\n")
    info = M.jpeg_info(two)
    assert [(info.scans[k].comps_in_scan, info.scans[k].restart_interval) for k in range(info.num_scans)] == [(1, 87), (2, 45)]
    for src in (two, TC.source("q90_2x1_r1")):
        padded, n = TC.add_fill_bytes(src, M.jpeg_info(src))
        assert n > 10 and len(padded) > len(src)
        for sw in ("revert", "revert_opt", "fastcrush_progressive"):
            kw, args = TC.SWITCHES[sw]
            ref = O.ref_jpegtran(src, ["-copy", "none"] + args)
            assert O.ref_jpegtran(padded, ["-copy", "none"] + args) == ref
            enc = M.Encoder(M.params_from_jpeg(src, **kw), max_batch=2)
            assert enc.transcode_host([src, padded]) == [ref, ref]
            enc.close()


# ---- 5. headers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TC.SOURCES))
def test_probe_fields(simt, name):
    want = TC.SOURCES[name]
    i = M.jpeg_info(TC.source(name))
    assert (i.image_width, i.image_height) == want["size"] and i.num_components == want["nc"] and i.data_precision == 8
    assert (i.h_samp_factor[0], i.v_samp_factor[0]) == want["samp0"]
    assert i.num_scans == want["scans"] and i.scans[0].restart_interval == want["ri"]
    assert i.jpeg_color_space == {"GRAYSCALE": M.CS_GRAYSCALE, "RGB": M.CS_RGB, "YCbCr": M.CS_YCBCR}[want["cs"]]
    assert i.sof_type in (0, 1)
    assert bool(i.saw_JFIF_marker) == (want["cs"] != "RGB") and bool(i.saw_Adobe_marker) == (want["cs"] == "RGB")
    total = 0
    for k in range(i.num_scans):
        sc = i.scans[k]
        assert TC.source(name)[sc.data_offset - 2 - (6 + 2 * sc.comps_in_scan):][:2] == b"\xff\xda"
        nxt = TC.source(name)[sc.data_offset + sc.data_size:][:2]
        assert nxt[0] == 0xFF and nxt[1] not in (0, 0xFF) and not 0xD0 <= nxt[1] <= 0xD7
        total += sc.comps_in_scan
        assert (sc.restart_markers > 0) == (sc.restart_interval > 0)
        ent = TC.source(name)[sc.data_offset:sc.data_offset + sc.data_size]
        assert sc.restart_markers == sum(1 for j in range(len(ent) - 1) if ent[j] == 0xFF and 0xD0 <= ent[j + 1] <= 0xD7)
    assert total == i.num_components
    if name == "jfif102":
        assert (i.JFIF_major_version, i.JFIF_minor_version, i.density_unit, i.X_density, i.Y_density) == (1, 2, 1, 72, 72)
    if name == "scans3_2x2_r2":
        assert [i.scans[k].restart_interval for k in range(3)] == [58, 30, 30]
        assert [i.scans[k].component_index[0] for k in range(3)] == [0, 1, 2]


def test_params_from_jpeg_against_the_oracle(simt):
    """what mjh_params_from_jpeg copies == oracle_lib.transcode_params of the parameters the source was encoded with"""
    data, _, src_p = TC.oracle_source()
    for kw in (dict(revert=True), dict(revert=True, optimize=True), dict(fastcrush=True, progressive=True), dict()):
        p = M.params_from_jpeg(data, **kw)
        okw = dict(kw)
        if not kw:
            okw = dict()
        o = O.transcode_params(src_p, **okw)
        assert (p.image_width, p.image_height, p.num_components) == (o.width, o.height, o.num_components)
        assert p.trellis_quant == 0 and p.optimize_coding == o.optimize_coding and p.num_scans == o.num_scans
        assert p.compress_profile == (M.PROFILE_FASTEST if kw.get("revert") else M.PROFILE_MAX_COMPRESSION)
        for c in range(3):
            assert (p.h_samp_factor[c], p.v_samp_factor[c]) == (o.h_samp[c], o.v_samp[c])
            assert list(p.quantval[p.quant_tbl_no[c]]) == list(o.qtbl[p.quant_tbl_no[c]])
    q = M.jpeg_info(TC.source("rgb"))
    p = M.params_from_jpeg(q, revert=True)
    assert p.color_transform == M.COLOR_NONE and p.write_JFIF_header == 0 and [p.component_id[c] for c in range(3)] == [82, 71, 66]
    assert [p.dc_tbl_no[c] for c in range(3)] == [0, 0, 0]
    g = M.params_from_jpeg(TC.source("gray_r5b"), revert=True)
    assert g.num_components == 1 and g.restart_interval == 0 and g.restart_in_rows == 0      # the source's interval is not copied


def test_mismatching_file_in_a_batch_is_named(simt):
    enc = M.Encoder(M.params_from_jpeg(TC.source("revert"), revert=True), max_batch=3)
    with pytest.raises(M.MjhError) as ei:
        enc.transcode_host([TC.source("revert"), TC.source("q90_2x1_r1"), TC.source("revert")])
    assert ei.value.code == M.EINVAL and "file 1" in str(ei.value) and "sampling factors" in str(ei.value)
    with pytest.raises(M.MjhError) as ei:
        enc.transcode_host([TC.source("oracle_baseline")])
    assert ei.value.code == M.EINVAL and "file 0" in str(ei.value) and "image size" in str(ei.value)
    assert enc.transcode_host([TC.source("revert")])[0] == TC.reference("revert", "revert")
    enc.close()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", list(TC.REFUSALS))
def test_refused_sources(simt, what):
    args, word = TC.REFUSALS[what]
    src = TC.cjpeg(TC.testorig(), args)
    with pytest.raises(M.MjhError) as ei:
        M.jpeg_info(src)
    assert ei.value.code == M.EUNSUPPORTED and word in str(ei.value)
    r = M.recompress([src], revert=True)[0]
    assert isinstance(r, M.MjhError) and r.code == M.EUNSUPPORTED


def test_trellis_encoder_is_refused(simt):
    p = M.params_from_jpeg(TC.source("revert"), revert=True)
    p.trellis_quant = 1
    p.optimize_coding = 1
    enc = M.Encoder(p, max_batch=1)
    with pytest.raises(M.MjhError) as ei:
        enc.transcode_host([TC.source("revert")])
    assert ei.value.code == M.EINVAL and "trellis" in str(ei.value)
    enc.close()


# ---- 7. untrusted input (the emulator's device buffers end at unmapped pages) -----------------------------------------------------
def test_truncated_files_fail(simt):
    src = TC.source("revert")
    info = M.jpeg_info(src)
    a, n = info.scans[0].data_offset, info.scans[0].data_size
    enc = M.Encoder(M.params_from_jpeg(src, revert=True, optimize=True), max_batch=1)
    cuts = list(range(a, a + n, 97))
    assert len(cuts) > 20
    for cut in cuts:
        with pytest.raises(M.MjhError) as ei:
            enc.transcode_host([src[:cut]])
        assert ei.value.code == M.EINVAL
    # truncated inside the data with the end marker kept: the header walk cannot see it, the decoder must
    for cut in cuts[1::4]:
        with pytest.raises(M.MjhError) as ei:
            enc.transcode_host([src[:cut] + b"\xff\xd9"])
        assert ei.value.code == M.EINVAL
    assert enc.transcode_host([src])[0] == TC.reference("revert", "revert_opt")
    enc.close()


def test_bit_flips_decode_as_the_reference_or_fail(simt):
    src = TC.source("revert")
    info = M.jpeg_info(src)
    a, n = info.scans[0].data_offset, info.scans[0].data_size
    rng = random.Random(20240607)
    enc = M.Encoder(M.params_from_jpeg(src, revert=True, optimize=True), max_batch=1)
    equal = failed = 0
    for _ in range(200):
        pos, bit = a + rng.randrange(n), rng.randrange(8)
        bad = bytearray(src)
        bad[pos] ^= 1 << bit
        bad = bytes(bad)
        status, ref = TC.jpegtran_status(bad, ["-copy", "none", "-revert", "-optimize"])
        try:
            out = enc.transcode_host([bad])[0]
        except M.MjhError as exc:
            assert exc.code == M.EINVAL
            failed += 1
            continue
        if status == 0:
            assert out == ref, "flip of bit %d at %d: a file that differs from the reference's" % (bit, pos)
            equal += 1
    assert equal >= 100, "%d of 200 flips gave the reference's bytes, %d failed" % (equal, failed)
    assert enc.transcode_host([src])[0] == TC.reference("revert", "revert_opt")
    enc.close()


def test_damaged_file_in_a_batch(simt):
    src = TC.source("revert")
    info = M.jpeg_info(src)
    a, n = info.scans[0].data_offset, info.scans[0].data_size
    bad = src[:a + n // 2] + src[a + n // 2 + 40:]                # 40 bytes of entropy data missing, every marker in place
    good2 = TC.source("revert_opt")
    ref = [TC.reference("revert", "revert_opt"), None, TC.reference("revert_opt", "revert_opt")]
    enc = M.Encoder(M.params_from_jpeg(src, revert=True, optimize=True), max_batch=3)
    with pytest.raises(M.MjhError) as ei:
        enc.transcode_host([src, bad, good2])
    assert ei.value.code == M.EINVAL and "file 1" in str(ei.value)
    assert [enc.transcode_status(i)[0] for i in range(3)] == [M.OK, M.EINVAL, M.OK]
    assert "Corrupt" in enc.transcode_status(1)[1]
    assert enc.transcode_host([src, good2]) == [ref[0], ref[2]]       # the encoder stays usable
    enc.close()
    out = M.recompress([src, bad, good2], revert=True, optimize=True)
    assert out[0] == ref[0] and out[2] == ref[2]
    assert isinstance(out[1], M.MjhError) and out[1].code == M.EINVAL


# ---- 8. recompress() over a mix of signatures -------------------------------------------------------------------------------------
def test_recompress_keeps_input_order(simt):
    names = ["revert", "gray_r5b", "8x8", "revert_opt", "rgb", "17x9", "jfif102", "s1x2", "1x1", "noise_q100", "scans3_2x2_r2", "revert"]
    random.Random(5).shuffle(names)
    for sw in ("revert_opt", "default"):
        outs = M.recompress([TC.source(s) for s in names], max_batch=4, **TC.SWITCHES[sw][0])
        for s, o in zip(names, outs):
            assert o == TC.reference(s, sw), "%s %s" % (s, sw)
