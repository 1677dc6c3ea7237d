"""CPU suite: the JPEG reader (mjh_jpeg_probe, the Huffman decoder kernels of mjh_decode.hip, the pixel kernels of mjh_idct.hip) on
valid sequential files that no libjpeg encoder writes, executed by the lock-step wave64 emulator (tools/simt, SIMT_STRICT).  The
files come from tests/jpeg_writer.py at test time (tests/stream_cases.py holds the cases); every expected byte comes from the
reference's jpegtran and every expected pixel from its djpeg, both run at test time, and equality is exact."""
import os
import sys

import numpy as np
import pytest

import mozjpeg_amd as M
import decode_cases as DC
import jpeg_writer as W
import stream_cases as SC
import transcode_cases as TC
import transform_cases as XC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "simt"))

pytestmark = pytest.mark.skipif(not SC.have_tools(), reason="reference cjpeg / jpegtran / djpeg not built (oracle/_ref)")


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


# ---- 0. the writer ----------------------------------------------------------------------------------------------------------------
def test_writer_tables_hold_no_all_ones_code():
    rng = np.random.default_rng(3)
    for shape in W.SHAPES:
        for n in (1, 2, 7, 8, 40, 162, 256):
            freq = np.zeros(256, np.int64)
            freq[rng.choice(256, n, replace=False)] = rng.integers(1, 10 ** rng.integers(1, 7), n)
            for dc in (False, True):
                if dc:
                    freq[16:] = 0
                bits, vals = W.make_table(freq, shape, dc)
                code, size = W.canonical_codes(bits, vals)          # (asserts: no all-ones code word)
                assert sum(bits[1:]) == len(vals) == len(set(vals)) and all(size[s] for s in range(256) if freq[s])
                assert sum(b / (1 << l) for l, b in enumerate(bits) if l) < 1.0
                if shape == "full256" and not dc:
                    assert len(vals) == 256


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_writer_roundtrip(simt, seed):
    """random descriptions: the reference's djpeg and jpegtran accept the file, and the coefficients the device decodes are the
    arrays it was written from"""
    rng = np.random.default_rng(seed)
    samp = [SC.S420, ((2, 1), (1, 1), (1, 1)), ((1, 1), (1, 1), (1, 1)), ((2, 2), (2, 1), (1, 2))][seed - 1]
    comps = SC.ycc(*samp) if seed != 3 else SC.gray()
    w, h = int(rng.integers(9, 70)), int(rng.integers(9, 70))
    shapes = [str(s) for s in rng.choice(W.SHAPES, 3)]
    if len(comps) == 1:
        scans = [dict(comps=[0], dc=[int(rng.integers(4))], ac=[int(rng.integers(4))], ri=int(rng.integers(0, 5)), shape=shapes[0])]
    elif seed & 1:
        scans = [dict(comps=[0, 1, 2], dc=[int(x) for x in rng.integers(0, 4, 3)], ac=[int(x) for x in rng.integers(0, 4, 3)], ri=int(rng.integers(0, 5)), shape=shapes[0])]
    else:
        scans = [dict(comps=[k], dc=[int(rng.integers(4))], ac=[int(rng.integers(4))], ri=int(rng.integers(0, 9)), shape=shapes[k]) for k in (1, 0, 2)]
    c = SC.build(300 + seed, w, h, comps, scans=scans, sof=1, qtables={t: SC.quant(seed * 11 + t, 1, 500, 1) for t in set(x[3] for x in comps)})
    SC.check_premise(M, c)
    SC.check_coefficients(M, c)


# ---- 1. every family: premise, bytes == jpegtran's, pixels == djpeg's, transforms -----------------------------------------------------
@pytest.mark.parametrize("name", SC.NAMES)
def test_premise(simt, name):
    c = SC.case(name)
    SC.check_premise(M, c)
    assert M.jpeg_info(c.data).jpeg_color_space == SC.expected_colour_space(M, c)


@pytest.mark.parametrize("name,sw", SC.TRANSCODE_PAIRS, ids=["%s-%s" % p for p in SC.TRANSCODE_PAIRS])
def test_transcode_matches_jpegtran(simt, name, sw):
    SC.check_transcode(M, SC.case(name), sw)


@pytest.mark.parametrize("name", SC.NAMES)
def test_decode_matches_djpeg(simt, name):
    SC.check_decode(M, SC.case(name))


@pytest.mark.parametrize("name", SC.TRANSFORM_NAMES)
def test_transforms_match_jpegtran(simt, name):
    SC.check_transforms(M, SC.case(name))


@pytest.mark.parametrize("name", SC.GRAY_FORCED)
def test_gray_frame_header_is_forced_to_1x1(simt, name):
    """a gray source with other sampling factors: the reference writes 1x1 into SOF (jtransform_adjust_parameters), with and
    without a transform; the default switches (recompress: the smaller of source and result) agree as well"""
    c = SC.case(name)
    assert (c.comps[0][1], c.comps[0][2]) != (1, 1)
    for sw in SC.CODINGS:
        out = SC.transcode(M, c.data, sw)
        assert XC.frame(M, out)[3] == ((1, 1),)
    status, ref = TC.jpegtran_status(c.data, ["-copy", "none"])
    assert status == 0 and M.recompress([c.data])[0] == (ref if len(ref) <= len(c.data) else c.data)
    # a batch of gray files whose source factors differ: they share every parameter the encoder has
    enc = M.Encoder(M.params_from_jpeg(c.data, revert=True), max_batch=2)
    a = SC.build(171, 45, 37, SC.gray(1, 1), qtables=c.qtables)
    outs = enc.transcode_host([c.data, a.data])
    enc.close()
    assert outs[0] == TC.jpegtran_status(c.data, ["-copy", "none", "-revert"])[1]
    assert outs[1] == TC.jpegtran_status(a.data, ["-copy", "none", "-revert"])[1]


def test_marker_noise_changes_nothing(simt):
    clean, noisy = SC.case("noise_clean"), SC.case("noise_markers")
    assert clean.data != noisy.data and len(noisy.data) > len(clean.data) + 80
    for sw in SC.CODINGS:
        assert SC.transcode(M, noisy.data, sw) == SC.transcode(M, clean.data, sw)
    for mode in DC.MODES:
        kw = DC.MODES[mode][0]
        assert SC.same(M.decode([noisy.data], **kw)[0], M.decode([clean.data], **kw)[0])


def test_fractional_sampling_is_refused(simt):
    SC.check_fractional_refusal(M)


# ---- 2. small sizes: downsampled widths of 1, 2 and 3, every partial 4-pixel store group -----------------------------------------------
@pytest.mark.parametrize("w,h", SC.SMALL_SIZES, ids=["%dx%d" % s for s in SC.SMALL_SIZES])
def test_small_sizes(simt, w, h):
    for samp in SC.SMALL_SAMPLINGS:
        c = SC.small_case(w, h, samp)
        assert (M.jpeg_info(c.data).image_width, M.jpeg_info(c.data).image_height) == (w, h)
        SC.check_decode(M, c, layouts=SC.SMALL_LAYOUTS)


# ---- 3. amplitudes beyond +-1023 / DC differences beyond +-2047 ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.OUT_OF_RANGE))
def test_out_of_range_amplitudes(simt, name):
    SC.check_out_of_range(M, name)


# ---- 4. synchronisation ------------------------------------------------------------------------------------------------------------
def test_slow_synchronisation(simt, subseq):
    st, nsub = SC.check_slow_sync(M, SC.case("slow_sync_96"), 16, subseq)
    assert st["subseq"] == 16 and nsub > 100
    print("slow synchronisation: %d rounds for %d subsequences" % (st["rounds"], nsub))


@pytest.mark.parametrize("S", [16, None])
@pytest.mark.parametrize("name", SC.SUBSEQ_CASES)
def test_long_codes_over_many_subsequences(simt, subseq, name, S):
    c = SC.case(name)
    assert c.stats["long_share"] >= 0.5
    st = SC.check_subseq(M, c, S, subseq)
    if S:
        assert st["subseq"] == S and st["rounds"] >= 3


def test_subsequences_that_start_on_a_stuffed_zero(simt, subseq):
    st, nsub = SC.check_stuffed_boundaries(M, SC.stuffed_boundaries(), subseq)
    print("stuffed boundaries: %d rounds for %d subsequences" % (st["rounds"], nsub))


# ---- 5. damage only these tables can show --------------------------------------------------------------------------------------------
def test_undefined_16_bit_code_is_reported(simt):
    """a code word of 16 bits beyond the last one its table defines, in a file whose every code is 16 bits long.  The missing symbol
    is the EOB of the one block that has one, so reading the undefined code as symbol 0 (as the reference does, with a warning)
    decodes the right number of blocks with nothing left over: only the check of the code itself can tell.  The reference warns
    (JWRN_HUFF_BAD_CODE, exit 2); decoding and re-compression report the file as corrupt, and its neighbour in the batch is fine."""
    c = SC.lone_eob_case()
    bits, vals = c.stats["scans"][0][("ac", 0)]
    bad, sym = SC.undefine_rarest_code(c)
    assert sym == vals[-1] == 0 and bits[16] == len(vals) == 4 and len(bad) == len(c.data) - 1
    assert DC.djpeg_status(c.data)[0] == 0
    assert DC.djpeg_status(bad)[0] == 2 and TC.jpegtran_status(bad, ["-copy", "none", "-revert"])[0] == 2
    enc = M.Encoder(M.params_from_jpeg(c.data, revert=True), max_batch=2)
    for call in (enc.decode_host, enc.transcode_host):
        res = call([bad, c.data], errors="return")
        assert isinstance(res[0], M.MjhError) and res[0].code == M.EINVAL and "Corrupt" in str(res[0]) and res[1] is None
    assert SC.same(enc.decode_host([c.data])[0], DC.djpeg(c.data))
    enc.close()
