"""GPU (-m gpu): the JPEG reader on valid sequential files that no libjpeg encoder writes, on the chip.  The families of
test_simt_streams.py (tests/stream_cases.py; files from tests/jpeg_writer.py at test time), plus the sizes the emulator cannot
afford: 1080p files whose every code word is 16 bits long, batches of files in different table shapes, and the slow-synchronisation
stream over the default subsequence length.  Every expected byte comes from the reference's jpegtran and every expected pixel from
its djpeg (oracle/_ref), both run at test time; equality is exact."""
import pytest

import mozjpeg_amd as M
import decode_cases as DC
import stream_cases as SC

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not SC.have_tools(), reason="reference cjpeg / jpegtran / djpeg not built (oracle/_ref)")]


@pytest.fixture
def subseq(monkeypatch):
    def set_(s):
        if s is None:
            monkeypatch.delenv("MJH_DECODE_SUBSEQ", raising=False)
        else:
            monkeypatch.setenv("MJH_DECODE_SUBSEQ", str(s))
    return set_


# ---- 1. every family ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.NAMES)
def test_premise(name):
    c = SC.case(name)
    SC.check_premise(M, c)
    assert M.jpeg_info(c.data).jpeg_color_space == SC.expected_colour_space(M, c)


@pytest.mark.parametrize("name,sw", SC.TRANSCODE_PAIRS, ids=["%s-%s" % p for p in SC.TRANSCODE_PAIRS])
def test_transcode_matches_jpegtran(name, sw):
    SC.check_transcode(M, SC.case(name), sw)


@pytest.mark.parametrize("name", SC.NAMES)
def test_decode_matches_djpeg(name):
    SC.check_decode(M, SC.case(name))


@pytest.mark.parametrize("name", SC.TRANSFORM_NAMES)
def test_transforms_match_jpegtran(name):
    SC.check_transforms(M, SC.case(name))


@pytest.mark.parametrize("seed", [1, 2])
def test_decoded_coefficients_equal_the_writers(seed):
    c = SC.case(("scans_2_0_1", "shape_full256")[seed - 1])
    SC.check_coefficients(M, c)


def test_marker_noise_changes_nothing():
    clean, noisy = SC.case("noise_clean"), SC.case("noise_markers")
    assert clean.data != noisy.data
    for sw in SC.CODINGS:
        assert SC.transcode(M, noisy.data, sw) == SC.transcode(M, clean.data, sw)
    for mode in DC.MODES:
        kw = DC.MODES[mode][0]
        assert SC.same(M.decode([noisy.data], **kw)[0], M.decode([clean.data], **kw)[0])


def test_fractional_sampling_is_refused():
    SC.check_fractional_refusal(M)


@pytest.mark.parametrize("w,h", SC.SMALL_SIZES, ids=["%dx%d" % s for s in SC.SMALL_SIZES])
def test_small_sizes(w, h):
    for samp in SC.SMALL_SAMPLINGS:
        SC.check_decode(M, SC.small_case(w, h, samp), layouts=SC.SMALL_LAYOUTS)


@pytest.mark.parametrize("name", list(SC.OUT_OF_RANGE))
def test_out_of_range_amplitudes(name):
    SC.check_out_of_range(M, name)


@pytest.mark.parametrize("S", [16, None])
@pytest.mark.parametrize("name", SC.SUBSEQ_CASES)
def test_long_codes_over_many_subsequences(subseq, name, S):
    c = SC.case(name)
    assert c.stats["long_share"] >= 0.5
    st = SC.check_subseq(M, c, S, subseq)
    if S:
        assert st["subseq"] == S and st["rounds"] >= 3


# ---- 2. what the emulator cannot afford --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(SC.BIG_SCANS))
def test_1080p_every_code_16_bits(subseq, kind):
    c = SC.big_case(kind)
    SC.check_premise(M, c)
    assert c.stats["long_share"] == 1.0
    st = SC.check_subseq(M, c, None, subseq)
    assert st["rounds"] >= 3
    SC.check_transcode(M, c, "fastcrush_progressive")
    SC.check_decode(M, c)


def test_1080p_batch_of_different_table_shapes():
    cases = SC.big_batch()
    assert len(set(repr(sorted(c.stats["scans"][0].items())) for c in cases)) == len(cases), "two files share their Huffman tables"
    SC.check_batch(M, cases)


def test_64_small_files_of_mixed_tables_in_one_call():
    cases = SC.small_batch()
    assert len(cases) == 64 and len(set(M._signature(M.jpeg_info(c.data)) for c in cases)) == 1
    SC.check_batch(M, cases)
    outs = M.decode([c.data for c in cases], max_batch=64)
    assert all(SC.same(o, DC.djpeg(c.data)) for o, c in zip(outs, cases))


def test_slow_synchronisation_512(subseq):
    c = SC.slow_sync(512)
    st, nsub = SC.check_slow_sync(M, c, None, subseq)
    assert nsub >= 100, "%d subsequences of %d bytes" % (nsub, st["subseq"])
    print("slow synchronisation: %d rounds for %d subsequences of %d bytes" % (st["rounds"], nsub, st["subseq"]))


def test_slow_synchronisation_96(subseq):
    st, nsub = SC.check_slow_sync(M, SC.case("slow_sync_96"), 16, subseq)
    assert st["subseq"] == 16 and nsub > 100


def test_subsequences_that_start_on_a_stuffed_zero(subseq):
    SC.check_stuffed_boundaries(M, SC.stuffed_boundaries(), subseq)
