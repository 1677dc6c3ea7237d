"""CPU suite: decoding JPEG files at reduced size (mjh_decode_host with scale_num / scale_denom, djpeg -scale 1/2, 1/4, 1/8) with the
kernels of mjh_decode.hip and mjh_idct.hip executed by the lock-step wave64 emulator (tools/simt, SIMT_STRICT), whose device buffers
end at unmapped pages.  Every expected pixel comes from the reference's djpeg -scale at test time and is compared for exact
equality, the array shape included (tests/scale_cases.py)."""
import os
import random
import sys

import pytest

import mozjpeg_amd as M
import decode_cases as DC
import scale_cases as SC
import transcode_cases as TC

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


@pytest.mark.parametrize("src,mode,sc", SC.CASES, ids=[SC.case_id(c) for c in SC.CASES])
def test_scaled_decode_matches_djpeg(simt, src, mode, sc):
    SC.check_case(M, src, mode, sc)


@pytest.mark.parametrize("src,layout,sc", SC.LAYOUT_CASES, ids=[SC.case_id(c) for c in SC.LAYOUT_CASES])
def test_scaled_four_byte_layout(simt, src, layout, sc):
    SC.check_layout_case(M, src, layout, sc)


@pytest.mark.parametrize("src,frac", SC.FRACTION_CASES, ids=[SC.case_id(c) for c in SC.FRACTION_CASES])
def test_fraction_is_resolved_as_djpeg_does(simt, src, frac):
    SC.check_fraction(M, src, frac)


def test_every_transform_size_is_reached(simt):
    SC.check_every_transform_size_is_reached(M)


def test_one_encoder_serves_every_scale(simt):
    SC.check_one_encoder_serves_every_scale(M)


def test_mixed_batch_with_a_damaged_file(simt):
    SC.check_mixed_batch(M)


def test_refusals(simt):
    SC.check_refusals(M)


# ---- untrusted input at 1/8: the reduced planes are the new bounds ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["revert", "s_mixed"])
def test_truncated_files_fail_at_one_eighth(simt, name):
    src = SC.source(name)
    info = M.jpeg_info(src)
    a, n = info.scans[0].data_offset, info.scans[0].data_size
    enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=1)
    cuts = list(range(a, a + n, 197))
    assert len(cuts) > 10
    for cut in cuts:
        with pytest.raises(M.MjhError) as ei:
            enc.decode_host([src[:cut]], scale="1/8")
        assert ei.value.code == M.EINVAL
    for cut in cuts[1::4]:
        with pytest.raises(M.MjhError) as ei:
            enc.decode_host([src[:cut] + b"\xff\xd9"], scale="1/8")
        assert ei.value.code == M.EINVAL
    assert SC.same(enc.decode_host([src], scale="1/8")[0], SC.reference(name, "default", "1/8"))
    enc.close()


def test_bit_flips_at_one_eighth_decode_as_the_reference_or_fail(simt):
    """the seeded flips of test_simt_decode.py (same seed, same source, the first 100) at 1/8: a file the reference decodes
    without a warning gives its pixels, the others fail"""
    src = TC.source("revert")
    info = M.jpeg_info(src)
    a, n = info.scans[0].data_offset, info.scans[0].data_size
    rng = random.Random(20240607)
    enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=1)
    equal = failed = 0
    for _ in range(100):
        pos, bit = a + rng.randrange(n), rng.randrange(8)
        bad = bytearray(src)
        bad[pos] ^= 1 << bit
        bad = bytes(bad)
        status, ref = DC.djpeg_status(bad, ["-scale", "1/8"])
        try:
            out = enc.decode_host([bad], scale="1/8")[0]
        except M.MjhError as exc:
            assert exc.code == M.EINVAL
            failed += 1
            continue
        if status == 0:
            assert SC.same(out, ref), "flip of bit %d at %d: pixels that differ from the reference's" % (bit, pos)
            equal += 1
    print("bit flips at 1/8: %d equal, %d failed" % (equal, failed))
    assert equal >= 50, "%d of 100 flips gave the reference's pixels, %d failed" % (equal, failed)
    assert SC.same(enc.decode_host([src], scale="1/8")[0], SC.reference("revert", "default", "1/8"))
    enc.close()
