"""CPU suite: the libjpeg decompress API of the stand-alone libjpeg.so.62 and RGB565 output, with the kernels executed by the
lock-step wave64 emulator (tools/simt, SIMT_STRICT): the libraries on the emulator through fuzz_cjpeg.dropin_dir().  Every expected
byte comes from the reference at test time (tests/djpeg_cases.py); comparison is exact equality."""
import os
import sys

import pytest

import mozjpeg_amd as M
import decode_cases as DC
import transcode_cases as TC
import djpeg_cases as DJ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "simt"))

pytestmark = pytest.mark.skipif(not DJ.have_tools(), reason="reference djpeg / libjpeg.so.62 or tests/native/djpeg_client not built")


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


@pytest.fixture(scope="module")
def R():
    """the stand-alone libjpeg.so.62 next to the emulator build of libmozjpeg_hip.so"""
    import fuzz_cjpeg
    return DJ.Runner(os.path.join(fuzz_cjpeg.dropin_dir(), "standalone"), env={"SIMT_STRICT": "1"})


# ---- 1. RGB565 through the C ABI ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dither,fancy", DJ.PAIRS_565, ids=DJ.PAIR_IDS_565)
def test_rgb565_matches_djpeg(simt, src, dither, fancy):
    DJ.check_565(M, src, dither, fancy)


@pytest.mark.parametrize("src,scale", DJ.SCALED_565, ids=["%s-%s" % (s, sc.replace("/", "_")) for s, sc in DJ.SCALED_565])
def test_rgb565_scaled(simt, src, scale):
    for dither in (True, False):
        DJ.check_565(M, src, dither, True, scale)


def test_rgb565_batch(simt):
    DJ.check_565_batch(M)


def test_rgb565_dither_goes_in_before_the_clamp(simt):
    DJ.check_565_dither_before_clamp(M)


def test_rgb565_refusals(simt):
    DJ.check_565_refusals(M)


# ---- 2. the unchanged djpeg on the stand-alone library ------------------------------------------------------------------------------
@pytest.mark.parametrize("src,switches", DJ.DJPEG_PAIRS, ids=["%s-%s" % p for p in DJ.DJPEG_PAIRS])
def test_unchanged_djpeg(R, src, switches):
    DJ.check_djpeg(R, src, DJ.DJPEG_SWITCHES[switches])


def test_djpeg_from_stdin(R):
    DJ.check_djpeg(R, "revert", [], how="stdin")
    DJ.check_djpeg(R, "gray_r5b", ["-bmp"], how="stdin")


def test_djpeg_verbose_prints_the_same(R):
    """-verbose: the marker reader's trace messages, and COM / APP12 through djpeg's own marker processor (jpeg_getc on the source)"""
    out = DJ.check_djpeg(R, "com", ["-verbose"], stderr=True)
    assert b"made for the djpeg test" in out[2] and b"Start Of Frame" in out[2]
    DJ.check_djpeg(R, "com", ["-verbose", "-verbose"], stderr=True)
    DJ.check_djpeg(R, "rgb", ["-verbose"], stderr=True)


def test_djpeg_extracts_the_icc_profile(R):
    out = DJ.check_djpeg(R, "icc", ["-icc", "@EXTRA@"])
    assert out[3] == DJ.icc_source()[1]


@pytest.mark.parametrize("what", list(DJ.DJPEG_REFUSED))
def test_djpeg_refused_switches(R, what):
    switches, word = DJ.DJPEG_REFUSED[what]
    DJ.check_djpeg_refused(R, DC.source("revert"), switches, word)


@pytest.mark.parametrize("what", list(TC.REFUSALS))
def test_djpeg_refused_sources(R, what):
    args, word = TC.REFUSALS[what]
    DJ.check_djpeg_refused(R, TC.cjpeg(TC.testorig(), args), [], word)


# ---- 3. the API beyond what djpeg reaches (tests/native/djpeg_client.c) -------------------------------------------------------------
@pytest.mark.parametrize("case", list(DJ.FIELD_CASES))
def test_fields(R, case):
    DJ.check_fields(R, case)


def test_saved_markers(R):
    out = R.both_client("markers", [DJ.markers_source()])
    assert "icc 3000 bytes" in out[1] and out[1].count("marker 0x") == 6


@pytest.mark.parametrize("cs", DJ.RGB_FAMILY)
def test_out_color_spaces(R, cs):
    for src in ("revert", "gray_r5b", "rgb"):
        R.both_client("pixels", [DC.source(src)], 1, (cs, 1, 1))
    if cs == DJ.JCS_RGB565:
        R.both_client("pixels", [DC.source("revert")], 1, (cs, 1, 0))


def test_unsupported_out_color_spaces(R):
    for cs in (3, 4, 5):                                  # JCS_YCbCr, JCS_CMYK, JCS_YCCK
        rc, out, _ = R.client(True, "pixels", [DC.source("revert")], 1, (cs, 1, 1))
        assert rc == 1 and "Unsupported color conversion request" in out, out


@pytest.mark.parametrize("src", ["revert", "gray_r5b", "q90_2x1_r1"])
def test_rows_per_call(R, src):
    DJ.check_rows_per_call(R, src)


@pytest.mark.parametrize("src", ["revert", "noise_q100", "gray_r5b"])
def test_raw_data(R, src):
    out = R.both_client("raw", [DC.source(src)], 1)
    assert ", 0 bytes touched" in out[1]


def test_two_images_in_one_buffer(R):
    R.both_client("two", [DC.source("revert"), DC.source("gray_r5b")], 1)
    R.both_client("two", [DC.source("17x9"), DC.source("17x9")], 1)


def test_abbreviated_datastreams(R):
    rc, text, files = R.client(False, "mkabbrev", [], 2)
    assert rc == 0 and files[0] and files[1], text
    assert b"\xff\xdb" not in files[1][:60] and b"\xff\xc4" not in files[1]      # the image defines no table
    R.both_client("abbrev", files, 1)


def test_abort_after_the_header(R):
    R.both_client("abort", [DJ.markers_source(), DC.source("q90_2x1_r1")], 1)


def test_damaged_data_is_fatal(R):
    DJ.check_damaged(R)
