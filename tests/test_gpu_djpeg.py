"""GPU suite: the libjpeg decompress API of the stand-alone libjpeg.so.62 (an unchanged djpeg, tests/native/djpeg_client.c) and
RGB565 output on the chip.  The cases are those of test_simt_djpeg.py (tests/djpeg_cases.py); every expected byte comes from the
reference at test time and is compared for exact equality.  Damaged files run on the emulator only, as in test_gpu_decode.py."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mozjpeg_amd as M
import oracle_lib as O
import decode_cases as DC
import transcode_cases as TC
import djpeg_cases as DJ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STANDALONE_DIR = os.path.join(ROOT, "mozjpeg_amd", "standalone")

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not (DJ.have_tools() and os.path.exists(os.path.join(STANDALONE_DIR, "libjpeg.so.62"))),
                                 reason="reference djpeg / libjpeg.so.62, tests/native/djpeg_client or the stand-alone library not built")]


@pytest.fixture(scope="module")
def R():
    return DJ.Runner(STANDALONE_DIR)


# ---- 1. RGB565 through the C ABI ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dither,fancy", DJ.PAIRS_565, ids=DJ.PAIR_IDS_565)
def test_rgb565_matches_djpeg(src, dither, fancy):
    DJ.check_565(M, src, dither, fancy)


@pytest.mark.parametrize("src,scale", DJ.SCALED_565, ids=["%s-%s" % (s, sc.replace("/", "_")) for s, sc in DJ.SCALED_565])
def test_rgb565_scaled(src, scale):
    for dither in (True, False):
        DJ.check_565(M, src, dither, True, scale)


def test_rgb565_batch():
    DJ.check_565_batch(M)


def test_rgb565_dither_goes_in_before_the_clamp():
    DJ.check_565_dither_before_clamp(M)


def test_rgb565_refusals():
    DJ.check_565_refusals(M)


# ---- 2. the unchanged djpeg on the stand-alone library ------------------------------------------------------------------------------
def test_only_the_standalone_library_is_mapped(R, tmp_path):
    """the loader's own trace names every object it maps: this libjpeg.so.62, never the reference's"""
    inp, outp = str(tmp_path / "in.jpg"), str(tmp_path / "out.ppm")
    with open(inp, "wb") as f:
        f.write(DC.source("revert"))
    r = R.run(True, [DC.DJPEG, "-outfile", outp, inp], env={"LD_DEBUG": "libs"})
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    loaded = [ln for ln in r.stderr.decode(errors="replace").splitlines() if "calling init:" in ln]
    assert any(STANDALONE_DIR in ln and "libjpeg.so.62" in ln for ln in loaded), loaded
    assert any("libmozjpeg_hip.so" in ln for ln in loaded), loaded
    assert not any(O.REF_DIR in ln and "libjpeg" in ln for ln in loaded), "the reference's libjpeg was loaded"
    assert np.array_equal(DC.parse_pnm(open(outp, "rb").read()), DC.reference("revert", "default"))


@pytest.mark.parametrize("src,switches", DJ.DJPEG_PAIRS, ids=["%s-%s" % p for p in DJ.DJPEG_PAIRS])
def test_unchanged_djpeg(R, src, switches):
    DJ.check_djpeg(R, src, DJ.DJPEG_SWITCHES[switches])


def test_djpeg_from_stdin(R):
    DJ.check_djpeg(R, "revert", [], how="stdin")
    DJ.check_djpeg(R, "gray_r5b", ["-bmp"], how="stdin")


def test_djpeg_verbose_prints_the_same(R):
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


def test_eight_threads_with_an_object_each(R):
    names = ["revert", "gray_r5b", "rgb", "q90_2x1_r1", "17x9", "33x47", "s_mixed", "revert_opt"]
    R.both_client("threads", [DC.source(s) for s in names], -len(names))


# ---- 4. full size -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files_4k():
    return [TC.cjpeg(O.synthetic_frame(3840, 2160, seed=300 + i), ["-revert", "-quality", "75", "-sample", "2x2"]) for i in range(4)]


def test_4k_files_through_djpeg(R, files_4k):
    for i, f in enumerate(files_4k):
        ref = R.djpeg(False, f, [])
        out = R.djpeg(True, f, [])
        assert ref[0] == 0 and out[0] == 0, out[2][-2000:]
        assert out[1] == ref[1], "file %d" % i


def test_4k_files_rgb565_in_one_batch(files_4k):
    outs = M.decode(files_4k, color="rgb565")
    for f, o in zip(files_4k, outs):
        assert DJ.same565(o, DJ.djpeg565(f))
