"""GPU suite (-m gpu): four-component JPEG files (Adobe-style CMYK and YCCK) on the chip -- decode(), decode_planes(),
decode_coefficients(), the TurboJPEG-signature library next to the reference's, and the unchanged djpeg on the stand-alone
libjpeg.so.62.  The cases are those of test_simt_cmyk.py (tests/cmyk_cases.py); every expected value comes from the reference at
test time and is compared for exact equality."""
import os

import pytest

import mozjpeg_amd as M
import cmyk_cases as K
import djpeg_cases as DJ
import tj_decompress_cases as TD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STANDALONE_DIR = os.path.join(ROOT, "mozjpeg_amd", "standalone")

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not (K.have_tools() and os.path.exists(os.path.join(STANDALONE_DIR, "libjpeg.so.62"))),
                                 reason="reference binaries and headers (oracle/_ref), tests/native/djpeg_client, the TurboJPEG-signature or the stand-alone library not built")]


@pytest.fixture(scope="module")
def R():
    return DJ.Runner(STANDALONE_DIR)


@pytest.fixture(scope="module")
def libs():
    if "simt" in os.path.basename(M.LIB_PATH or ""):
        pytest.skip("the TurboJPEG-signature library is linked to the device library, not to the emulator")
    return TD.load(TD.TJSHIM), TD.load(TD.TJLIB)


# ---- 1. pixels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,mode", K.PIXEL_CASES, ids=[K.case_id(c) for c in K.PIXEL_CASES])
def test_pixels(src, mode):
    K.check_pixels(M, src, mode)


@pytest.mark.parametrize("src,denom,fancy", K.SCALED_CASES, ids=[K.case_id(c) for c in K.SCALED_CASES])
def test_scaled(src, denom, fancy):
    K.check_scaled(M, src, denom, fancy)


def test_inverted_samples_stay_inverted():
    K.check_inverted_samples_stay_inverted(M)


# ---- 2. coefficients and planes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", K.COEF_SOURCES)
def test_coefficients(src):
    K.check_coefficients(M, src)


@pytest.mark.parametrize("src", K.PLANE_SOURCES)
def test_planes(src):
    K.check_planes(M, src)


# ---- 3. batches, progressive files, the probe, refusals -------------------------------------------------------------------------------
def test_batch_with_a_damaged_file():
    K.check_batch_with_a_damaged_file(M)


def test_mixed_batch():
    K.check_mixed_batch(M)


def test_progressive():
    K.check_progressive(M)


def test_info():
    K.check_info(M)


def test_refusals():
    K.check_refusals(M)


def test_nothing_is_written():
    K.check_nothing_is_written(M)


# ---- 4. the TurboJPEG-signature library -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.TJ_CHECKS))
def test_tj(libs, name):
    K.TJ_CHECKS[name](*libs)


# ---- 5. the stand-alone libjpeg.so.62 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,switches", K.DJPEG_PAIRS, ids=["%s-%s" % p for p in K.DJPEG_PAIRS])
def test_unchanged_djpeg(R, src, switches):
    K.check_djpeg(R, src, K.DJPEG_SWITCHES[switches])


def test_djpeg_refused_conversions(R):
    K.check_djpeg_refused_conversions(R)


@pytest.mark.parametrize("src", K.CLIENT_SOURCES)
def test_client(R, src):
    K.check_client(R, src)


@pytest.mark.parametrize("src", ["ycck2x2k_r2", "scans4_16", "tj_cmyk420"])
def test_read_coefficients(R, src):
    K.check_read_coefficients(R, src)
