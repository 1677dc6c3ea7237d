"""CPU suite: four-component JPEG files (Adobe-style CMYK and YCCK) through decode(), decode_planes(), decode_coefficients(), the
TurboJPEG-signature library and the stand-alone libjpeg.so.62, with the kernels of mjh_decode.hip, mjh_decode_prog.hip and mjh_idct.hip
(k_upcolor4 among them) executed by the lock-step wave64 emulator (tools/simt, SIMT_STRICT).  Every expected value comes from the
reference at test time (tests/cmyk_cases.py); every comparison is exact equality."""
import json
import os
import shutil
import subprocess
import sys

import pytest

import mozjpeg_amd as M
import cmyk_cases as K
import djpeg_cases as DJ
import tj_decompress_cases as TD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "simt"))

pytestmark = pytest.mark.skipif(not K.have_tools(), reason="reference binaries and headers (oracle/_ref), tests/native/djpeg_client or the TurboJPEG-signature library not built")


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


@pytest.fixture(scope="module")
def tj_results():
    """every TurboJPEG check in ONE child process: a process holds one library named libmozjpeg_hip.so, and this one may hold the device's"""
    import fuzz_cjpeg
    dst = os.path.join(fuzz_cjpeg.dropin_dir(), "libmozjpeg_hip_turbojpeg.so")
    if not os.path.exists(dst) or os.path.getmtime(dst) < os.path.getmtime(TD.TJSHIM):
        shutil.copy2(TD.TJSHIM, dst)
    env = dict(os.environ, SIMT_STRICT="1", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + sys.path))
    env.pop("MOZJPEG_HIP_TJ_DECOMPRESS", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cmyk_cases.py"), dst], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1200)
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("CMYK_TJ_RESULTS ")]
    assert r.returncode == 0 and lines, "the child ended with %d: %s" % (r.returncode, r.stderr.decode()[-2000:])
    return json.loads(lines[-1].split(" ", 1)[1])


def test_the_reference_reads_the_sources():
    K.check_sources_are_read_by_the_reference()


# ---- 1. pixels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,mode", K.PIXEL_CASES, ids=[K.case_id(c) for c in K.PIXEL_CASES])
def test_pixels(simt, src, mode):
    K.check_pixels(M, src, mode)


@pytest.mark.parametrize("src,denom,fancy", K.SCALED_CASES, ids=[K.case_id(c) for c in K.SCALED_CASES])
def test_scaled(simt, src, denom, fancy):
    K.check_scaled(M, src, denom, fancy)


def test_inverted_samples_stay_inverted(simt):
    K.check_inverted_samples_stay_inverted(M)


# ---- 2. coefficients and planes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", K.COEF_SOURCES)
def test_coefficients(simt, src):
    K.check_coefficients(M, src)


@pytest.mark.parametrize("src", K.PLANE_SOURCES)
def test_planes(simt, src):
    K.check_planes(M, src)


# ---- 3. batches, progressive files, the probe, refusals -------------------------------------------------------------------------------
def test_batch_with_a_damaged_file(simt):
    K.check_batch_with_a_damaged_file(M)


def test_mixed_batch(simt):
    K.check_mixed_batch(M)


def test_progressive(simt):
    K.check_progressive(M)


def test_info(simt):
    K.check_info(M)


def test_refusals(simt):
    K.check_refusals(M)


def test_nothing_is_written(simt):
    K.check_nothing_is_written(M)


# ---- 4. the TurboJPEG-signature library -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.TJ_CHECKS))
def test_tj(tj_results, name):
    assert tj_results[name] == "ok", tj_results[name]


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
