"""CPU suite: decoding a region of a JPEG file (mjh_decode_opts.crop_x / crop_y / crop_w / crop_h: djpeg -crop WxH+X+Y;
k_idct_region, k_idct_region_scaled, k_upcolor_region and k_upcolor_565_region of mjh_idct.hip, and the restart segments the
host leaves out) with the kernels executed by the lock-step wave64 emulator (tools/simt, SIMT_STRICT), whose device buffers end
at unmapped pages.  Every expected pixel comes from the reference's djpeg -crop at test time and is compared for exact equality,
the array shape included (tests/region_cases.py)."""
import ctypes
import os
import sys

import pytest

import mozjpeg_amd as M
import region_cases as RG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "simt"))

pytestmark = pytest.mark.skipif(not RG.have_tools(), reason="reference cjpeg / jpegtran / djpeg not built (oracle/_ref)")


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


@pytest.mark.parametrize("src,mode", RG.CASES, ids=[RG.case_id(c) for c in RG.CASES])
def test_every_region_matches_djpeg_crop(simt, src, mode):
    RG.check_case(M, src, mode)


def test_premise_of_the_case_list(simt):
    RG.check_premise(M)


@pytest.mark.parametrize("src", RG.LAYOUT_SOURCES)
def test_layouts_and_bottom_up(simt, src):
    RG.check_layout(M, src)


needs_client = pytest.mark.skipif(not RG.have_client(), reason="reference libjpeg.so.62 or tests/native/region_client not built")


@needs_client
@pytest.mark.parametrize("src,dither,scale", RG.CASES_565, ids=[RG.case_id(c) for c in RG.CASES_565])
def test_rgb565_regions(simt, src, dither, scale):
    RG.check_565(M, src, dither, scale)


def test_restart_segments_outside_the_region_are_left_out(simt):
    RG.check_pruning(M)


def test_progressive_and_arithmetic_sources(simt):
    RG.check_other_entropy_coders(M)


def test_one_encoder_serves_regions_and_whole_images(simt):
    RG.check_one_encoder(M)


def test_batch_with_a_damaged_file_and_the_device_buffer(simt):
    RG.check_batch(M, ctypes.string_at)                  # (the emulator's device memory is the process's own)


def test_refusals(simt):
    RG.check_refusals(M)


# ---- the TurboJPEG library over the emulator, MOZJPEG_HIP_REGIONS=1 -------------------------------------------------------------------
import json  # noqa: E402
import shutil  # noqa: E402
import subprocess  # noqa: E402

import tj_decompress_cases as TD  # noqa: E402

needs_tj = pytest.mark.skipif(not TD.have_tools(), reason="reference binaries (oracle/_ref) or the TurboJPEG-signature library are not built")


@pytest.fixture(scope="module")
def tj_results():
    import fuzz_cjpeg
    dst = os.path.join(fuzz_cjpeg.dropin_dir(), "libmozjpeg_hip_turbojpeg.so")
    if not os.path.exists(dst) or os.path.getmtime(dst) < os.path.getmtime(TD.TJSHIM):
        shutil.copy2(TD.TJSHIM, dst)
    env = dict(os.environ, SIMT_STRICT="1", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + sys.path))
    env.pop("MOZJPEG_HIP_TJ_DECOMPRESS", None)
    env.pop(RG.ENV, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "region_cases.py"), dst], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1200)
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("REGION_TJ_RESULTS ")]
    assert r.returncode == 0 and lines, "the child ended with %d: %s" % (r.returncode, r.stderr.decode()[-2000:])
    return json.loads(lines[-1].split(" ", 1)[1])


@needs_tj
@pytest.mark.parametrize("name", list(RG.TJ_CHECKS))
def test_turbojpeg_library(tj_results, name):
    assert tj_results[name] == "ok", tj_results[name]


# ---- the stand-alone libjpeg.so.62 over the emulator, MOZJPEG_HIP_REGIONS=1 ---------------------------------------------------------
import djpeg_cases as DJ  # noqa: E402

needs_djpeg = pytest.mark.skipif(not DJ.have_tools(), reason="reference djpeg / libjpeg.so.62 or tests/native/djpeg_client not built")


@pytest.fixture(scope="module")
def standalone_dir():
    import fuzz_cjpeg
    return os.path.join(fuzz_cjpeg.dropin_dir(), "standalone")


@needs_djpeg
@pytest.mark.parametrize("src,switches", RG.DJPEG_PAIRS, ids=["%s-%s" % p for p in RG.DJPEG_PAIRS])
def test_unchanged_djpeg_with_the_variable(standalone_dir, src, switches):
    RG.check_djpeg(DJ.Runner(standalone_dir, env={"SIMT_STRICT": "1", RG.ENV: "1"}), src, switches)


@needs_djpeg
def test_unchanged_djpeg_refuses_without_the_variable(standalone_dir):
    RG.check_djpeg_refuses_without_the_variable(DJ.Runner(standalone_dir, env={"SIMT_STRICT": "1"}))


@needs_client
@pytest.mark.parametrize("case", list(RG.CLIENT_CASES))
def test_libjpeg_client_on_both_libraries(standalone_dir, case):
    RG.check_client(standalone_dir, {"SIMT_STRICT": "1", RG.ENV: "1"}, case)
