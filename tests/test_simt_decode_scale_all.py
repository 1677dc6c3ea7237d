"""CPU suite: decoding at the twelve other IDCT sizes (mjh_decode_opts.all_scales: djpeg -scale 3/8, 5/8, 6/8, 7/8, 9/8 to 16/8;
k_idct_sized of mjh_idct.hip) with the kernels executed by the lock-step wave64 emulator (tools/simt, SIMT_STRICT), whose device
buffers end at unmapped pages.  Every expected pixel comes from the reference's djpeg -scale at test time and is compared for
exact equality, the array shape included (tests/scale_all_cases.py)."""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import pytest

import mozjpeg_amd as M
import djpeg_cases as DJ
import scale_all_cases as SA
import tj_decompress_cases as TD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "simt"))

pytestmark = pytest.mark.skipif(not SA.have_tools(), reason="reference cjpeg / jpegtran / djpeg not built (oracle/_ref)")
needs_djpeg = pytest.mark.skipif(not DJ.have_tools(), reason="reference djpeg / libjpeg.so.62 or tests/native/djpeg_client not built")
needs_tj = pytest.mark.skipif(not TD.have_tools(), reason="reference binaries (oracle/_ref) or the TurboJPEG-signature library are not built")


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


@pytest.mark.parametrize("src,mode,k", SA.CASES, ids=[SA.case_id(c) for c in SA.CASES])
def test_every_new_size_matches_djpeg(simt, src, mode, k):
    SA.check_case(M, src, mode, k)


def test_every_transform_size_is_reached(simt):
    SA.check_every_transform_size_is_reached(M)


@pytest.mark.parametrize("src,frac", SA.FRACTION_CASES, ids=[SA.case_id(c) for c in SA.FRACTION_CASES])
def test_fraction_is_resolved_as_djpeg_does(simt, src, frac):
    SA.check_fraction(M, src, frac)


@pytest.mark.parametrize("src,k", SA.LAYOUT_CASES, ids=[SA.case_id(c) for c in SA.LAYOUT_CASES])
def test_layouts_and_colour_kernels(simt, src, k):
    SA.check_layouts(M, src, k)


def test_four_component_files(simt):
    SA.check_four_components(M)


def test_progressive_and_arithmetic_sources(simt):
    SA.check_other_entropy_coders(M)


@pytest.mark.parametrize("src,k", SA.PLANE_CASES, ids=[SA.case_id(c) for c in SA.PLANE_CASES])
def test_raw_planes(simt, src, k):
    SA.check_planes(M, src, k)
    SA.check_device_planes(M, src, k, ctypes.string_at)        # (the emulator's device memory is the process's own)


def test_one_encoder_serves_every_scale(simt):
    SA.check_one_encoder_serves_every_scale(M)


def test_mixed_batch_with_a_damaged_file(simt):
    SA.check_mixed_batch(M)


def test_the_opt_in_is_the_only_door(simt):
    SA.check_opt_in(M)


# ---- the drop-in libraries over the emulator ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def standalone_dir():
    import fuzz_cjpeg
    return os.path.join(fuzz_cjpeg.dropin_dir(), "standalone")


@needs_djpeg
@pytest.mark.parametrize("src,switches", SA.DJPEG_PAIRS, ids=["%s-%s" % p for p in SA.DJPEG_PAIRS])
def test_unchanged_djpeg_with_the_variable(standalone_dir, src, switches):
    SA.check_djpeg(DJ.Runner(standalone_dir, env={"SIMT_STRICT": "1", SA.ENV: "1"}), src, switches)


@needs_djpeg
def test_unchanged_djpeg_refuses_without_the_variable(standalone_dir):
    SA.check_djpeg_refuses_without_the_variable(DJ.Runner(standalone_dir, env={"SIMT_STRICT": "1"}))


@pytest.fixture(scope="module")
def tj_results():
    import fuzz_cjpeg
    dst = os.path.join(fuzz_cjpeg.dropin_dir(), "libmozjpeg_hip_turbojpeg.so")
    if not os.path.exists(dst) or os.path.getmtime(dst) < os.path.getmtime(TD.TJSHIM):
        shutil.copy2(TD.TJSHIM, dst)
    env = dict(os.environ, SIMT_STRICT="1", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + sys.path))
    env.pop("MOZJPEG_HIP_TJ_DECOMPRESS", None)
    env.pop(SA.ENV, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "scale_all_cases.py"), dst], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1200)
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("SCALE_ALL_TJ_RESULTS ")]
    assert r.returncode == 0 and lines, "the child ended with %d: %s" % (r.returncode, r.stderr.decode()[-2000:])
    return json.loads(lines[-1].split(" ", 1)[1])


@needs_tj
@pytest.mark.parametrize("name", list(SA.TJ_CHECKS))
def test_turbojpeg_library(tj_results, name):
    assert tj_results[name] == "ok", tj_results[name]
