"""CPU suite: TurboJPEG decompress instances of the SHIPPED mozjpeg_amd/libmozjpeg_hip_turbojpeg.so (tj_shim.c) while its
libmozjpeg_hip.so is the kernel sources on the wave64 emulator (tools/simt, SIMT_STRICT), against the reference's
oracle/_ref/libturbojpeg.so.0 call by call and byte by byte (tests/tj_decompress_cases.py).  All checks run in one child process,
because a process holds only one library named libmozjpeg_hip.so and this one may hold the device library already; each test
below reads one check's outcome."""
import json
import os
import shutil
import subprocess
import sys

import pytest

import tj_decompress_cases as TD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "simt"))

pytestmark = pytest.mark.skipif(not TD.have_tools(), reason="reference binaries (oracle/_ref) or the TurboJPEG-signature library are not built")


@pytest.fixture(scope="module")
def shim_over_emulator():
    import fuzz_cjpeg
    d = fuzz_cjpeg.dropin_dir()
    dst = os.path.join(d, "libmozjpeg_hip_turbojpeg.so")
    if not os.path.exists(dst) or os.path.getmtime(dst) < os.path.getmtime(TD.TJSHIM):
        shutil.copy2(TD.TJSHIM, dst)
    return dst


@pytest.fixture(scope="module")
def results(shim_over_emulator):
    env = dict(os.environ, SIMT_STRICT="1", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + sys.path))
    env.pop("MOZJPEG_HIP_TJ_DECOMPRESS", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tj_decompress_cases.py"), shim_over_emulator], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1200)
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("TJ_DECOMPRESS_RESULTS ")]
    assert r.returncode == 0 and lines, "the child ended with %d: %s" % (r.returncode, r.stderr.decode()[-2000:])
    return json.loads(lines[-1].split(" ", 1)[1])


@pytest.mark.parametrize("name", list(TD.CHECKS))
def test_tj_decompress(results, name):
    assert results[name] == "ok", results[name]


def test_forwarding_switch(shim_over_emulator):
    TD.check_forwarding_switch(shim_over_emulator)
