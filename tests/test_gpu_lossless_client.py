"""GPU suite: a libjpeg client in lossless mode (tests/native/lossless_client.c) -- the compress object from image to image: lossy ->
lossless -> lossy on one object, abbreviated datastreams, jpeg_abort_compress in the middle of a lossless image,
jpeg16_write_scanlines / jpeg12_write_scanlines with the rows handed over in pieces, scan_info set by the client, markers between
jpeg_start_compress and the first row, the refusals, and the fields the client reads back after jpeg_start_compress.  Every printed
line (file sizes and hashes, the object's fields, error codes and messages) equals the same binary on the reference's libjpeg."""
import os
import subprocess

import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIENT = os.path.join(ROOT, "tests", "native", "lossless_client")
SHIM = os.path.join(ROOT, "mozjpeg_amd", "libmozjpeg_hip_jpeg62.so")
STANDALONE_DIR = os.path.join(ROOT, "mozjpeg_amd", "standalone")
SCENARIOS = ["lossy_lossless_lossy", "fields", "sixteen", "sixteen_lossy", "script", "bad_script", "abbreviated", "abort", "markers",
             "raw_data", "restart_blocks"]

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not (os.path.exists(CLIENT) and os.path.exists(SHIM)), reason="tests/native/lossless_client or the drop-in libraries are not built")]


def run_client(scenario, mode, shim=SHIM, standalone_dir=STANDALONE_DIR, env_extra=None):
    env = dict(os.environ)
    O.set_preload(env, shim if mode == "preload" else None)
    env["LD_LIBRARY_PATH"] = standalone_dir if mode == "standalone" else O.REF_DIR
    env.update(env_extra or {})
    return subprocess.run([CLIENT, scenario], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)


def check(scenario, mode, **kw):
    want = run_client(scenario, "reference", **kw)
    assert want.returncode == 0 and want.stdout.count(b"\n") > 1, want.stderr.decode()
    got = run_client(scenario, mode, **kw)
    assert got.returncode == 0, got.stderr.decode()[-2000:]
    w, g = want.stdout.decode().splitlines(), got.stdout.decode().splitlines()
    assert g == w, [(a, b) for a, b in zip(g, w) if a != b][:4] + [got.stderr.decode()[-500:]]


@pytest.mark.parametrize("mode", ["preload", "standalone"])
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_lossless_client_scenarios(scenario, mode):
    check(scenario, mode)
