#!/usr/bin/env python3
"""Decompress drop-in throughput: what an UNCHANGED libjpeg client gets from jpeg_read_scanlines (never bench.py's `value`).
tests/native/djpeg_bench (public libjpeg API, T threads with a decompress object each, jpeg_mem_src over distinct files) against
  - the reference's libjpeg.so.62 (CPU, oracle/_ref)               -> "reference"
  - mozjpeg_amd/standalone/libjpeg.so.62 instead of it              -> "standalone"
Workload: distinct seeded 4K 4:2:0 q75 sequential files; rows asked for one at a time (what djpeg does) and all at once.  The
stand-alone runs are repeated with MOZJPEG_HIP_TIMING=1 for the split of one call: reading the source, marker walk + encoder lease,
mjh_decode_host + wait, copy-out to host memory, row copies.
usage: python tools/bench_djpeg_dropin.py [--threads 1,16] [--files 16] [--seconds 3] [--out profiles/djpeg_dropin_bench]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.path.join(ROOT, "oracle", "_ref")
STANDALONE = os.path.join(ROOT, "mozjpeg_amd", "standalone")
BENCH = os.path.join(ROOT, "tests", "native", "djpeg_bench")
import oracle_lib as O  # noqa: E402
import transcode_cases as TC  # noqa: E402


def run(mode, threads, per_thread, rows, paths, timing=False, timeout=900):
    env = dict(os.environ)
    O.set_preload(env)
    env["LD_LIBRARY_PATH"] = STANDALONE if mode == "standalone" else REF
    if timing:
        env["MOZJPEG_HIP_TIMING"] = "1"
    try:
        r = subprocess.run([BENCH, str(threads), str(per_thread), str(rows)] + paths, env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        return {"mode": mode, "threads": threads, "rows_per_call": rows, "error": "timeout"}
    if r.returncode != 0:
        return {"mode": mode, "threads": threads, "rows_per_call": rows, "error": r.stderr[-400:]}
    d = json.loads(r.stdout.strip().splitlines()[-1])
    d["mode"] = mode
    if timing:
        m = re.search(r"decompress timing: (\d+) images; per image: source ([\d.]+) ms, probe\+lease ([\d.]+) ms, decode\+wait ([\d.]+) ms, copy-out ([\d.]+) ms, rows ([\d.]+) ms", r.stderr)
        if m:
            d["split_ms_per_file"] = dict(zip(("source", "probe_lease", "decode_wait", "copy_out", "rows"), (float(x) for x in m.groups()[1:])))
    return d


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", default="1,16")
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=3.0, help="target duration of one measured point")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    with ThreadPoolExecutor(16) as ex:
        files = list(ex.map(lambda i: TC.cjpeg(O.synthetic_frame(3840, 2160, seed=1234 + i), ["-revert", "-quality", "75", "-sample", "2x2"]), range(a.files)))
    res = {"what": "unchanged libjpeg decompress clients on this box: JPEG files in host memory, pixels in ordinary host memory",
           "files": a.files, "size": "3840x2160", "source_bytes_per_file": sum(len(f) for f in files) // len(files), "points": []}
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    with tempfile.TemporaryDirectory(dir=base) as td:
        paths = []
        for i, f in enumerate(files):
            paths.append(os.path.join(td, "%d.jpg" % i))
            with open(paths[-1], "wb") as fh:
                fh.write(f)
        hashes = set()
        for t in [int(x) for x in a.threads.split(",")]:
            for rows in (1, 0):
                for mode in ("reference", "standalone"):
                    probe = run(mode, t, 2, rows, paths)                      # a short run sizes the measured one
                    if "error" in probe:
                        res["points"].append(probe)
                        continue
                    per_thread = max(4, int(a.seconds * probe["files_per_s"] / t))
                    d = run(mode, t, per_thread, rows, paths)
                    hashes.add(d.get("fnv1a_first"))
                    if mode == "standalone" and "error" not in d:
                        d["timed_run"] = run(mode, t, per_thread, rows, paths, timing=True)
                    res["points"].append(d)
                    print(json.dumps(d), file=sys.stderr, flush=True)
        res["pixels_identical"] = len(hashes) == 1
    text = json.dumps(res, indent=1)
    if a.out:
        with open(a.out + ".json", "w") as f:
            f.write(text + "\n")
    print(text)
