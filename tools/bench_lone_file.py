#!/usr/bin/env python3
"""One 4K file at a time: is the GPU path faster than the reference on one CPU core when there is no batch to fill the chip with?

The first image of workload A (tools/bench_transcode.py) as a sequential file and as the two kinds of progressive file; per file the
median wall time of one call with max_batch = 1 -- to coefficients in device memory, to RGB pixels in device memory, to a re-coded
file in host memory (-revert -optimize) -- next to the median wall time of one process of the reference's djpeg -pnm and
jpegtran -copy none -revert -optimize on the same file (RAM disk; process start included, as in the other profile files).
usage: python tools/bench_lone_file.py [--calls 15] [--out profiles/lone_file_bench]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402,F401  (torch's runtime first: tests/conftest.py)
import mozjpeg_amd as M  # noqa: E402
import oracle_lib as O  # noqa: E402
import transcode_cases as TC  # noqa: E402
import decode_cases as DC  # noqa: E402
from bench_transcode import PROGRESSIVE_ARGS  # noqa: E402


def median(v):
    return sorted(v)[len(v) // 2]


def wall_ms(fn, calls):
    fn()
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.init()
    img = O.synthetic_frame(3840, 2160, seed=1234)
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    result = {}
    for kind in (None, "simple", "default"):
        src = TC.cjpeg(img, PROGRESSIVE_ARGS[kind] + ["-quality", "75", "-sample", "2x2"])
        prog = kind is not None
        enc = M.Encoder(M.params_from_jpeg(src, revert=True, optimize=True, progressive_sources=prog), max_batch=1)
        enc.set_sources(progressive=prog)

        def coefs():
            enc.submit_decode([src], coefficients=True)
            enc.sync()

        def pixels():
            enc.submit_decode([src])
            enc.sync()

        r = {"source_bytes": len(src), "gpu_ms": {"coefficients_device": wall_ms(coefs, a.calls), "pixels_device": wall_ms(pixels, a.calls),
                                                    "recoded_host": wall_ms(lambda: enc.transcode_host([src]), a.calls)}}
        if prog:
            r["levels"] = enc.prog_stats()["levels"]
        enc.close()
        with tempfile.TemporaryDirectory(dir=base) as td:
            inp = os.path.join(td, "in.jpg")
            with open(inp, "wb") as f:
                f.write(src)
            r["reference_ms"] = {
                "djpeg": wall_ms(lambda: subprocess.check_call([DC.DJPEG, "-pnm", "-outfile", os.path.join(td, "o.ppm"), inp]), max(3, a.calls // 3)),
                "jpegtran": wall_ms(lambda: subprocess.check_call([TC.JPEGTRAN, "-copy", "none", "-revert", "-optimize", "-outfile", os.path.join(td, "o.jpg"), inp]),
                                    max(3, a.calls // 3))}
        result[kind or "sequential"] = r
        print(json.dumps({kind or "sequential": r}), flush=True)
    if a.out:
        with open(a.out + ".json", "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
