#!/usr/bin/env python3
"""Decode throughput on one GPU: JPEG bytes in host memory -> interleaved RGB pixels (mjh_decode_host), against the reference's djpeg on
the same files.

Workload A: 64 distinct seeded 4K 4:2:0 q75 sequential files without restart markers per call.  Workload B: 1024 files of 320x240.
Per workload, on one host thread: files/s and Mpixels/s to pixels in device memory (mjh_decode_host + mjh_encoder_sync) and to pixels
in pinned host memory (+ mjh_get_pixels of every image), alternating in the same run (--repeats rounds, >= --seconds timed per round
after a warm-up) with the run-to-run spread; the phase times of the Huffman decoder and of the two pixel kernels
(mjh_set_profiling(1), a separate pass) with the bytes per second the pixel kernels reach against their byte counts; and the
yardstick: oracle/_ref/djpeg -pnm over the same files, 16 processes at a time, input on a RAM disk and output discarded (that
figure includes process start and PPM formatting).  The first call's pixels are compared with djpeg's before anything is timed.
--scale M/N: both workloads decoded at that scale (1/2, 1/4, 1/8: the reduced inverse DCTs), the reference being djpeg -scale M/N.
usage: python tools/bench_decode.py [--workloads A,B] [--scale 1/1] [--seconds 2] [--repeats 3] [--out profiles/decode_bench]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402,F401  (torch's runtime first: tests/conftest.py)
import numpy as np  # noqa: E402
import mozjpeg_amd as M  # noqa: E402
import decode_cases as DC  # noqa: E402
from bench_transcode import sources  # noqa: E402


def reference_rate(files, args=(), procs=16):
    """files/s of the reference's djpeg, `procs` processes at a time, input on a RAM disk, output discarded"""
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    with tempfile.TemporaryDirectory(dir=base) as td:
        for i, f in enumerate(files):
            with open(os.path.join(td, "%d.jpg" % i), "wb") as fh:
                fh.write(f)

        def one(i):
            subprocess.check_call([DC.DJPEG, "-pnm"] + list(args) + ["-outfile", os.devnull, os.path.join(td, "%d.jpg" % i)])
        with ThreadPoolExecutor(procs) as ex:
            list(ex.map(one, range(min(len(files), 2 * procs))))          # warm-up
            t0 = time.perf_counter()
            list(ex.map(one, range(len(files))))
            dt = time.perf_counter() - t0
    return len(files) / dt, base is not None


def timed(enc, files, seconds, host, opts):
    calls, t0 = 0, time.perf_counter()
    while True:
        enc.submit_decode(files, opts=opts)
        if host is None:
            enc.sync()
        else:
            for i in range(len(files)):
                enc.get_pixels(i, out=host[i])
        calls += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return calls * len(files) / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="A,B")
    ap.add_argument("--scale", default="1/1")
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    opts = M.decode_opts(scale=a.scale)
    k = M.scale_idct_size(opts.scale_num, opts.scale_denom)
    dj_args = ["-scale", a.scale] if k != 8 else []
    isa = json.load(open(os.path.join(ROOT, "mozjpeg_amd", "kernel_isa.json")))["kernels"]
    result = {"kernel_sha": {k: isa[k]["sha"] for k in isa if k in ("k_dec_sync", "k_dec_prefix", "k_dec_store", "k_dec_dc", "k_idct", "k_upcolor") or k.startswith("k_idct_scaled")},
              "scale": a.scale, "idct_size": k, "workloads": {}}
    for wl in a.workloads.split(","):
        files = sources(wl)
        n = len(files)
        info = M.jpeg_info(files[0])
        w, h = info.image_width, info.image_height
        enc = M.Encoder(M.params_from_jpeg(files[0], revert=True), max_batch=n)
        outs = enc.decode_host(files, opts=opts)
        ow, oh = -(-w * k // 8), -(-h * k // 8)
        assert outs[0].shape == (oh, ow, 3)
        with ThreadPoolExecutor(16) as ex:
            same = list(ex.map(lambda i: bool(np.array_equal(outs[i], DC.djpeg(files[i], dj_args))), range(n)))
        del outs
        ref_rate, ramdisk = reference_rate(files, dj_args)
        r = {"files": n, "width": w, "height": h, "out_width": ow, "out_height": oh, "source_bytes": sum(len(f) for f in files), "identical_to_reference": all(same),
             "reference_files_per_s": ref_rate, "reference_on_ramdisk": ramdisk, "stats": {k: v for k, v in enc.transcode_stats().items() if k != "ms"}, "paths": {}}
        host = M.pinned_empty((n, oh, ow, 3))
        paths = {"device": None, "host": host}
        for name, dst in paths.items():
            timed(enc, files, 0.0, dst, opts)          # warm-up
            r["paths"][name] = {"files_per_s": []}
        for _ in range(a.repeats):                     # alternating
            for name, dst in paths.items():
                r["paths"][name]["files_per_s"].append(timed(enc, files, a.seconds, dst, opts))
        for name in paths:
            c = r["paths"][name]
            v = c["files_per_s"]
            c["median_files_per_s"] = sorted(v)[len(v) // 2]
            c["median_mpixels_per_s"] = c["median_files_per_s"] * w * h / 1e6
            c["spread"] = (max(v) - min(v)) / c["median_files_per_s"]
            c["ratio_to_reference"] = c["median_files_per_s"] / ref_rate
        enc.set_profiling(1)
        ms = []
        for _ in range(5):
            enc.submit_decode(files, opts=opts)
            enc.sync()
            ms.append(dict(enc.transcode_stats()["ms"], **enc.decode_stats()["ms"]))
        enc.set_profiling(0)
        r["phase_ms"] = {k: sorted(m[k] for m in ms)[len(ms) // 2] for k in ms[0]}
        # byte counts of the pixel kernels: coefficients read + planes written; planes read + pixels written (4:2:0: 1.5 samples a pixel)
        # (full size only: a reduced transform reads a subset of the coefficient planes that depends on every component's size)
        if k == 8:
            coef_bytes, plane_bytes, pix_bytes = n * w * h * 1.5 * 2, n * w * h * 1.5, n * w * h * 3
            r["idct_gbytes_per_s"] = (coef_bytes + plane_bytes) / r["phase_ms"]["idct"] / 1e6
            r["upcolor_gbytes_per_s"] = (plane_bytes + pix_bytes) / r["phase_ms"]["upcolor"] / 1e6
        kd = sum(r["phase_ms"][k] for k in ("sync", "prefix", "store", "dc"))
        r["pixel_kernels_to_huffman_decoder"] = (r["phase_ms"]["idct"] + r["phase_ms"]["upcolor"]) / kd
        enc.close()
        del host
        result["workloads"][wl] = r
        print(json.dumps({wl: r}), flush=True)
    if a.out:
        with open(a.out + ".json", "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
