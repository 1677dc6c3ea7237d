#!/usr/bin/env python3
"""Lossless decode throughput on one GPU: lossless JPEG bytes (SOF3) in host memory -> samples in device memory (mjh_decode_host on an
encoder made from the file's own parameters, Encoder.set_sources(lossless=True)), against the reference's djpeg on the same files.

Workloads, each --files distinct seeded 3840 x 2160 files per call, made by the reference's cjpeg -revert -lossless psv,0:
  rgb8_psv1   8-bit RGB, predictor 1 (undifferencing = independent row prefix sums)
  rgb8_psv7   8-bit RGB, predictor 7 (undifferencing = the row wavefront of k_ll_wave)
  gray16_psv1 16-bit gray, predictor 1
Per workload, on one host thread: files/s and Msamples/s to samples in device memory (mjh_decode_host + mjh_encoder_sync), --repeats
rounds of >= --seconds each after a warm-up, with the run-to-run spread; the phase times of the kernels (mjh_set_profiling(1), a
separate pass: sync = first pass + synchronisation rounds, prefix, store, undiff = k_ll_col0 + k_ll_rows + k_ll_wave, pixels =
k_ll_pixels); and the yardstick: oracle/_ref/djpeg -pnm over the same files, 16 processes at a time, input on a RAM disk and output
discarded (that figure includes process start and PNM formatting).  The first call's samples are compared with djpeg's and with the
source images before anything is timed.
usage: python tools/bench_lossless_decode.py [--workloads rgb8_psv1,rgb8_psv7,gray16_psv1] [--files 8] [--seconds 2] [--repeats 3] [--out profiles/lossless_decode_bench]"""
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
import torch  # noqa: E402,F401  (torch's runtime first: tests/conftest.py)
import numpy as np  # noqa: E402
import mozjpeg_amd as M  # noqa: E402
import lossless_cases as LC  # noqa: E402
import lossless_decode_cases as LD  # noqa: E402
import oracle_lib as O  # noqa: E402

WORKLOADS = {"rgb8_psv1": (3, 8, 1), "rgb8_psv7": (3, 8, 7), "gray16_psv1": (1, 16, 1)}      # components, precision, predictor
W, H = 3840, 2160
KERNELS = ("k_ldec_sync", "k_dec_prefix", "k_ldec_store", "k_ll_col0", "k_ll_rows", "k_ll_wave")


def images(comps, precision, n):
    def one(i):
        a = O.synthetic_frame(W, H, seed=4321 + i)
        if comps == 1:                                  # the green plane as the high byte, the red one as the low byte: 16 significant bits
            a = ((a[:, :, 1].astype(np.uint16) << 8) | a[:, :, 0])[:, :, None]
        return np.ascontiguousarray(a)
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(one, range(n)))


def reference_rate(files, procs=16):
    """files/s of the reference's djpeg, `procs` processes at a time (every file often enough to keep them busy), input on a RAM disk"""
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    jobs = list(range(len(files))) * max(1, -(-2 * procs // len(files)))
    with tempfile.TemporaryDirectory(dir=base) as td:
        for i, f in enumerate(files):
            with open(os.path.join(td, "%d.jpg" % i), "wb") as fh:
                fh.write(f)

        def one(i):
            subprocess.check_call([LD.DJPEG, "-pnm", "-outfile", os.devnull, os.path.join(td, "%d.jpg" % i)])
        with ThreadPoolExecutor(procs) as ex:
            list(ex.map(one, jobs[:procs]))             # warm-up
            t0 = time.perf_counter()
            list(ex.map(one, jobs))
            dt = time.perf_counter() - t0
    return len(jobs) / dt, base is not None


def timed(enc, files, seconds):
    calls, t0 = 0, time.perf_counter()
    while True:
        enc.submit_decode(files)
        enc.sync()
        calls += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return calls * len(files) / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    isa = json.load(open(os.path.join(ROOT, "mozjpeg_amd", "kernel_isa.json")))
    result = {"source_stamp": isa.get("source_stamp"),
              "kernel_sha": {k: isa["kernels"][k]["sha"] for k in isa["kernels"] if k in KERNELS or k.startswith("k_ll_pixels")},
              "vgpr": {k: isa["kernels"][k]["vgpr"] for k in isa["kernels"] if k in KERNELS or k.startswith("k_ll_pixels")},
              "width": W, "height": H, "workloads": {}}
    for wl in a.workloads.split(","):
        comps, precision, psv = WORKLOADS[wl]
        n = a.files
        imgs = images(comps, precision, n)
        with ThreadPoolExecutor(16) as ex:
            files = list(ex.map(lambda im: LC.reference(im, psv, 0, precision), imgs))
        assert all(isinstance(f, bytes) for f in files) and len(set(files)) == n
        enc = M.Encoder(M.params_from_jpeg(files[0], revert=True, lossless_sources=True), max_batch=n)
        enc.set_sources(progressive=False, lossless=True)
        outs = enc.decode_host(files)
        with ThreadPoolExecutor(16) as ex:
            same = list(ex.map(lambda i: bool(LD.same(outs[i], LD.djpeg(files[i])) and np.array_equal(outs[i], imgs[i][:, :, 0] if comps == 1 else imgs[i])), range(n)))
        del outs
        ref_rate, ramdisk = reference_rate(files)
        samples = W * H * comps
        r = {"files": n, "components": comps, "precision": precision, "predictor": psv, "source_bytes": sum(len(f) for f in files),
             "bits_per_sample": 8.0 * sum(len(f) for f in files) / (n * samples), "identical_to_reference_and_to_the_images": all(same),
             "reference_files_per_s": ref_rate, "reference_on_ramdisk": ramdisk, "stats": {k: v for k, v in enc.transcode_stats().items() if k != "ms"}}
        timed(enc, files, 0.0)                          # warm-up
        v = [timed(enc, files, a.seconds) for _ in range(a.repeats)]
        r["files_per_s"] = v
        r["median_files_per_s"] = sorted(v)[len(v) // 2]
        r["median_msamples_per_s"] = r["median_files_per_s"] * samples / 1e6
        r["median_mpixels_per_s"] = r["median_files_per_s"] * W * H / 1e6
        r["spread"] = (max(v) - min(v)) / r["median_files_per_s"]
        r["ratio_to_reference"] = r["median_files_per_s"] / ref_rate
        enc.set_profiling(1)
        ms = []
        for _ in range(5):
            enc.submit_decode(files)
            enc.sync()
            t, d = enc.transcode_stats()["ms"], enc.decode_stats()["ms"]
            ms.append({"sync": t["sync"], "prefix": t["prefix"], "store": t["store"], "undiff": d["idct"], "pixels": d["upcolor"]})
        enc.set_profiling(0)
        r["phase_ms"] = {k: sorted(m[k] for m in ms)[len(ms) // 2] for k in ms[0]}
        # byte counts: undifferencing reads and writes every 16-bit plane once; the pixel kernel reads them and writes the samples
        sb = 2 if precision > 8 else 1
        r["undiff_gbytes_per_s"] = n * samples * 4 / r["phase_ms"]["undiff"] / 1e6
        r["pixels_gbytes_per_s"] = n * samples * (2 + sb) / r["phase_ms"]["pixels"] / 1e6
        enc.close()
        result["workloads"][wl] = r
        print(json.dumps({wl: r}), flush=True)
    if a.out:
        with open(a.out + ".json", "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
