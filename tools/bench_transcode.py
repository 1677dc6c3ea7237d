#!/usr/bin/env python3
"""Re-compression throughput on one GPU: JPEG bytes in host memory -> re-coded JPEG bytes in host memory (mjh_transcode_host +
mjh_collect), `-revert -optimize`, against the reference's jpegtran on the same files.

Workload A: 64 distinct seeded 4K 4:2:0 q75 sequential files without restart markers per call.  Workload B: 1024 files of 320x240.
Per workload: files/s with the default subsequence length and with MJH_DECODE_SUBSEQ=0 (one lane per restart segment), alternating
in the same run (--repeats rounds, >= --seconds timed per round after a warm-up), the run-to-run spread, the synchronisation rounds
and host synchronisations per call, the decoder's phase times and the per-kernel times of the schedule behind it
(mjh_set_profiling(1), a separate pass), and the yardstick: oracle/_ref/jpegtran -copy none -revert -optimize over the same files,
16 processes at a time, files on a RAM disk.  The first call's files are compared with the reference's.
--transform NAME [--trim]: the same under a lossless transform (mozjpeg_amd.TRANSFORMS; the reference side runs jpegtran with the same
switch), and next to the decoder's phase times what a plain device-to-device copy and a zeroing of the batch's coefficient planes take
(the yardstick a separate permutation pass would have to be measured against).
--progressive default|simple: the same images as progressive files, written by the reference's cjpeg with its default switches or with
-revert -progressive, decoded with Encoder.set_sources(progressive=True); the refinement levels' time is reported next to the phases.
--copy MODE: both workloads with a 12 KB Exif APP1 and a 3 KB ICC APP2 added to every file, under copy="none" and copy=MODE.
usage: python tools/bench_transcode.py [--copy all] [--progressive default|simple] [--source arith420] [--workloads A,B] [--seconds 2] [--repeats 3] [--subseq 512,0] [--transform rot90 [--trim]]
                                       [--out profiles/transcode_bench]"""
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
import numpy as np  # noqa: E402,F401
import mozjpeg_amd as M  # noqa: E402
import oracle_lib as O  # noqa: E402
import transcode_cases as TC  # noqa: E402
import transform_cases as XC  # noqa: E402

SWITCHES = ["-copy", "none", "-revert", "-optimize"]


def plane_probe(p, n, rounds=5):
    """(bytes, copy ms, zeroing ms) of the coefficient planes of n images with parameters p: int16, per component 64 zig-zag planes of
    the block count rounded up to 64; a plain device-to-device copy and a memset of that size, the best of `rounds`"""
    per_image = 0
    maxh = max(p.h_samp_factor[c] for c in range(p.num_components))
    maxv = max(p.v_samp_factor[c] for c in range(p.num_components))
    for c in range(p.num_components):
        wib = -(-p.image_width * p.h_samp_factor[c] // (maxh * 8))
        hib = -(-p.image_height * p.v_samp_factor[c] // (maxv * 8))
        per_image += ((wib * hib + 63) & ~63) * 64
    a = torch.empty(n * per_image, dtype=torch.int16, device="cuda")
    b = torch.empty_like(a)
    best = [1e9, 1e9]
    for _ in range(rounds + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        b.copy_(a)
        ev[1].record()
        a.zero_()
        ev[2].record()
        torch.cuda.synchronize()
        best = [min(best[0], ev[0].elapsed_time(ev[1])), min(best[1], ev[1].elapsed_time(ev[2]))]
    return a.numel() * 2, best[0], best[1]


# --progressive: the sources as the reference's cjpeg writes them with its default switches (the max-compression profile: progressive
# with scan search and trellis quantization, its own quantization tables) or with -revert -progressive (jpeg_simple_progression)
PROGRESSIVE_ARGS = {None: ["-revert"], "default": [], "simple": ["-revert", "-progressive"]}
# --source arith420: the same images as arithmetic-coded sequential files with a restart interval of one MCU row (cjpeg -revert
# -restart 1 -arithmetic), decoded with Encoder.set_sources(arithmetic=True): jpegtran from arithmetic to optimised Huffman coding
ARITH_ARGS = ["-restart", "1", "-arithmetic"]


def sources(workload, progressive=None, arith=False):
    if workload == "A":
        imgs = [O.synthetic_frame(3840, 2160, seed=1234 + i) for i in range(64)]
    else:
        big = [O.synthetic_frame(3840, 2160, seed=77 + i) for i in range(4)]
        imgs = [big[i % 4][y:y + 240, x:x + 320] for i, (y, x) in enumerate((y, x) for y in range(0, 1920, 120) for x in range(0, 3520, 55))][:1024]
        assert len(imgs) == 1024
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda a: TC.cjpeg(a, PROGRESSIVE_ARGS[progressive] + ["-quality", "75", "-sample", "2x2"] + (ARITH_ARGS if arith else [])), imgs))


def reference_rate(files, procs=16, switches=None):
    """files/s of the reference's jpegtran, `procs` processes at a time, input and output on a RAM disk; also its output files"""
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    with tempfile.TemporaryDirectory(dir=base) as td:
        for i, f in enumerate(files):
            with open(os.path.join(td, "%d.jpg" % i), "wb") as fh:
                fh.write(f)

        def one(i):
            subprocess.check_call([TC.JPEGTRAN] + (switches or SWITCHES) + ["-outfile", os.path.join(td, "o%d.jpg" % i), os.path.join(td, "%d.jpg" % i)])
        with ThreadPoolExecutor(procs) as ex:
            list(ex.map(one, range(min(len(files), 2 * procs))))          # warm-up
            t0 = time.perf_counter()
            list(ex.map(one, range(len(files))))
            dt = time.perf_counter() - t0
        outs = [open(os.path.join(td, "o%d.jpg" % i), "rb").read() for i in range(len(files))]
    return len(files) / dt, outs, base is not None


def timed(enc, files, seconds):
    calls, t0 = 0, time.perf_counter()
    while True:
        enc.submit_transcode(files)
        enc.collect(0, copy=True)
        calls += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return calls * len(files) / dt


def with_markers(jpeg, seed):
    """the file with a 12 KB Exif APP1 and a 3 KB ICC profile (one APP2) behind its JFIF APP0: what a camera file carries"""
    import copy_cases as CC
    exif = CC.seg(0xE1, b"Exif\0\0" + CC.blob(12 * 1024, seed))       # (no TIFF header in it: nothing to adjust, as without a transform)
    return CC.behind_app0(jpeg, exif + CC.icc_segments(CC.blob(3 * 1024, seed + 1)))


def copy_bench(a):
    """--copy MODE: workloads A and B with markers added to every file, re-coded under copy="none" and copy=MODE by two encoders
    of one process, alternating; the reference is jpegtran -copy MODE, 16 processes at a time.  MOZJPEG_AMD_LIB naming a library
    that predates the copy modes: only copy="none" is measured (the parent's figure for the same files)."""
    result = {"copy": a.copy, "library": M.LIB_PATH, "workloads": {}}
    old = not hasattr(M.lib(), "mjh_encoder_set_copy_markers")
    modes = ["none"] if old or a.copy == "none" else ["none", a.copy]      # (--copy none: the one encoder of a run on an older library, for a like-for-like pair)
    for wl in a.workloads.split(","):
        files = [with_markers(f, 500 + i) for i, f in enumerate(sources(wl))]
        r = {"files": len(files), "source_bytes": sum(len(f) for f in files), "configs": {}}
        encs = {}
        for m in modes:
            ref_rate, ref_outs, _ = reference_rate(files, switches=["-copy", m, "-revert", "-optimize"])
            enc = encs[m] = M.Encoder(M.params_from_jpeg(files[0], revert=True, optimize=True), max_batch=len(files))
            if m != "none":
                enc.set_copy(m)
            outs = enc.transcode_host(files)
            r["configs"][m] = {"reference_files_per_s": ref_rate, "identical_to_reference": outs == ref_outs, "files_per_s": [],
                               "output_bytes": sum(len(o) for o in outs)}
            enc.submit_transcode(files)
            enc.collect(0)                      # warm-up
        for _ in range(a.repeats):             # alternating
            for m, enc in encs.items():
                r["configs"][m]["files_per_s"].append(timed(enc, files, a.seconds))
        for m, enc in encs.items():
            c = r["configs"][m]
            v = c["files_per_s"]
            c["median_files_per_s"] = sorted(v)[len(v) // 2]
            c["spread"] = (max(v) - min(v)) / c["median_files_per_s"]
            enc.close()
        result["workloads"][wl] = r
        print(json.dumps({wl: r}), flush=True)
    if a.out:
        with open(a.out + ".json", "w") as f:
            json.dump(result, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copy", default=None, choices=["none", "comments", "all", "icc"],
                    help="markers added to every file; copy=none against this mode (see copy_bench)")
    ap.add_argument("--workloads", default="A,B")
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--subseq", default="512,0")
    ap.add_argument("--transform", default=None, choices=sorted(M.TRANSFORMS))
    ap.add_argument("--trim", action="store_true")
    ap.add_argument("--progressive", default=None, choices=["default", "simple"])
    ap.add_argument("--source", default=None, choices=["arith420"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    arith = a.source == "arith420"
    if a.copy:
        return copy_bench(a)
    prog = a.progressive is not None
    xf = dict(transform=a.transform, trim=a.trim) if a.transform else {}
    switches = SWITCHES[:2] + XC.jpegtran_args(**xf) + SWITCHES[2:]
    result = {"switches": switches, "progressive_sources": a.progressive, "arithmetic_sources": arith, "workloads": {}}
    for wl in a.workloads.split(","):
        files = sources(wl, a.progressive, arith)
        ref_rate, ref_outs, ramdisk = reference_rate(files, switches=switches)
        r = {"files": len(files), "source_bytes": sum(len(f) for f in files), "reference_files_per_s": ref_rate, "reference_on_ramdisk": ramdisk, "configs": {}}
        encs = {}
        for s in a.subseq.split(","):
            os.environ["MJH_DECODE_SUBSEQ"] = s
            encs[s] = M.Encoder(M.params_from_jpeg(files[0], revert=True, optimize=True, progressive_sources=prog, arithmetic_sources=arith, **xf), max_batch=len(files))
            encs[s].set_sources(progressive=prog, arithmetic=arith)
        os.environ.pop("MJH_DECODE_SUBSEQ", None)
        for s, enc in encs.items():
            outs = enc.transcode_host(files)
            r["configs"][s] = {"identical_to_reference": outs == ref_outs, "stats": enc.transcode_stats(), "files_per_s": []}
            enc.submit_transcode(files)
            enc.collect(0)                      # warm-up
        for _ in range(a.repeats):             # alternating
            for s, enc in encs.items():
                r["configs"][s]["files_per_s"].append(timed(enc, files, a.seconds))
        for s, enc in encs.items():
            c = r["configs"][s]
            v = c["files_per_s"]
            c["median_files_per_s"] = sorted(v)[len(v) // 2]
            c["spread"] = (max(v) - min(v)) / c["median_files_per_s"]
            c["ratio_to_reference"] = c["median_files_per_s"] / ref_rate
            enc.set_profiling(1)
            for _ in range(3):
                enc.submit_transcode(files)
                enc.collect(0)
            c["decoder_ms"] = enc.transcode_stats()["ms"]
            if arith:
                c["arith"] = enc.arith_stats()               # chains, launches, and the milliseconds of K-DA
            if prog:
                c["refinement"] = enc.prog_stats()          # levels of scans, and the milliseconds of the levels above 0
            c["kernel_ms"] = enc.kernel_times()
            enc.set_profiling(0)
            enc.close()
        if xf:
            r["plane_bytes"], r["plane_copy_ms"], r["plane_zero_ms"] = plane_probe(M.params_from_jpeg(files[0], revert=True, optimize=True, **xf), len(files))
        result["workloads"][wl] = r
        print(json.dumps({wl: r}), flush=True)
    if a.out:
        with open(a.out + ".json", "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
