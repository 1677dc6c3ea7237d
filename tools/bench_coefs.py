#!/usr/bin/env python3
"""Reading DCT coefficients on one GPU: JPEG bytes in host memory -> block-major natural-order coefficient arrays
(mjh_decode_opts.raw_coefs), next to the pixel path on the same files in the same run.

Workload: 64 distinct seeded 4K 4:2:0 q75 sequential files per call (workload A of tools/bench_transcode.py).
Rates, on one host thread, alternating in the same run (--repeats rounds, >= --seconds timed per round after a warm-up) with the
run-to-run spread: files/s to coefficients in device memory (submit + mjh_encoder_sync), to coefficients in pinned host memory
(+ mjh_get_coefs of every component of every image), and to RGB pixels in device memory (the pixel path's rate, the yardstick).
Export kernel: the milliseconds of k_export_coefs (device events under mjh_set_profiling(1)) next to a plain device-to-device copy of
the same bytes (torch, device events), alternating, median of --rounds calls; the ratio to that copy is the figure the kernel is
judged by (profiles/coef_bench.md has it for the variant that lost as well).  The first call's arrays are compared with the
reference's jpeg_read_coefficients (tests/native/coef_dump on oracle/_ref) before anything is timed.
--jpegtran: instead of the above, files/s of the reference's unchanged jpegtran -copy none -optimize over the same files with the
stand-alone libjpeg.so.62 on its library path (every process decodes and codes on the GPU) against the reference's library, 16
processes at a time for each, input and output on a RAM disk; this process opens no GPU in that mode, so never more than 16 do.
--against LIB: instead of the above, the paths that existed before -- files/s to RGB pixels in device memory (mjh_decode_host) and
files/s of re-compression to host memory (mjh_transcode_host, -revert -optimize) -- on this tree's library and on LIB, a
libmozjpeg_hip.so built from the parent commit (python -m mozjpeg_amd.build in a checkout of it): one child process per library and
round (MOZJPEG_AMD_LIB), alternating, the same files; the two must agree within the run-to-run spread.
--progressive default|simple [--workload A|B]: the first mode on the same images as progressive files (the reference's cjpeg with its
default switches, or with -revert -progressive), decoded with Encoder.set_sources(progressive=True); the phase times then hold
"refinement", the milliseconds of the refinement levels.
usage: python tools/bench_coefs.py [--jpegtran | --against LIB | --progressive default|simple [--workload B]] [--seconds 2] [--repeats 3] [--rounds 11] [--out profiles/coef_bench]"""
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
import oracle_lib as O  # noqa: E402
import transcode_cases as TC  # noqa: E402
import coef_cases as CC  # noqa: E402
from bench_transcode import sources  # noqa: E402

KERNELS = ("k_dec_sync", "k_dec_prefix", "k_dec_store", "k_dec_dc", "k_export_coefs", "k_idct", "k_upcolor")
STANDALONE_DIR = os.path.join(ROOT, "mozjpeg_amd", "standalone")


def median(v):
    return sorted(v)[len(v) // 2]


def summary(v):
    return {"files_per_s": v, "median_files_per_s": median(v), "spread": (max(v) - min(v)) / median(v)}


def timed(enc, files, seconds, what, host):
    calls, t0 = 0, time.perf_counter()
    while True:
        enc.submit_decode(files, coefficients=what != "pixels")
        if host is None:
            enc.sync()
        else:
            for i in range(len(files)):
                for c, a in enumerate(host):
                    M._chk(M.lib().mjh_get_coefs(enc._h, i, c, a[i].ctypes.data, a.shape[2]))
        calls += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return calls * len(files) / dt


def bench_gpu(a, isa):
    torch.cuda.init()                                  # torch's runtime before the library's (tests/conftest.py has the reason)
    prog = a.progressive is not None
    files = sources(a.workload, a.progressive)
    n = len(files)
    info = M.jpeg_info(files[0], prog)
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True, progressive_sources=prog), max_batch=n)
    enc.set_sources(progressive=prog)
    # ---- the arrays are the reference's (8 of the files through coef_dump)
    outs = enc.decode_host(files, coefficients=True)
    with ThreadPoolExecutor(8) as ex:
        same = all(ex.map(lambda i: CC.same_arrays(outs[i], CC.parse_dump(CC.dump_files(O.REF_DIR, "dump", [files[i]])[2])), range(0, n, 8)))
    del outs
    res = {"progressive_sources": a.progressive, "files": n, "width": info.image_width, "height": info.image_height, "source_bytes": sum(len(f) for f in files),
           "identical_to_reference": same, "kernel_sha": {k: isa[k]["sha"] for k in KERNELS}, "vgpr": {"k_export_coefs": isa["k_export_coefs"]["vgpr"]}}
    # ---- rates
    geo = [enc.coefficients_device(c) for c in range(info.num_components)]
    host = [M.pinned_empty((n, g[3], g[4], 64), np.int16) for g in geo]
    paths = {"coefficients_device": ("coefs", None), "coefficients_host": ("coefs", host), "pixels_device": ("pixels", None)}
    rates = {k: [] for k in paths}
    for name, (what, dst) in paths.items():
        timed(enc, files, 0.0, what, dst)              # warm-up
    for _ in range(a.repeats):                         # alternating
        for name, (what, dst) in paths.items():
            rates[name].append(timed(enc, files, a.seconds, what, dst))
    res["rates"] = {k: summary(v) for k, v in rates.items()}
    res["coefficients_over_pixels"] = res["rates"]["coefficients_device"]["median_files_per_s"] / res["rates"]["pixels_device"]["median_files_per_s"]
    del host
    # ---- the export kernel and a device-to-device copy of the same bytes
    nbytes = sum(n * g[1] for g in geo)                # image stride * files, every component
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty_like(src)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = {"export": [], "copy": []}
    phases = []
    enc.set_profiling(1)
    for r in range(a.rounds + 2):
        enc.submit_decode(files, coefficients=True)
        enc.sync()
        ev[0].record()
        dst.copy_(src)
        ev[1].record()
        torch.cuda.synchronize()
        if r >= 2:                                      # (two warm-up rounds)
            phases.append(dict(enc.transcode_stats()["ms"], **({"refinement": enc.prog_stats()["ms"]} if prog else {})))
            ms["export"].append(phases[-1]["export"])
            ms["copy"].append(ev[0].elapsed_time(ev[1]))
    if prog:
        res["levels"] = enc.prog_stats()["levels"]
    enc.close()
    res["export"] = {"bytes": nbytes, "rounds": a.rounds, "ms_all": ms}
    for k in ms:
        res["export"][k + "_ms"] = median(ms[k])
        res["export"][k + "_gbytes_per_s"] = 2 * nbytes / median(ms[k]) / 1e6          # read + written
    res["export"]["export_over_copy"] = res["export"]["export_ms"] / res["export"]["copy_ms"]
    res["decoder_phase_ms"] = {k: median([p[k] for p in phases]) for k in phases[0]}
    return res


def jpegtran_rate(files, libdir, procs=16):
    """files/s of oracle/_ref/jpegtran -copy none -optimize with LD_LIBRARY_PATH at libdir, `procs` processes at a time; its files"""
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    env = dict(os.environ)
    O.set_preload(env)
    env["LD_LIBRARY_PATH"] = libdir
    with tempfile.TemporaryDirectory(dir=base) as td:
        for i, f in enumerate(files):
            with open(os.path.join(td, "%d.jpg" % i), "wb") as fh:
                fh.write(f)

        def one(i):
            subprocess.check_call([TC.JPEGTRAN, "-copy", "none", "-optimize", "-outfile", os.path.join(td, "o%d.jpg" % i), os.path.join(td, "%d.jpg" % i)], env=env)
        with ThreadPoolExecutor(procs) as ex:
            list(ex.map(one, range(min(len(files), 2 * procs))))          # warm-up
            t0 = time.perf_counter()
            list(ex.map(one, range(len(files))))
            dt = time.perf_counter() - t0
        outs = [open(os.path.join(td, "o%d.jpg" % i), "rb").read() for i in range(len(files))]
    return len(files) / dt, outs, base is not None


def bench_jpegtran(a, isa):
    files = sources("A")
    rates = {"standalone": [], "reference": []}
    outs = {}
    for _ in range(a.repeats):                         # alternating
        for name, libdir in (("standalone", STANDALONE_DIR), ("reference", O.REF_DIR)):
            rate, outs[name], ramdisk = jpegtran_rate(files, libdir)
            rates[name].append(rate)
    res = {"files": len(files), "processes": 16, "switches": "-copy none -optimize", "on_ramdisk": ramdisk, "identical_files": outs["standalone"] == outs["reference"],
           "kernel_sha": {k: isa[k]["sha"] for k in KERNELS}}
    res.update({k: summary(v) for k, v in rates.items()})
    res["ratio_to_reference"] = res["standalone"]["median_files_per_s"] / res["reference"]["median_files_per_s"]
    return res


def existing_paths(a):
    """the child of --against: the two rates on the library MOZJPEG_AMD_LIB names, files from the pickle the parent process wrote"""
    import pickle
    from bench_transcode import timed as timed_transcode
    torch.cuda.init()
    files = pickle.load(open(a.existing_paths, "rb"))
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True), max_batch=len(files))
    timed(enc, files, 0.0, "pixels", None)
    pixels = timed(enc, files, a.seconds, "pixels", None)
    enc.close()
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True, optimize=True), max_batch=len(files))
    timed_transcode(enc, files, 0.0)
    transcode = timed_transcode(enc, files, a.seconds)
    enc.close()
    print(json.dumps({"pixels_device": pixels, "transcode_host": transcode}), flush=True)


def bench_against(a, isa):
    import pickle
    files = sources("A")
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    libs = {"this_tree": M.LIB_PATH, "parent": os.path.abspath(a.against)}
    rates = {k: {"pixels_device": [], "transcode_host": []} for k in libs}
    with tempfile.TemporaryDirectory(dir=base) as td:
        pkl = os.path.join(td, "files.pkl")
        pickle.dump(files, open(pkl, "wb"))
        for _ in range(a.repeats):                     # alternating
            for name, lib in libs.items():
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--existing-paths", pkl, "--seconds", str(a.seconds)],
                                     env=dict(os.environ, MOZJPEG_AMD_LIB=lib), stdout=subprocess.PIPE, check=True, timeout=120).stdout
                r = json.loads(out.decode().strip().splitlines()[-1])
                for k in r:
                    rates[name][k].append(r[k])
    res = {"files": len(files), "kernel_sha": {k: isa[k]["sha"] for k in KERNELS if k != "k_export_coefs"}}
    for name in libs:
        res[name] = {k: summary(v) for k, v in rates[name].items()}
    res["this_tree_over_parent"] = {k: res["this_tree"][k]["median_files_per_s"] / res["parent"][k]["median_files_per_s"] for k in ("pixels_device", "transcode_host")}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jpegtran", action="store_true")
    ap.add_argument("--against", default=None)
    ap.add_argument("--existing-paths", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--progressive", default=None, choices=["default", "simple"])
    ap.add_argument("--workload", default="A", choices=["A", "B"])
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.existing_paths:
        return existing_paths(a)
    isa = json.load(open(os.path.join(ROOT, "mozjpeg_amd", "kernel_isa.json")))["kernels"]
    key = "jpegtran" if a.jpegtran else "against" if a.against else "gpu"
    result = {key: {"jpegtran": bench_jpegtran, "against": bench_against, "gpu": bench_gpu}[key](a, isa)}
    print(json.dumps(result), flush=True)
    if a.out:
        with open(a.out + ("" if key == "gpu" else "_" + key) + ".json", "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
