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
--scale M/N: both workloads decoded at that scale (all_scales=True: any of the sixteen IDCT sizes), the reference being djpeg -scale
M/N.  At the twelve sizes of k_idct_sized one file per call is compared with djpeg (file 0), and above full size only the path to
device memory is timed (64 enlarged 4K images do not belong in pinned host memory); the result then names the bytes of sample
planes the transform writes per second.
--dct fast: instead of the above, the K-I1 time of k_idct_ifast (mjh_decode_opts.dct_method 1) next to k_idct's on the same batch of
workload A, alternating calls under mjh_set_profiling(1); the fast pixels of the first call are compared with djpeg -dct fast.
--color rgb565: instead of the above, the K-I2 time of k_upcolor_565 (16-bit pixels, ordered dither and plain) next to k_upcolor's
(3-byte RGB) on the same batch of workload A, alternating calls under mjh_set_profiling(1); the 565 pixels of the first call are
compared with djpeg -rgb565 -bmp.
--tj: instead of the above, files/s of tj3Decompress8 (TJPF_RGB, full size) through mozjpeg_amd/libmozjpeg_hip_turbojpeg.so on 8 files
of workload A from one thread -- one image per call, each call synchronises -- next to the reference's oracle/_ref/libturbojpeg.so.0
in the same process, alternating rounds; the two libraries' pixels are compared first.
--progressive default|simple: the workloads' images as progressive files (the reference's cjpeg with its default switches, or with
-revert -progressive), decoded with Encoder.set_sources(progressive=True); phase_ms then holds "refinement", the refinement levels' time.
--source ycck420: instead of the above, workload A's 64 frames as four-component files -- 4K YCCK 4:2:0 with K sampled 2x2, made by the
reference's tj3Compress8(TJPF_CMYK, TJCS_YCCK, TJSAMP_420) from the synthetic frames (inverted) plus a K plane -- decoded to CMYK pixels
(k_upcolor4): files/s to device and to pinned host memory, the phase times, the reference's djpeg from 16 processes on the same files,
and the YCbCr files of the same frames decoded in the same run for k_upcolor's time per pixel; every file's pixels are first compared
with the reference's tj3Decompress8(TJPF_CMYK).
--source arith420: workload A's 64 frames as arithmetic-coded files (cjpeg -revert -arithmetic, with and without a restart interval),
decoded with Encoder.set_sources(arithmetic=True) against the reference's djpeg on the same files.

usage: python tools/bench_decode.py [--progressive default|simple] [--source ycck420|arith420] [--workloads A,B] [--scale 1/1] [--dct fast] [--color rgb565] [--tj] [--seconds 2] [--repeats 3] [--out profiles/decode_bench]"""
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


def median(v):
    return sorted(v)[len(v) // 2]


def bench_dct_fast(a, isa):
    """K-I1 of both IDCT methods on the 64 x 4K batch: ms per call (median of `rounds` alternating calls, device events)"""
    files = sources("A")
    n = len(files)
    info = M.jpeg_info(files[0])
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True), max_batch=n)
    opts = {"int": M.decode_opts(dct="int"), "fast": M.decode_opts(dct="fast")}
    outs = enc.decode_host(files[:n], opts=opts["fast"])
    with ThreadPoolExecutor(16) as ex:
        same = list(ex.map(lambda i: bool(np.array_equal(outs[i], DC.djpeg(files[i], ["-dct", "fast"]))), range(n)))
    del outs
    enc.set_profiling(1)
    ms = {"int": [], "fast": []}
    up = {"int": [], "fast": []}
    rounds = 11
    for r in range(rounds + 2):
        for name in ("int", "fast"):
            enc.submit_decode(files, opts=opts[name])
            enc.sync()
            st = enc.decode_stats()["ms"]
            if r >= 2:                                  # (two warm-up rounds)
                ms[name].append(st["idct"])
                up[name].append(st["upcolor"])
    enc.close()
    w, h = info.image_width, info.image_height
    traffic = n * w * h * 1.5 * 3                       # coefficients read (2 bytes a sample) + samples written
    res = {"files": n, "width": w, "height": h, "rounds": rounds, "identical_to_djpeg_dct_fast": all(same),
           "kernel_sha": {k: isa[k]["sha"] for k in ("k_idct", "k_idct_ifast")}, "vgpr": {k: isa[k]["vgpr"] for k in ("k_idct", "k_idct_ifast")},
           "k_idct_ms": median(ms["int"]), "k_idct_ifast_ms": median(ms["fast"]), "k_idct_ms_all": ms["int"], "k_idct_ifast_ms_all": ms["fast"],
           "k_upcolor_ms": median(up["int"] + up["fast"]),
           "k_idct_gbytes_per_s": traffic / median(ms["int"]) / 1e6, "k_idct_ifast_gbytes_per_s": traffic / median(ms["fast"]) / 1e6}
    res["ifast_over_islow"] = res["k_idct_ifast_ms"] / res["k_idct_ms"]
    return res


def bench_rgb565(a, isa):
    """K-I2 of the 3-byte and the 565 kernels on the 64 x 4K batch: ms per call (median of `rounds` alternating calls, device events)"""
    import djpeg_cases as DJ
    files = sources("A")
    n = len(files)
    info = M.jpeg_info(files[0])
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True), max_batch=n)
    opts = {"rgb": M.decode_opts(color="rgb"), "rgb565": M.decode_opts(color="rgb565"), "rgb565_plain": M.decode_opts(color="rgb565", dither=False)}
    outs = enc.decode_host(files[:n], opts=opts["rgb565"])
    with ThreadPoolExecutor(16) as ex:
        same = list(ex.map(lambda i: bool(DJ.same565(outs[i], DJ.djpeg565(files[i]))), range(n)))
    del outs
    enc.set_profiling(1)
    ms = {k: [] for k in opts}
    rounds = 11
    for r in range(rounds + 2):
        for name in opts:
            enc.submit_decode(files, opts=opts[name])
            enc.sync()
            if r >= 2:                                  # (two warm-up rounds)
                ms[name].append(enc.decode_stats()["ms"]["upcolor"])
    enc.close()
    w, h = info.image_width, info.image_height
    planes = n * w * h * 1.5                            # 4:2:0: 1.5 samples a pixel read
    res = {"files": n, "width": w, "height": h, "rounds": rounds, "identical_to_djpeg_rgb565": all(same),
           "kernel_sha": {k: isa[k]["sha"] for k in ("k_upcolor", "k_upcolor_565")}, "vgpr": {k: isa[k]["vgpr"] for k in ("k_upcolor", "k_upcolor_565")},
           "k_upcolor_ms": median(ms["rgb"]), "k_upcolor_565_ms": median(ms["rgb565"]), "k_upcolor_565_plain_ms": median(ms["rgb565_plain"]),
           "ms_all": ms,
           "k_upcolor_gbytes_per_s": (planes + n * w * h * 3) / median(ms["rgb"]) / 1e6,
           "k_upcolor_565_gbytes_per_s": (planes + n * w * h * 2) / median(ms["rgb565"]) / 1e6}
    res["rgb565_over_rgb"] = res["k_upcolor_565_ms"] / res["k_upcolor_ms"]
    return res


def bench_tj(a, isa):
    """tj3Decompress8, one image per call from one thread: the shipped TurboJPEG-signature library against the reference's"""
    import ctypes as C
    import tj_decompress_cases as TD
    files = sources("A")[:8]
    info = M.jpeg_info(files[0])
    w, h = info.image_width, info.image_height
    libs = {"mozjpeg_hip_turbojpeg": TD.load(TD.TJSHIM), "reference_libturbojpeg": TD.load(TD.TJLIB)}
    handles = {k: L.tj3Init(TD.TJINIT_DECOMPRESS) for k, L in libs.items()}
    bufs = {k: np.zeros((h, w, 3), np.uint8) for k in libs}

    def one(k, f):
        rc = libs[k].tj3Decompress8(handles[k], f, len(f), bufs[k].ctypes.data, 0, TD.PF_RGB)
        assert rc == 0, libs[k].tj3GetErrorStr(handles[k])

    same = []
    for f in files:
        for k in libs:
            one(k, f)
        same.append(bool(np.array_equal(*bufs.values())))
    rates = {k: [] for k in libs}
    for _ in range(a.repeats):
        for k in libs:
            calls, t0 = 0, time.perf_counter()
            while True:
                one(k, files[calls % len(files)])
                calls += 1
                dt = time.perf_counter() - t0
                if dt >= a.seconds:
                    break
            rates[k].append(calls / dt)
    for k, L in libs.items():
        L.tj3Destroy(handles[k])
    res = {"files": len(files), "width": w, "height": h, "identical_to_reference": all(same), "threads": 1,
           "kernel_sha": {k: isa[k]["sha"] for k in ("k_dec_sync", "k_dec_store", "k_idct", "k_upcolor")}}
    for k, v in rates.items():
        res[k] = {"files_per_s": v, "median_files_per_s": median(v), "median_mpixels_per_s": median(v) * w * h / 1e6, "spread": (max(v) - min(v)) / median(v)}
    res["ratio_to_reference"] = res["mozjpeg_hip_turbojpeg"]["median_files_per_s"] / res["reference_libturbojpeg"]["median_files_per_s"]
    return res


def bench_ycck(a, isa):
    """the 64 x 4K frames as YCCK 4:2:0 files -> CMYK pixels, next to the same frames as YCbCr 4:2:0 files -> RGB pixels"""
    import cmyk_cases as K
    import oracle_lib as O
    import transcode_cases as TC
    n = 64
    with ThreadPoolExecutor(16) as ex:
        imgs = list(ex.map(lambda i: O.synthetic_frame(3840, 2160, seed=1234 + i), range(n)))
        cmyk = lambda im: np.ascontiguousarray(np.concatenate([255 - im, np.roll(im[..., 1:2], (540, 960), (0, 1))], axis=-1))
        files = list(ex.map(lambda im: K.tj_compress(cmyk(im), K.TJCS_YCCK, K.TJSAMP_420, quality=75), imgs))
        ycc = list(ex.map(lambda im: TC.cjpeg(im, ["-revert", "-quality", "75", "-sample", "2x2"]), imgs))
    del imgs
    info = M.jpeg_info(files[0])
    w, h = info.image_width, info.image_height
    assert info.jpeg_color_space == M.CS_YCCK and [info.h_samp_factor[c] for c in range(4)] == [2, 1, 1, 2]
    res = {"files": n, "width": w, "height": h, "source_bytes": sum(len(f) for f in files), "ycbcr_source_bytes": sum(len(f) for f in ycc),
           "kernel_sha": {k: isa[k]["sha"] for k in ("k_dec_sync", "k_dec_store", "k_idct", "k_upcolor", "k_upcolor4")},
           "vgpr": {k: isa[k]["vgpr"] for k in ("k_upcolor", "k_upcolor4")}}
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True), max_batch=n)
    opts = M.decode_opts()
    outs = enc.decode_host(files, opts=opts)
    assert outs[0].shape == (h, w, 4)
    with ThreadPoolExecutor(16) as ex:
        same = list(ex.map(lambda i: bool(np.array_equal(outs[i], K.tj_pixels(files[i])[1])), range(n)))
    del outs
    res["identical_to_reference"] = all(same)
    res["reference_files_per_s"], res["reference_on_ramdisk"] = reference_rate(files)
    res["reference_ycbcr_files_per_s"] = reference_rate(ycc)[0]
    host = M.pinned_empty((n, h, w, 4))
    paths = {"device": None, "host": host}
    res["paths"] = {}
    for name, dst in paths.items():
        timed(enc, files, 0.0, dst, opts)              # warm-up
        res["paths"][name] = {"files_per_s": []}
    for _ in range(a.repeats):                         # alternating
        for name, dst in paths.items():
            res["paths"][name]["files_per_s"].append(timed(enc, files, a.seconds, dst, opts))
    for name in paths:
        c = res["paths"][name]
        v = c["files_per_s"]
        c["median_files_per_s"] = median(v)
        c["median_mpixels_per_s"] = c["median_files_per_s"] * w * h / 1e6
        c["spread"] = (max(v) - min(v)) / c["median_files_per_s"]
        c["ratio_to_reference"] = c["median_files_per_s"] / res["reference_files_per_s"]
    del host
    # the phases of both kinds of file, alternating calls under the profiler (two warm-up rounds, the median of 7)
    enc3 = M.Encoder(M.params_from_jpeg(ycc[0], revert=True), max_batch=n)
    ms = {"ycck": [], "ycbcr": []}
    for e in (enc, enc3):
        e.set_profiling(1)
    for r in range(9):
        for name, e, fs in (("ycck", enc, files), ("ycbcr", enc3, ycc)):
            e.submit_decode(fs, opts=opts)
            e.sync()
            if r >= 2:
                ms[name].append(dict(e.transcode_stats()["ms"], **e.decode_stats()["ms"]))
    stats = {"ycck": {k: v for k, v in enc.transcode_stats().items() if k != "ms"}, "ycbcr": {k: v for k, v in enc3.transcode_stats().items() if k != "ms"}}
    enc.close()
    enc3.close()
    res["phase_ms"] = {name: {k: median([m[k] for m in v]) for k in v[0]} for name, v in ms.items()}
    res["stats"] = stats
    px = n * w * h
    # algorithmic bytes per pixel of the colour kernels: 2.25 samples in and 4 bytes out against 1.5 in and 3 out
    res["k_upcolor4_gbytes_per_s"] = px * 6.25 / res["phase_ms"]["ycck"]["upcolor"] / 1e6
    res["k_upcolor_gbytes_per_s"] = px * 4.5 / res["phase_ms"]["ycbcr"]["upcolor"] / 1e6
    res["upcolor4_over_upcolor_time_per_pixel"] = res["phase_ms"]["ycck"]["upcolor"] / res["phase_ms"]["ycbcr"]["upcolor"]
    res["bytes_ratio"] = 6.25 / 4.5
    return res


def bench_arith(a, isa):
    """workload A's 64 x 4K frames as arithmetic-coded 4:2:0 files (cjpeg -revert -arithmetic, SOF9) -> RGB pixels, once with a
    restart interval of one MCU row (135 chains per file) and once without (one chain per file); the reference: djpeg on the same
    files, 16 processes.  One wave decodes one chain, so the files/s follow the chains in flight, not the bytes."""
    import oracle_lib as O
    import transcode_cases as TC
    n = 64
    res = {"files": n, "kernel_sha": {"k_adec_scans": isa["k_adec_scans"]["sha"]}, "vgpr": isa["k_adec_scans"]["vgpr"], "variants": {}}
    with ThreadPoolExecutor(16) as ex:
        imgs = list(ex.map(lambda i: O.synthetic_frame(3840, 2160, seed=1234 + i), range(n)))
        variants = {"restart_1_row": list(ex.map(lambda im: TC.cjpeg(im, ["-revert", "-quality", "75", "-sample", "2x2", "-restart", "1", "-arithmetic"]), imgs)),
                    "no_restart": list(ex.map(lambda im: TC.cjpeg(im, ["-revert", "-quality", "75", "-sample", "2x2", "-arithmetic"]), imgs))}
    del imgs
    opts = M.decode_opts()
    for name, files in variants.items():
        info = M.jpeg_info(files[0], arithmetic_sources=True)
        w, h = info.image_width, info.image_height
        assert info.sof_type == 9
        enc = M.Encoder(M.params_from_jpeg(info, revert=True), max_batch=n)
        enc.set_sources(progressive=False, arithmetic=True)
        outs = enc.decode_host(files, opts=opts)
        with ThreadPoolExecutor(16) as ex:
            same = list(ex.map(lambda i: bool(np.array_equal(outs[i], DC.djpeg(files[i]))), range(n)))
        del outs
        r = {"width": w, "height": h, "source_bytes": sum(len(f) for f in files), "identical_to_reference": all(same)}
        r["reference_files_per_s"], r["reference_on_ramdisk"] = reference_rate(files)
        timed(enc, files, 0.0, None, opts)                # warm-up
        v = [timed(enc, files, a.seconds, None, opts) for _ in range(a.repeats)]
        r["files_per_s"] = v
        r["median_files_per_s"] = median(v)
        r["spread"] = (max(v) - min(v)) / median(v)
        r["ratio_to_reference"] = median(v) / r["reference_files_per_s"]
        enc.set_profiling(1)
        ms = []
        for _ in range(3):
            enc.submit_decode(files, opts=opts)
            enc.sync()
            ms.append(enc.arith_stats())
        r["arith"] = dict(ms[0], ms=median([m["ms"] for m in ms]))
        enc.close()
        res["variants"][name] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="A,B")
    ap.add_argument("--scale", default="1/1")
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dct", default=None, choices=["fast"])
    ap.add_argument("--tj", action="store_true")
    ap.add_argument("--color", default=None, choices=["rgb565"])
    ap.add_argument("--progressive", default=None, choices=["default", "simple"])
    ap.add_argument("--source", default=None, choices=["ycck420", "arith420"])
    a = ap.parse_args()
    prog = a.progressive is not None
    if a.dct or a.tj or a.color or a.source:
        isa = json.load(open(os.path.join(ROOT, "mozjpeg_amd", "kernel_isa.json")))
        result = {"source_stamp": isa.get("source_stamp")}
        if a.dct:
            result["dct_fast"] = bench_dct_fast(a, isa["kernels"])
            print(json.dumps({"dct_fast": result["dct_fast"]}), flush=True)
        if a.color:
            result["rgb565"] = bench_rgb565(a, isa["kernels"])
            print(json.dumps({"rgb565": result["rgb565"]}), flush=True)
        if a.tj:
            result["tj"] = bench_tj(a, isa["kernels"])
            print(json.dumps({"tj": result["tj"]}), flush=True)
        if a.source == "ycck420":
            result["ycck420"] = bench_ycck(a, isa["kernels"])
            print(json.dumps({"ycck420": result["ycck420"]}), flush=True)
        if a.source == "arith420":
            result["arith420"] = bench_arith(a, isa["kernels"])
            print(json.dumps({"arith420": result["arith420"]}), flush=True)
        if a.out:
            with open(a.out + ".json", "w") as f:
                json.dump(result, f, indent=1)
        return
    opts = M.decode_opts(scale=a.scale, all_scales=True)
    k = M.scale_idct_size(opts.scale_num, opts.scale_denom)
    dj_args = ["-scale", a.scale] if k != 8 else []
    isa = json.load(open(os.path.join(ROOT, "mozjpeg_amd", "kernel_isa.json")))["kernels"]
    result = {"kernel_sha": {k: isa[k]["sha"] for k in isa if k in ("k_dec_sync", "k_dec_prefix", "k_dec_store", "k_dec_dc", "k_idct", "k_upcolor") or k.startswith("k_idct_scaled") or k.startswith("k_idct_sized")},
              "scale": a.scale, "idct_size": k, "progressive_sources": a.progressive, "workloads": {}}
    for wl in a.workloads.split(","):
        files = sources(wl, a.progressive)
        n = len(files)
        info = M.jpeg_info(files[0], prog)
        w, h = info.image_width, info.image_height
        enc = M.Encoder(M.params_from_jpeg(files[0], revert=True, progressive_sources=prog), max_batch=n)
        enc.set_sources(progressive=prog)
        ow, oh = -(-w * k // 8), -(-h * k // 8)
        if k in M.SCALED_IDCT_SIZES:
            outs = enc.decode_host(files, opts=opts)
            assert outs[0].shape == (oh, ow, 3)
            with ThreadPoolExecutor(16) as ex:
                same = list(ex.map(lambda i: bool(np.array_equal(outs[i], DC.djpeg(files[i], dj_args))), range(n)))
            del outs
        else:                                          # one file per call
            enc.submit_decode(files, opts=opts)
            out0 = enc.get_pixels(0)
            assert out0.shape == (oh, ow, 3)
            same = [bool(np.array_equal(out0, DC.djpeg(files[0], dj_args)))]
            del out0
        ref_rate, ramdisk = reference_rate(files, dj_args)
        r = {"files": n, "width": w, "height": h, "out_width": ow, "out_height": oh, "source_bytes": sum(len(f) for f in files), "identical_to_reference": all(same),
             "reference_files_per_s": ref_rate, "reference_on_ramdisk": ramdisk, "stats": {k: v for k, v in enc.transcode_stats().items() if k != "ms"}, "paths": {}}
        host = M.pinned_empty((n, oh, ow, 3)) if k <= 8 else None
        paths = {"device": None, "host": host} if k <= 8 else {"device": None}
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
            if prog:
                ms[-1]["refinement"] = enc.prog_stats()["ms"]
                r["levels"] = enc.prog_stats()["levels"]
        enc.set_profiling(0)
        r["phase_ms"] = {k: sorted(m[k] for m in ms)[len(ms) // 2] for k in ms[0]}
        # byte counts of the pixel kernels: coefficients read + planes written; planes read + pixels written (4:2:0: 1.5 samples a pixel)
        # (full size only: a reduced transform reads a subset of the coefficient planes that depends on every component's size)
        if k == 8:
            coef_bytes, plane_bytes, pix_bytes = n * w * h * 1.5 * 2, n * w * h * 1.5, n * w * h * 3
            r["idct_gbytes_per_s"] = (coef_bytes + plane_bytes) / r["phase_ms"]["idct"] / 1e6
            r["upcolor_gbytes_per_s"] = (plane_bytes + pix_bytes) / r["phase_ms"]["upcolor"] / 1e6
        if k >= 8:                                     # (4:2:0: every component is at k itself from full size up)
            r["idct_plane_gbytes_written_per_s"] = n * w * h * 1.5 * (k / 8.0) ** 2 / r["phase_ms"]["idct"] / 1e6
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
