#!/usr/bin/env python3
"""Lossless JPEG (SOF3) throughput on one GPU: device-resident batches of distinct 4K frames, two batches in flight (the encoder's own
stream), for 8-bit RGB with PSV 1 and PSV 6 and 16-bit gray with PSV 1.  Per configuration: Gpixels/s, ms per step, the step's
algorithmic bytes (input samples read once + files written) as a fraction of 8 TB/s, the per-kernel breakdown (mjh_set_profiling(1),
a separate pass: the events serialise the launches), and the reference's rate on 16 host threads (oracle/_ref/libturbojpeg.so.0,
tj3Compress8/16 with TJPARAM_LOSSLESS).  Every GPU file of the first step is compared with the reference's.
--scans each: the same frames as a script of one scan per component (the reference: `cjpeg -revert -lossless psv -scans FILE`, 16
processes at a time, files read from a RAM disk where there is one -- its TurboJPEG API has no scan scripts).
--through libjpeg: libjpeg client threads (tests/native/lossless_client bench) on the stand-alone libjpeg.so.62, 1 and 16 threads,
images/s beside the C-ABI figure: what host staging costs.
usage: python tools/bench_lossless.py [--batch 8] [--steps 20] [--warmup 3] [--ref-frames 32] [--scans each] [--through libjpeg]
                                      [--configs rgb8_psv1,...] [--repeats 1] [--out profiles/NAME]"""
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
import torch  # noqa: E402  (torch's runtime first: tests/conftest.py)
import numpy as np  # noqa: E402
import mozjpeg_amd as M  # noqa: E402
import lossless_cases as LC  # noqa: E402
import lossless_script_cases as SC  # noqa: E402
import oracle_lib as O  # noqa: E402

W, H = 3840, 2160
CONFIGS = [("rgb8_psv1", 8, 3, 1), ("rgb8_psv6", 8, 3, 6), ("gray16_psv1", 16, 1, 1)]
ROOFLINE = 8e12


def frames(n, prec, comps):
    """distinct frames: the SURVEY 8d synthetic frame (smooth colour fields + noise + saturated tiles) with a seed per frame; 16-bit
    gray = the 12-bit variant's first channel x 16"""
    if prec == 8:
        return [O.synthetic_frame(W, H, seed=1234 + i)[..., :comps] for i in range(n)]
    return [(O.synthetic_frame12(W, H, seed=1234 + i)[..., :comps].astype(np.uint32) * 16).astype(np.uint16) for i in range(n)]


def reference_rate(imgs, psv, prec, threads=16, total=32):
    L = LC.tj()
    handles = [L.tj3Init(0) for _ in range(threads)]
    fmt = "GRAY" if imgs[0].shape[2] == 1 else "RGB"

    def work(t):
        for k in range(t, total, threads):
            LC.tj_compress(imgs[k % len(imgs)], psv, 0, prec, fmt, handle=handles[t])
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(work, range(threads)))            # warm-up round
        t0 = time.perf_counter()
        list(ex.map(work, range(threads)))
        dt = time.perf_counter() - t0
    for h in handles:
        L.tj3Destroy(h)
    return total / dt


def reference_rate_cjpeg(imgs, script, prec, procs=16, total=32):
    """the reference on a scan script: its cjpeg, `procs` processes at a time; returns (frames/s, the files of imgs)"""
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    with tempfile.TemporaryDirectory(dir=base) as d:
        sf = os.path.join(d, "s.scans")
        with open(sf, "w") as f:
            f.write(SC.script_text(script))
        for i, a in enumerate(imgs):
            LC.write_pnm(os.path.join(d, "%d.pnm" % i), a, prec)
        cmd = [LC.CJPEG, "-revert", "-lossless", "1"] + (["-precision", str(prec)] if prec != 8 else []) + ["-scans", sf]

        def work(k):
            return subprocess.run(cmd + [os.path.join(d, "%d.pnm" % (k % len(imgs)))], capture_output=True, check=True).stdout
        with ThreadPoolExecutor(procs) as ex:
            files = list(ex.map(work, range(len(imgs))))
            t0 = time.perf_counter()
            list(ex.map(work, range(total)))
            dt = time.perf_counter() - t0
    return total / dt, files


def through_libjpeg(psv, each, images_per_thread=8):
    """client threads on the stand-alone library: {threads: images/s}"""
    client = os.path.join(ROOT, "tests", "native", "lossless_client")
    env = dict(os.environ)
    O.set_preload(env)
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "mozjpeg_amd", "standalone")
    out = {}
    for threads in (1, 16):
        r = subprocess.run([client, "bench", str(threads), str(images_per_thread), str(W), str(H), str(psv)] + (["each"] if each else []),
                           env=env, capture_output=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(r.stderr.decode()[-500:])
        out[str(threads)] = json.loads(r.stdout.decode().strip().splitlines()[-1])["images_per_s"]
    return out


def run(name, prec, comps, psv, a):
    imgs = frames(a.batch, prec, comps)
    host = np.stack(imgs)
    d = torch.from_numpy(host.view(np.int16) if prec > 8 else host).cuda()
    script = [((c,), psv, 0) for c in range(comps)] if a.scans == "each" else None
    enc = M.Encoder(SC.params(M, imgs[0], script, prec) if script else LC.params(M, imgs[0], psv, 0, prec), max_batch=a.batch)
    enc.encode_tensor(d, stream="own")
    files = [enc.get_jpeg(i) for i in range(a.batch)]
    ref_fps = None
    if script:
        ref_fps, refs = reference_rate_cjpeg(imgs, script, prec, total=a.ref_frames)
    else:
        with ThreadPoolExecutor(16) as ex:
            refs = list(ex.map(lambda f: LC.tj_compress(f, psv, 0, prec, "GRAY" if comps == 1 else "RGB"), imgs))
    identical = files == refs
    for _ in range(a.warmup):
        enc.encode_tensor(d, stream="own")
    enc.sync()
    repeats = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            enc.encode_tensor(d, stream="own")
        enc.sync()
        repeats.append((time.perf_counter() - t0) / a.steps)
    dt = min(repeats)
    in_bytes = host.nbytes
    out_bytes = sum(len(f) for f in files)
    enc.set_inflight(1)
    enc.set_profiling(1)
    for _ in range(5):
        enc.encode_tensor(d, stream="own")
    kt = enc.kernel_times()
    enc.set_profiling(0)
    if ref_fps is None:
        ref_fps = reference_rate(imgs, psv, prec, total=a.ref_frames)
    gpu_fps = a.batch / dt
    extra = {}
    if a.through == "libjpeg" and prec == 8 and comps == 3:
        extra["libjpeg_standalone_images_per_s_by_threads"] = through_libjpeg(psv, bool(script))
    return {
        **extra, "scans": len(script) if script else 1, "ms_per_step_repeats": [round(x * 1e3, 3) for x in repeats],
        "reference": "cjpeg, 16 processes" if script else "TurboJPEG, 16 threads",
        "config": name, "precision": prec, "components": comps, "psv": psv, "batch": a.batch, "width": W, "height": H,
        "identical_to_reference": identical, "ms_per_step": round(dt * 1e3, 3), "gpixels_per_s": round(W * H * a.batch / dt / 1e9, 2),
        "algorithmic_bytes_per_step": in_bytes + out_bytes, "input_bytes": in_bytes, "file_bytes": out_bytes,
        "ratio": round(in_bytes / out_bytes, 3), "roofline_fraction": round((in_bytes + out_bytes) / dt / ROOFLINE, 4),
        "kernel_ms_per_step": {k: round(v, 4) for k, v in kt},
        "reference_frames_per_s_16_threads": round(ref_fps, 2), "gpu_frames_per_s": round(gpu_fps, 1),
        "speedup_vs_reference": round(gpu_fps / ref_fps, 1),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ref-frames", type=int, default=32)
    ap.add_argument("--scans", choices=["one", "each"], default="one", help="each: a script of one scan per component")
    ap.add_argument("--through", choices=["abi", "libjpeg"], default="abi", help="libjpeg: also client threads on the stand-alone library (8-bit RGB)")
    ap.add_argument("--configs", default=None, help="comma-separated subset of " + ",".join(c[0] for c in CONFIGS))
    ap.add_argument("--repeats", type=int, default=1, help="timed repeats of --steps steps; ms_per_step is the fastest, all are listed")
    ap.add_argument("--out", default=None, help="write NAME.json next to the printed lines")
    a = ap.parse_args()
    res = []
    for name, prec, comps, psv in CONFIGS:
        if a.configs and name not in a.configs.split(","):
            continue
        r = run(name, prec, comps, psv, a)
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        with open(a.out + ".json", "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "library": M.lib().mjh_version().decode(), "results": res}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
