#!/usr/bin/env python3
"""Region decode against the whole decode of the same files on one GPU (mjh_decode_opts.crop_*: djpeg -crop WxH+X+Y).

The 64 distinct seeded 4K 4:2:0 q75 sequential files of tools/bench_decode.py's workload A, once without restart markers and once
with a restart interval of one MCU row (cjpeg -restart 1).  Per variant, from the same run and the same encoder, alternating whole
and region calls on one host thread:
  1. files/s of the region call next to the whole decode, to pixels in device memory (mjh_decode_host + mjh_encoder_sync) and
  2. to pixels in pinned host memory (+ mjh_get_pixels of every image): --repeats rounds of >= --seconds each after a warm-up;
  3. under mjh_set_profiling(1), a separate pass: the Huffman decoder's phases and the two pixel kernels' times of both calls
     (k_idct / k_upcolor next to k_idct_region / k_upcolor_region), median of 9 alternating calls;
  4. restart segments decoded out of those the files have.
The region's pixels of the first files are compared with the reference's djpeg -crop before anything is timed.

usage: python tools/bench_decode_region.py [--crop 256x256+1800+900] [--seconds 2] [--repeats 3] [--files 64] [--out profiles/region_decode_bench]"""
import argparse
import json
import os
import sys
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
import oracle_lib as O  # noqa: E402
import transcode_cases as TC  # noqa: E402
from bench_decode import timed, median  # noqa: E402

VARIANTS = {"no_restart": [], "restart_1_row": ["-restart", "1"]}


def make_files(n, extra):
    imgs = [O.synthetic_frame(3840, 2160, seed=1234 + i) for i in range(n)]
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda a: TC.cjpeg(a, ["-revert", "-quality", "75", "-sample", "2x2"] + extra), imgs))


def bench_variant(files, crop, seconds, repeats):
    n = len(files)
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True), max_batch=n)
    opts = {"whole": M.decode_opts(), "region": M.decode_opts(crop=crop)}
    outs = enc.decode_host(files, opts=opts["region"])
    x, y, w, h = enc.decode_region()
    kept, total = enc.decode_segments()
    with ThreadPoolExecutor(16) as ex:
        same = list(ex.map(lambda i: bool(np.array_equal(outs[i], DC.djpeg(files[i], ["-crop", crop]))), range(min(n, 8))))
    del outs
    info = M.jpeg_info(files[0])
    host = {"whole": M.pinned_empty((n, info.image_height, info.image_width, 3)), "region": M.pinned_empty((n, h, w, 3))}
    res = {"files": n, "width": info.image_width, "height": info.image_height, "crop": crop, "region_decoded": [x, y, w, h],
           "identical_to_djpeg_crop": all(same), "segments_decoded": kept, "segments": total, "segments_pruned": total - kept,
           "seconds": seconds, "repeats": repeats, "files_per_s": {}}
    for name in opts:                                   # warm-up of both paths
        timed(enc, files, 0.3, None, opts[name])
        timed(enc, files, 0.3, host[name], opts[name])
    rates = {(name, dst): [] for name in opts for dst in ("device", "host")}
    for _ in range(repeats):
        for name in opts:
            rates[(name, "device")].append(timed(enc, files, seconds, None, opts[name]))
            rates[(name, "host")].append(timed(enc, files, seconds, host[name], opts[name]))
    for (name, dst), v in rates.items():
        res["files_per_s"]["%s_to_%s" % (name, dst)] = {"median": median(v), "all": v}
    for dst in ("device", "host"):
        res["files_per_s"]["region_over_whole_to_%s" % dst] = median(rates[("region", dst)]) / median(rates[("whole", dst)])
    enc.set_profiling(1)
    ms = {name: [] for name in opts}
    for r in range(11):
        for name in opts:
            enc.submit_decode(files, opts=opts[name])
            enc.sync()
            if r >= 2:
                ms[name].append(dict(enc.transcode_stats()["ms"], **enc.decode_stats()["ms"]))
    enc.close()
    res["phase_ms"] = {name: {k: median([m[k] for m in v]) for k in v[0]} for name, v in ms.items()}
    return res


def table(result):
    lines = ["# Region decode against the whole decode", "",
             "`python tools/bench_decode_region.py --crop %s`: %d 4K 4:2:0 q75 files per call, one MI355X, one host thread; files/s are medians of %d rounds of %.1f s."
             % (result["crop"], result["files"], result["repeats"], result["seconds"]), ""]
    for name, r in result["variants"].items():
        f, p = r["files_per_s"], r["phase_ms"]
        lines += ["## %s" % name, "",
                  "Region asked %s, decoded %dx%d+%d+%d; identical to djpeg -crop: %s; restart segments decoded %d of %d (%d left out)."
                  % (r["crop"], r["region_decoded"][2], r["region_decoded"][3], r["region_decoded"][0], r["region_decoded"][1], r["identical_to_djpeg_crop"],
                     r["segments_decoded"], r["segments"], r["segments_pruned"]), "",
                  "| files/s | whole | region | region / whole |", "|---|---|---|---|"]
        for dst in ("device", "host"):
            lines.append("| to %s memory | %.0f | %.0f | %.2f |" % ("device" if dst == "device" else "pinned host", f["whole_to_%s" % dst]["median"], f["region_to_%s" % dst]["median"],
                                                                   f["region_over_whole_to_%s" % dst]))
        lines += ["", "| ms per call | whole | region |", "|---|---|---|"]
        for k in p["whole"]:
            lines.append("| %s | %.3f | %.3f |" % ({"idct": "inverse DCT (k_idct / k_idct_region)", "upcolor": "upsampling + colour (k_upcolor / k_upcolor_region)"}.get(k, "Huffman decoder: " + k),
                                                   p["whole"][k], p["region"][k]))
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crop", default="256x256+1800+900")
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_decode_bench"))
    a = ap.parse_args()
    isa = json.load(open(os.path.join(ROOT, "mozjpeg_amd", "kernel_isa.json")))["kernels"]
    result = {"crop": a.crop, "files": a.files, "seconds": a.seconds, "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
              "kernel_sha": {k: isa[k]["sha"] for k in isa if k.startswith(("k_idct_region", "k_upcolor_region", "k_upcolor_565_region"))}, "variants": {}}
    for name, extra in VARIANTS.items():
        t0 = time.perf_counter()
        files = make_files(a.files, extra)
        result["variants"][name] = bench_variant(files, a.crop, a.seconds, a.repeats)
        print(json.dumps({name: result["variants"][name], "wall_s": time.perf_counter() - t0}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out + ".json", "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    with open(a.out + ".md", "w") as f:
        f.write(table(result) + "\n")


if __name__ == "__main__":
    main()
