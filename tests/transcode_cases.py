"""The case list of the re-compression tests (test_simt_transcode.py on the emulator, test_gpu_transcode.py on the chip).

Sources are made at test time by the reference's cjpeg (oracle/_ref/cjpeg) from tests/golden/testorig.ppm and seeded synthetic
images, and by the oracle (oracle_lib.encode) for the max-compression profile's sequential files; the expected bytes always come
from the reference's jpegtran (oracle_lib.ref_jpegtran) at test time."""
import functools
import os
import subprocess
import tempfile

import numpy as np

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PPM = os.path.join(ROOT, "tests", "golden", "testorig.ppm")
CJPEG = os.path.join(O.REF_DIR, "cjpeg")
JPEGTRAN = os.path.join(O.REF_DIR, "jpegtran")

# three sequential scans, one component each (non-interleaved)
SCRIPT_3 = "0: 0 63 0 0;\n1: 0 63 0 0;\n2: 0 63 0 0;\n"


def have_tools():
    return os.path.exists(CJPEG) and os.path.exists(JPEGTRAN)


def cjpeg(img, args, script=None):
    """the reference's cjpeg on an [H, W, 3] uint8 image"""
    with tempfile.TemporaryDirectory() as td:
        h, w = img.shape[:2]
        with open(os.path.join(td, "in.ppm"), "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(img, dtype=np.uint8).tobytes())
        args = list(args)
        if script is not None:
            with open(os.path.join(td, "scans.txt"), "w") as f:
                f.write(script)
            args += ["-scans", os.path.join(td, "scans.txt")]
        outp = os.path.join(td, "out.jpg")
        subprocess.check_call([CJPEG] + args + ["-outfile", outp, os.path.join(td, "in.ppm")])
        with open(outp, "rb") as f:
            return f.read()


def jpegtran_status(jpeg, switches):
    """(exit status, output bytes or None) of the reference's jpegtran: 0 = clean, 2 = warnings, 1 = error"""
    with tempfile.TemporaryDirectory() as td:
        inp, outp = os.path.join(td, "in.jpg"), os.path.join(td, "out.jpg")
        with open(inp, "wb") as f:
            f.write(jpeg)
        r = subprocess.run([JPEGTRAN] + list(switches) + ["-outfile", outp, inp], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        data = None
        if os.path.exists(outp):
            with open(outp, "rb") as f:
                data = f.read()
        return r.returncode, data


@functools.lru_cache(maxsize=None)
def testorig():
    return O.read_ppm(PPM)


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def patch_jfif(jpeg, major, minor, unit, xd, yd):
    assert jpeg[2:4] == b"\xff\xe0" and jpeg[6:11] == b"JFIF\0"
    return jpeg[:11] + bytes([major, minor, unit, xd >> 8, xd & 255, yd >> 8, yd & 255]) + jpeg[18:]


# name -> what the test knows about the source: builder, and the facts test 5 checks (size, components, sampling of component 0,
# scans, restart interval of the first scan, colour space name)
def _src_revert():
    return cjpeg(testorig(), ["-revert"])


SOURCES = {
    "revert": dict(make=_src_revert, size=(227, 149), nc=3, samp0=(2, 2), scans=1, ri=0, cs="YCbCr"),
    "revert_opt": dict(make=lambda: cjpeg(testorig(), ["-revert", "-optimize"]), size=(227, 149), nc=3, samp0=(2, 2), scans=1, ri=0, cs="YCbCr"),
    "q90_2x1_r1": dict(make=lambda: cjpeg(testorig(), ["-revert", "-quality", "90", "-sample", "2x1", "-restart", "1"]),
                       size=(227, 149), nc=3, samp0=(2, 1), scans=1, ri=15, cs="YCbCr"),
    "gray_r5b": dict(make=lambda: cjpeg(testorig(), ["-revert", "-optimize", "-grayscale", "-restart", "5B"]),
                     size=(227, 149), nc=1, samp0=(1, 1), scans=1, ri=5, cs="GRAYSCALE"),
    "scans3_2x2_r2": dict(make=lambda: cjpeg(testorig(), ["-revert", "-sample", "2x2", "-restart", "2"], script=SCRIPT_3),
                          size=(227, 149), nc=3, samp0=(2, 2), scans=3, ri=58, cs="YCbCr"),
    "rgb": dict(make=lambda: cjpeg(testorig(), ["-revert", "-rgb"]), size=(227, 149), nc=3, samp0=(1, 1), scans=1, ri=0, cs="RGB"),
    "cjpeg_baseline": dict(make=lambda: cjpeg(testorig(), ["-baseline"]), size=(227, 149), nc=3, samp0=(2, 2), scans=1, ri=0, cs="YCbCr"),
    "oracle_baseline": dict(make=lambda: oracle_source()[0], size=(200, 120), nc=3, samp0=(2, 2), scans=1, ri=0, cs="YCbCr"),
    "jfif102": dict(make=lambda: patch_jfif(_src_revert(), 1, 2, 1, 72, 72), size=(227, 149), nc=3, samp0=(2, 2), scans=1, ri=0, cs="YCbCr"),
    "s1x2": dict(make=lambda: cjpeg(testorig(), ["-revert", "-sample", "1x2"]), size=(227, 149), nc=3, samp0=(1, 2), scans=1, ri=0, cs="YCbCr"),
    "s_mixed": dict(make=lambda: cjpeg(testorig(), ["-revert", "-sample", "2x2,1x1,2x1"]), size=(227, 149), nc=3, samp0=(2, 2), scans=1, ri=0, cs="YCbCr"),
    "1x1": dict(make=lambda: cjpeg(O.synthetic_frame(1, 1, 3), ["-revert"]), size=(1, 1), nc=3, samp0=(2, 2), scans=1, ri=0, cs="YCbCr"),
    "8x8": dict(make=lambda: cjpeg(O.synthetic_frame(8, 8, 4), ["-revert"]), size=(8, 8), nc=3, samp0=(2, 2), scans=1, ri=0, cs="YCbCr"),
    "17x9": dict(make=lambda: cjpeg(O.synthetic_frame(17, 9, 5), ["-revert"]), size=(17, 9), nc=3, samp0=(2, 2), scans=1, ri=0, cs="YCbCr"),
    # (cjpeg itself selects 1x1 sampling from quality 90 upwards, rdswitch.c set_quality_ratings)
    "noise_q100": dict(make=lambda: cjpeg(noise(64, 48, 11), ["-revert", "-quality", "100"]), size=(64, 48), nc=3, samp0=(1, 1), scans=1, ri=0, cs="YCbCr"),
}


def add_fill_bytes(jpeg, info):
    """the same file with 0xFF fill bytes in front of markers (T.81 B.1.1.2): one in front of every RSTn inside the entropy-coded data,
    two in front of the marker that ends each scan; info = mozjpeg_amd.jpeg_info(jpeg).  Returns (bytes, markers padded)."""
    ranges = [(info.scans[k].data_offset, info.scans[k].data_offset + info.scans[k].data_size) for k in range(info.num_scans)]
    out, n = bytearray(), 0
    for pos, b in enumerate(jpeg):
        if b == 0xFF and pos + 1 < len(jpeg):
            c = jpeg[pos + 1]
            if 0xD0 <= c <= 0xD7 and any(a <= pos < e for a, e in ranges):
                out += b"\xff"
                n += 1
            elif any(pos == e for _, e in ranges):
                out += b"\xff\xff"
                n += 1
        out.append(b)
    return bytes(out), n


@functools.lru_cache(maxsize=None)
def oracle_source():
    """(file, coefficient taps, parameters) of the oracle's max-compression sequential encode: one DHT segment with four tables,
    trellis-quantized coefficients"""
    img = O.synthetic_frame(200, 120, 7)
    p = O.make_params(200, 120, baseline=True)
    data, taps = O.encode(p, img, want_taps=True)
    return data, taps, p


@functools.lru_cache(maxsize=None)
def source(name):
    return SOURCES[name]["make"]()


# jpegtran's switches: name -> (keywords of mozjpeg_amd.params_from_jpeg / recompress, the program's arguments)
SWITCHES = {
    "default": (dict(), []),
    "revert": (dict(revert=True), ["-revert"]),
    "revert_opt": (dict(revert=True, optimize=True), ["-revert", "-optimize"]),
    "progressive": (dict(progressive=True), ["-progressive"]),
    "fastcrush_progressive": (dict(fastcrush=True, progressive=True), ["-fastcrush", "-progressive"]),
    "revert_restart2": (dict(revert=True, restart=2), ["-revert", "-restart", "2"]),
}


@functools.lru_cache(maxsize=None)
def reference(src_name, sw_name):
    return O.ref_jpegtran(source(src_name), ["-copy", "none"] + SWITCHES[sw_name][1])


ALL_PAIRS = [(s, w) for s in SOURCES for w in SWITCHES]

# refused sources: name -> (cjpeg arguments, a word of the reason)
REFUSALS = {
    "progressive": (["-quality", "75"], "progressive"),
    "arithmetic": (["-revert", "-arithmetic"], "arithmetic"),
    "precision12": (["-revert", "-precision", "12"], "12-bit"),
    "lossless": (["-revert", "-lossless", "1"], "lossless"),
}


def run_pair(M, src_name, sw_name, max_batch=1):
    """the file (source, switches) gives: through recompress() for the default switches (prefer_smallest), else the Encoder"""
    kw = SWITCHES[sw_name][0]
    src = source(src_name)
    if sw_name == "default":
        out = M.recompress([src], max_batch=max_batch, **kw)[0]
        if isinstance(out, Exception):
            raise out
        return out
    enc = M.Encoder(M.params_from_jpeg(src, **kw), max_batch=max_batch)
    try:
        return enc.transcode_host([src])[0]
    finally:
        enc.close()
