"""The case list and helpers of the pixel-decoder tests (test_simt_decode.py on the emulator, test_gpu_decode.py on the chip).

Sources are transcode_cases.SOURCES plus files made at test time by the reference's cjpeg that reach the remaining upsamplers;
the expected pixels always come from the reference's djpeg (oracle/_ref/djpeg -pnm ...) at test time, and every comparison is
exact equality with its PPM / PGM payload."""
import functools
import os
import subprocess
import tempfile

import numpy as np

import oracle_lib as O
import transcode_cases as TC

DJPEG = os.path.join(O.REF_DIR, "djpeg")


def have_tools():
    return TC.have_tools() and os.path.exists(DJPEG)


def parse_pnm(data):
    """[H, W] (P5) or [H, W, 3] (P6) uint8 array of a binary PNM file with maxval 255"""
    fields, pos = [], 0
    while len(fields) < 4:
        while data[pos:pos + 1].isspace():
            pos += 1
        if data[pos:pos + 1] == b"#":
            pos = data.index(b"\n", pos) + 1
            continue
        end = pos
        while not data[end:end + 1].isspace():
            end += 1
        fields.append(data[pos:end])
        pos = end
    pos += 1                                            # the single whitespace byte behind maxval
    magic, w, h, maxval = fields[0], int(fields[1]), int(fields[2]), int(fields[3])
    assert magic in (b"P5", b"P6") and maxval == 255
    c = 3 if magic == b"P6" else 1
    a = np.frombuffer(data, np.uint8, w * h * c, pos)
    assert len(data) == pos + w * h * c
    return a.reshape((h, w, 3) if c == 3 else (h, w))


def djpeg_status(jpeg, args=()):
    """(exit status, pixels or None) of the reference's djpeg -pnm: 0 = clean, 2 = warnings, 1 = error"""
    with tempfile.TemporaryDirectory() as td:
        inp, outp = os.path.join(td, "in.jpg"), os.path.join(td, "out.pnm")
        with open(inp, "wb") as f:
            f.write(jpeg)
        r = subprocess.run([DJPEG, "-pnm"] + list(args) + ["-outfile", outp, inp], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        pix = None
        if r.returncode != 1 and os.path.exists(outp):
            with open(outp, "rb") as f:
                data = f.read()
            try:
                pix = parse_pnm(data)
            except Exception:
                pix = None
        return r.returncode, pix


def djpeg(jpeg, args=()):
    status, pix = djpeg_status(jpeg, args)
    assert status == 0 and pix is not None, "djpeg exited with %d" % status
    return pix


# djpeg's switches: name -> (keywords of mozjpeg_amd.decode / decode_opts, the program's arguments)
MODES = {
    "default": (dict(), []),
    "nosmooth": (dict(fancy_upsampling=False), ["-nosmooth"]),
    "grayscale": (dict(color="gray"), ["-grayscale"]),
    "rgb": (dict(color="rgb"), ["-rgb"]),
}

# sources beyond transcode_cases.SOURCES: the upsamplers those do not reach, and sizes of 16 k + 1 and 16 k + 15
EXTRA = {
    "s4x1": lambda: TC.cjpeg(TC.testorig(), ["-revert", "-sample", "4x1"]),
    "s1x4": lambda: TC.cjpeg(TC.testorig(), ["-revert", "-sample", "1x4"]),
    "s_h1v2_h2v1": lambda: TC.cjpeg(TC.testorig(), ["-revert", "-sample", "2x2,2x1,1x2"]),
    "33x47": lambda: TC.cjpeg(O.synthetic_frame(33, 47, 21), ["-revert"]),
    "47x33_2x1": lambda: TC.cjpeg(O.synthetic_frame(47, 33, 22), ["-revert", "-sample", "2x1"]),
}
NAMES = list(TC.SOURCES) + list(EXTRA)
ALL_PAIRS = [(s, m) for s in NAMES for m in MODES]


@functools.lru_cache(maxsize=None)
def source(name):
    return TC.source(name) if name in TC.SOURCES else EXTRA[name]()


@functools.lru_cache(maxsize=None)
def reference(name, mode):
    return djpeg(source(name), MODES[mode][1])


def upsamplers(info, mode, CS_GRAYSCALE=1, CS_YCBCR=3):
    """the upsampling functions jinit_upsampler (jdsample.c:444-525) picks for a file under a mode, from its factors and width"""
    nc = info.num_components
    fancy = mode != "nosmooth"
    maxh = max(info.h_samp_factor[c] for c in range(nc))
    maxv = max(info.v_samp_factor[c] for c in range(nc))
    needed = range(nc)
    if mode == "grayscale" and info.jpeg_color_space in (CS_GRAYSCALE, CS_YCBCR):
        needed = [0]                                    # component_needed: Y alone
    used = set()
    for c in needed:
        h, v = info.h_samp_factor[c], info.v_samp_factor[c]
        dw = -(-info.image_width * h // maxh)
        if h == maxh and v == maxv:
            used.add("fullsize_upsample")
        elif h * 2 == maxh and v == maxv:
            used.add("h2v1_fancy_upsample" if fancy and dw > 2 else "h2v1_upsample")
        elif h == maxh and v * 2 == maxv and fancy:
            used.add("h1v2_fancy_upsample")
        elif h * 2 == maxh and v * 2 == maxv:
            used.add("h2v2_fancy_upsample" if fancy and dw > 2 else "h2v2_upsample")
        else:
            assert maxh % h == 0 and maxv % v == 0
            used.add("int_upsample")
    return used


ALL_UPSAMPLERS = {"fullsize_upsample", "h2v1_upsample", "h2v2_upsample", "h2v1_fancy_upsample", "h1v2_fancy_upsample",
                  "h2v2_fancy_upsample", "int_upsample"}


def run_pair(M, name, mode, max_batch=1):
    out = M.decode([source(name)], max_batch=max_batch, **MODES[mode][0])[0]
    if isinstance(out, Exception):
        raise out
    return out


def patch_dqt(jpeg, value):
    """the same file with every entry of every 8-bit DQT table set to `value`: it still parses, its coefficients now stand for
    samples far outside the clamp region of the post-IDCT range-limit table"""
    out = bytearray(jpeg)
    pos, n = 2, 0
    while pos + 4 <= len(out) and out[pos] == 0xFF and out[pos + 1] != 0xDA:
        length = (out[pos + 2] << 8) | out[pos + 3]
        if out[pos + 1] == 0xDB:
            q = pos + 4
            while q < pos + 2 + length:
                assert out[q] >> 4 == 0, "a 16-bit table"
                out[q + 1:q + 65] = bytes([value]) * 64
                q += 65
                n += 1
        pos += 2 + length
    assert n > 0
    return bytes(out)


ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])


def _idct_1d(x):
    """the 1-D inverse transform of the slow integer IDCT along the last axis of an int64 array: the sums in front of the shift"""
    x = x.astype(np.int64)
    z2, z3 = x[..., 2], x[..., 6]
    z1 = (z2 + z3) * 4433
    t2, t3 = z1 - z3 * 15137, z1 + z2 * 6270
    t0, t1 = (x[..., 0] + x[..., 4]) << 13, (x[..., 0] - x[..., 4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = x[..., 7], x[..., 5], x[..., 3], x[..., 1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    return np.stack([t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3], axis=-1)


def idct_unclamped(coef_zz, quant_nat):
    """coef_zz: [64 zig-zag][blocks] int16 (mjh TAP_COEF_Q), quant_nat: 64 steps in natural order.  Returns [blocks, 8, 8] int64:
    the values the slow integer IDCT indexes its range-limit table with, BEFORE the & 1023 (sample - 128, unclamped)."""
    nat = np.zeros((coef_zz.shape[1], 64), np.int64)
    nat[:, ZIGZAG] = coef_zz.T.astype(np.int64)
    blk = (nat * np.asarray(quant_nat, np.int64)[None, :]).reshape(-1, 8, 8)
    ws = (_idct_1d(blk.transpose(0, 2, 1)) + 1024) >> 11          # pass 1 runs down the columns
    ws = ws.astype(np.int32).astype(np.int64).transpose(0, 2, 1)   # (the workspace is int)
    return (_idct_1d(ws) + (1 << 17)) >> 18


def batch_files():
    """three files of one signature with different Huffman tables, restart intervals and densities"""
    img = TC.testorig()
    return [TC.patch_jfif(TC.cjpeg(img, ["-revert"]), 1, 2, 1, 72, 72),
            TC.cjpeg(img[::-1].copy(), ["-revert", "-optimize", "-restart", "1"]),
            TC.patch_jfif(TC.cjpeg(np.roll(img, 40, axis=1), ["-revert", "-optimize", "-restart", "7B"]), 1, 1, 2, 300, 150)]


def wrap_source():
    """a noisy quality-50 file whose quantization steps were all set to 255 after encoding"""
    return patch_dqt(TC.cjpeg(TC.noise(48, 40, 31), ["-revert", "-quality", "50", "-sample", "2x2"]), 255)


def wrapped_samples(M, enc, jpeg):
    """how many samples of the file's components land in the wrapped part of the post-IDCT range-limit table (outside
    [-512, 511] before the mask), from the coefficients enc decoded last and a NumPy restatement of the transform"""
    info = M.jpeg_info(jpeg)
    total = 0
    for c in range(info.num_components):
        v = idct_unclamped(enc.read_tap(M.TAP_COEF_Q, 0, c), list(info.quantval[info.quant_tbl_no[c]]))
        total += int(((v < -512) | (v > 511)).sum())
    return total


LAYOUT_ORDER = {"bgr": (2, 1, 0), "rgbx": (0, 1, 2), "bgrx": (2, 1, 0), "xbgr": (3, 2, 1), "xrgb": (1, 2, 3)}


def check_layout(rgb, out, layout):
    """out == the RGB result permuted into `layout`, filler 0xFF"""
    off = LAYOUT_ORDER[layout]
    px = 4 if "x" in layout else 3
    assert out.shape == rgb.shape[:2] + (px,)
    for k in range(3):
        assert np.array_equal(out[..., off[k]], rgb[..., k]), "%s: colour %d" % (layout, k)
    if px == 4:
        fill = ({0, 1, 2, 3} - set(off)).pop()
        assert (out[..., fill] == 0xFF).all(), "%s: filler" % layout
