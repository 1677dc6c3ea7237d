"""The cases and helpers of the libjpeg-decompress-API tests (test_simt_djpeg.py on the emulator, test_gpu_djpeg.py on the chip):
RGB565 through the C ABI, the unchanged djpeg binary on the stand-alone libjpeg.so.62, and tests/native/djpeg_client.c.

Every expected byte comes from the reference at test time -- oracle/_ref/djpeg, or the same client binary run with
LD_LIBRARY_PATH at oracle/_ref -- and every comparison is exact equality.  A test module hands the directory of the stand-alone
library (and what its processes need in the environment) to `Runner`."""
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle_lib as O
import decode_cases as DC
import transcode_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIENT = os.path.join(ROOT, "tests", "native", "djpeg_client")
JCS_RGB565 = 16
RGB_FAMILY = [2] + list(range(6, 16)) + [JCS_RGB565]         # JCS_RGB, the ten JCS_EXT_*, JCS_RGB565


def have_tools():
    return DC.have_tools() and os.path.exists(CLIENT) and os.path.exists(os.path.join(O.REF_DIR, "libjpeg.so.62"))


# ---- 1. RGB565 through the C ABI ------------------------------------------------------------------------------------------------
def parse_bmp24(data):
    """[H, W, 3] RGB of a 24-bit bottom-up BMP (wrbmp.c: rows padded to 4 bytes, stored B, G, R)"""
    assert data[:2] == b"BM"
    off = int.from_bytes(data[10:14], "little")
    w, h = int.from_bytes(data[18:22], "little"), int.from_bytes(data[22:26], "little")
    assert int.from_bytes(data[28:30], "little") == 24
    pitch = (w * 3 + 3) & ~3
    assert len(data) == off + pitch * h
    a = np.frombuffer(data, np.uint8, pitch * h, off).reshape(h, pitch)[::-1, :w * 3].reshape(h, w, 3)
    return np.ascontiguousarray(a[..., ::-1])


def expand565(p):
    """what wrbmp.c makes of a 565 pixel: (p >> 8) & 0xF8, (p >> 3) & 0xFC, (p << 3) & 0xF8 -- injective on the three fields"""
    p = p.astype(np.uint32)
    return np.stack([(p >> 8) & 0xF8, (p >> 3) & 0xFC, (p << 3) & 0xF8], axis=-1).astype(np.uint8)


def djpeg565_args(dither, fancy, scale=None):
    return ["-rgb565", "-bmp"] + ([] if dither else ["-dither", "none"]) + ([] if fancy else ["-nosmooth"]) + (["-scale", scale] if scale else [])


def djpeg565(jpeg, dither=True, fancy=True, scale=None):
    """the reference's djpeg -rgb565 -bmp: the expanded pixels [H, W, 3]"""
    with tempfile.TemporaryDirectory() as td:
        inp, outp = os.path.join(td, "in.jpg"), os.path.join(td, "out.bmp")
        with open(inp, "wb") as f:
            f.write(jpeg)
        subprocess.check_call([DC.DJPEG] + djpeg565_args(dither, fancy, scale) + ["-outfile", outp, inp])
        with open(outp, "rb") as f:
            return parse_bmp24(f.read())


@functools.lru_cache(maxsize=None)
def reference565(name, dither, fancy, scale=None):
    return djpeg565(DC.source(name), dither, fancy, scale)


SOURCES_565 = ["revert", "q90_2x1_r1", "s_mixed", "gray_r5b", "rgb", "17x9", "1x1", "33x47"]
MODES_565 = [(d, f) for d in (True, False) for f in (True, False)]
PAIRS_565 = [(s, d, f) for s in SOURCES_565 for d, f in MODES_565]
PAIR_IDS_565 = ["%s-%s-%s" % (s, "dither" if d else "none", "default" if f else "nosmooth") for s, d, f in PAIRS_565]
SCALED_565 = [(s, sc) for s in ("revert", "gray_r5b") for sc in ("1/2", "1/8")]


def same565(out, ref):
    return out.dtype == np.uint16 and out.shape == ref.shape[:2] and np.array_equal(expand565(out), ref)


def check_565(M, name, dither, fancy, scale=None):
    out = M.decode([DC.source(name)], color="rgb565", dither=dither, fancy_upsampling=fancy, scale=scale)[0]
    if isinstance(out, Exception):
        raise out
    ref = reference565(name, dither, fancy, scale)
    assert same565(out, ref), "%s %s, the reference %s" % (out.shape, out.dtype, ref.shape)


def check_565_batch(M):
    files = DC.batch_files()
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True), max_batch=3)
    for dither in (True, False):
        outs = enc.decode_host(files, color="rgb565", dither=dither)
        assert enc.decode_stats()["pixel_size"] == 2
        for f, o in zip(files, outs):
            assert same565(o, djpeg565(f, dither, True))
    # bottom_up: the same rows last to first (the dither row is the IMAGE row's)
    up = enc.decode_host(files[:1], color="rgb565", bottom_up=True)[0]
    assert np.array_equal(up[::-1], enc.decode_host(files[:1], color="rgb565")[0])
    enc.close()


def unclamped_rgb(M, jpeg):
    """the three sums ycc_rgb_convert puts into its range-limit table, of a 4:4:4 YCbCr file: [H, W, 3] int"""
    info = M.jpeg_info(jpeg)
    y, cb, cr = [p[:info.image_height, :info.image_width].astype(np.int64) for p in M.decode_planes([jpeg])[0]]
    cb, cr = cb - 128, cr - 128
    return np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb + 32768 - 46802 * cr) >> 16), y + ((116130 * cb + 32768) >> 16)], axis=-1)


def check_565_dither_before_clamp(M):
    """noise at quality 100: channels that leave [0, 255] before the range limit.  clamp(v + d) and clamp(clamp(v) + d) differ
    for v < 0, so the case first shows that it has such samples."""
    jpeg = DC.source("noise_q100")
    v = unclamped_rgb(M, jpeg)
    below, above = int((v < 0).sum()), int((v > 255 - 15).sum())
    assert below > 0 and above > 0, "no channel of the file leaves [0, 240] before the clamp: the case proves nothing"
    for fancy in (True, False):
        check_565(M, "noise_q100", True, fancy)
    # and the order is visible in this file: the wrong one gives other pixels somewhere
    wrong = np.clip(v, 0, 255)
    d = np.array([[(m >> (8 * x)) & 0xFF for x in range(4)] for m in (0x0008020A, 0x0C040E06, 0x030B0109, 0x0F070D05)])
    dd = d[np.arange(v.shape[0])[:, None] & 3, np.arange(v.shape[1])[None, :] & 3]
    right = np.clip(v + np.stack([dd, dd >> 1, dd], -1), 0, 255)
    wrong = np.clip(wrong + np.stack([dd, dd >> 1, dd], -1), 0, 255)
    pack = lambda a: ((a[..., 0] << 8) & 0xF800) | ((a[..., 1] << 3) & 0x7E0) | (a[..., 2] >> 3)
    assert np.array_equal(expand565(pack(right)), reference565("noise_q100", True, True))
    assert not np.array_equal(pack(right), pack(wrong))


def check_565_refusals(M):
    src = DC.source("revert")
    M._decode_encoders.clear()
    for kw in (dict(color="rgb565", pixel_size=3), dict(color="rgb565", rgb_offset=(2, 1, 0)), dict(color="rgb565", rgb_offset=(0, 1, 2)),
               dict(pixel_size=2), dict(color="rgb", pixel_size=2), dict(color="gray", pixel_size=2)):
        with pytest.raises(M.MjhError) as ei:
            M.decode([src], **kw)
        assert ei.value.code == M.EINVAL, kw
    assert not M._decode_encoders
    # the library's own checks, past the binding's
    enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=1)
    for cs, px, off in ((M.CS_RGB565, 3, (0, 0, 0)), (M.CS_RGB565, 0, (2, 1, 0)), (M.CS_RGB565, 2, (0, 1, 2)), (0, 2, (0, 0, 0)), (M.CS_RGB, 2, (0, 0, 0))):
        o = M.DecodeOpts()
        M.lib().mjh_decode_opts_defaults(o)
        o.out_color_space, o.pixel_size = cs, px
        o.rgb_offset[:] = off
        with pytest.raises(M.MjhError) as ei:
            enc.decode_host([src], opts=o)
        assert ei.value.code == M.EINVAL and ("pixel_size" in str(ei.value) or "rgb_offset" in str(ei.value)), str(ei.value)
    # a zeroed struct means what it meant: the file's default, 3-byte RGB
    assert np.array_equal(enc.decode_host([src], opts=M.DecodeOpts())[0], DC.reference("revert", "nosmooth"))
    o = M.DecodeOpts(out_color_space=M.CS_RGB565, pixel_size=2, fancy_upsampling=1)
    assert same565(enc.decode_host([src], opts=o)[0], reference565("revert", True, True))
    enc.close()


# ---- 2. / 3. processes on the two libraries ---------------------------------------------------------------------------------------
class Runner:
    """runs a binary that is linked to libjpeg.so.62 on the reference's library and on the stand-alone one"""

    def __init__(self, standalone_dir, env=None):
        self.sa = standalone_dir
        self.extra = dict(env or {})
        self.ref_cache = {}

    def env(self, ours):
        e = dict(os.environ)
        O.set_preload(e)
        e.pop("LD_DEBUG", None)
        if ours:
            e.update(self.extra)
        e["LD_LIBRARY_PATH"] = self.sa if ours else O.REF_DIR
        return e

    def run(self, ours, argv, stdin=None, cwd=None, env=None):
        e = self.env(ours)
        e.update(env or {})
        return subprocess.run(argv, env=e, stdin=stdin, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)

    def djpeg(self, ours, jpeg, args, how="file", extra_out=None):
        """(exit status, output file or None, stderr, extra output file or None) of djpeg; how: "file", "stdin" """
        with tempfile.TemporaryDirectory() as td:
            inp, outp = os.path.join(td, "in.jpg"), os.path.join(td, "out.bin")
            with open(inp, "wb") as f:
                f.write(jpeg)
            args = [a if a != "@EXTRA@" else os.path.join(td, "extra.bin") for a in args]
            if how == "stdin":
                with open(inp, "rb") as f:
                    r = self.run(ours, [DC.DJPEG] + args + ["-outfile", outp], stdin=f)
            else:
                r = self.run(ours, [DC.DJPEG] + args + ["-outfile", outp, inp])
            read = lambda p: open(p, "rb").read() if os.path.exists(p) else None
            return r.returncode, read(outp), r.stderr.replace(td.encode(), b"TD"), read(os.path.join(td, "extra.bin"))

    def client(self, ours, scenario, inputs, outputs=0, args=()):
        """(exit status, stdout, [output files]) of djpeg_client `scenario`: inputs are byte strings written to files, then come
        `outputs` output paths (a negative count: the one path is a PREFIX, -outputs files prefix.<i> are read), then args"""
        with tempfile.TemporaryDirectory() as td:
            paths = []
            for i, data in enumerate(inputs):
                paths.append(os.path.join(td, "in%d.jpg" % i))
                with open(paths[-1], "wb") as f:
                    f.write(data)
            outs = [os.path.join(td, "out%d.bin" % i) for i in range(abs(outputs) if outputs >= 0 else 1)]
            if scenario == "threads":
                argv = [CLIENT, scenario] + outs + paths
            else:
                argv = [CLIENT, scenario] + paths + outs + [str(a) for a in args]
            r = self.run(ours, argv)
            read = lambda p: open(p, "rb").read() if os.path.exists(p) else None
            files = [read(p) for p in outs] if outputs >= 0 else [read("%s.%d" % (outs[0], i)) for i in range(-outputs)]
            return r.returncode, r.stdout.decode(errors="replace") + r.stderr.decode(errors="replace").replace(td, "TD"), files

    def both_client(self, scenario, inputs, outputs=0, args=()):
        ref = self.client(False, scenario, inputs, outputs, args)
        assert ref[0] == 0, "the client on the reference's library: %d\n%s" % (ref[0], ref[1])
        out = self.client(True, scenario, inputs, outputs, args)
        assert out[1] == ref[1], "printed on the stand-alone library:\n%s\non the reference's:\n%s" % (out[1], ref[1])
        assert out[0] == 0
        for a, b in zip(out[2], ref[2]):
            assert b is not None and a == b, "an output file differs"
        return out


def com_source():
    """revert with a COM marker and an APP12 segment, which djpeg -verbose prints through its own marker processor"""
    j = DC.source("revert")
    seg = lambda code, body: bytes([0xFF, code]) + (2 + len(body)).to_bytes(2, "big") + body
    com, app12 = seg(0xFE, b"made for the djpeg test\n"), seg(0xEC, b"Ducky\x00\x01\x02ab")
    return j[:2] + com + app12 + j[2:]


def markers_source():
    """revert with COM, two APP1 segments (one longer than the 16 bytes kept) and a 2-chunk ICC profile in APP2"""
    j = DC.source("revert")
    seg = lambda code, body: bytes([0xFF, code]) + (2 + len(body)).to_bytes(2, "big") + body
    icc = bytes(np.random.default_rng(12).integers(0, 256, 3000, dtype=np.uint8))
    parts = [icc[:1700], icc[1700:]]
    extra = seg(0xFE, b"first comment") + seg(0xE1, b"Exif\x00\x00" + bytes(range(40))) + seg(0xE1, b"short")
    extra += b"".join(seg(0xE2, b"ICC_PROFILE\x00" + bytes([i + 1, 2]) + p) for i, p in enumerate(parts)) + seg(0xFE, b"")
    return j[:2] + extra + j[2:]


def icc_source():
    """a file made by the reference's cjpeg -icc from a 3000-byte blob, and the blob"""
    icc = bytes(np.random.default_rng(7).integers(0, 256, 3000, dtype=np.uint8))
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "p.icc")
        with open(p, "wb") as f:
            f.write(icc)
        return TC.cjpeg(TC.testorig()[:64, :80], ["-revert", "-icc", p]), icc


DJPEG_SOURCES = ["revert", "gray_r5b", "q90_2x1_r1"]
DJPEG_SWITCHES = {
    "ppm": [], "grayscale": ["-grayscale"], "rgb": ["-rgb"], "nosmooth": ["-nosmooth"], "dctfast": ["-dct", "fast"],
    "scale2": ["-scale", "1/2"], "scale4": ["-scale", "1/4"], "scale8": ["-scale", "1/8"], "bmp": ["-bmp"], "targa": ["-targa"],
    "rgb565": ["-rgb565", "-bmp"], "rgb565_none": ["-rgb565", "-bmp", "-dither", "none"], "memsrc": ["-memsrc"],
    "nosmooth_scale2": ["-nosmooth", "-scale", "1/2"],
}
DJPEG_PAIRS = [(s, k) for s in DJPEG_SOURCES for k in DJPEG_SWITCHES]
DJPEG_REFUSED = {
    "gif": (["-gif"], "quantization"), "colors": (["-colors", "64"], "quantization"), "scale3_8": (["-scale", "3/8"], "3x3"),
    "crop": (["-crop", "16x16+8+8"], "jpeg_crop_scanline"), "skip": (["-skip", "1,2"], "jpeg_skip_scanlines"), "dctfloat": (["-dct", "float"], "float"),
}


def _named_source(name):
    if name == "com":
        return com_source()
    if name == "icc":
        return icc_source()[0]
    return DC.source(name)


def check_djpeg(R, name, switches, how="file", stderr=False):
    """the unchanged djpeg on the stand-alone library == on the reference's: output file, exit status and (on request) stderr"""
    key = (name, tuple(switches), how)
    if key not in R.ref_cache:                            # (the reference's run is shared by the tests that need it)
        R.ref_cache[key] = R.djpeg(False, _named_source(name), list(switches), how)
    ref = R.ref_cache[key]
    assert ref[0] == 0 and ref[1], "the reference's djpeg: %d %s" % (ref[0], ref[2][-500:])
    out = R.djpeg(True, _named_source(name), list(switches), how)
    assert out[0] == ref[0], "exit status %d, the reference %d\n%s" % (out[0], ref[0], out[2].decode(errors="replace")[-2000:])
    assert out[1] == ref[1], "the output file differs"
    assert out[3] == ref[3], "the second output file differs"
    if stderr:
        assert out[2] == ref[2], "stderr:\n%s\nthe reference's:\n%s" % (out[2].decode(errors="replace"), ref[2].decode(errors="replace"))
    return out


def check_djpeg_refused(R, jpeg, switches, word):
    out = R.djpeg(True, jpeg, switches)
    text = out[2].decode(errors="replace")
    assert out[0] == 1, "exit status %d\n%s" % (out[0], text)
    assert "mozjpeg_hip:" in text and word in text, text
    assert "omitted at compile time" in text, text          # JERR_NOT_COMPILED through the client's error manager


# ---- 3. the client ------------------------------------------------------------------------------------------------------------------
FIELD_CASES = {      # name -> (source, scale_denom, fancy, out_cs)
    "ycc420": ("revert", 1, 1, -1), "gray": ("gray_r5b", 1, 1, -1), "rgb_adobe": ("rgb", 1, 1, -1), "restart": ("q90_2x1_r1", 1, 1, -1),
    "ycc420_merged": ("revert", 1, 0, -1), "h2v1_merged_565": ("q90_2x1_r1", 1, 0, JCS_RGB565), "ycc420_half_nosmooth": ("revert", 2, 0, -1),
    "ycc420_eighth": ("revert", 8, 1, 1), "gray_to_bgrx": ("gray_r5b", 4, 1, 9), "jfif102": ("jfif102", 1, 1, 12),
}


def check_fields(R, case):
    src, denom, fancy, cs = FIELD_CASES[case]
    R.both_client("fields", [DC.source(src)], 0, (denom, fancy, cs))


def check_rows_per_call(R, name):
    """the pixels are the same however many rows a call asks for (the 8-bit layouts)"""
    jpeg = DC.source(name)
    ref = R.client(False, "pixels", [jpeg], 1, (-1, 1, 1))
    assert ref[0] == 0
    for rows in (1, 3, 0):
        out = R.client(True, "pixels", [jpeg], 1, (-1, rows, 1))
        assert out[0] == 0 and out[1] == ref[1] and out[2][0] == ref[2][0], "%d rows per call" % rows


def damaged_sources():
    """revert truncated in the middle of its entropy-coded data, and revert with one bit flipped there: the first of the seeded
    flips of test_simt_decode.py on which the reference's djpeg warns (those are the ones the device decoder fails)"""
    import random
    import mozjpeg_amd as M
    src = DC.source("revert")
    info = M.jpeg_info(src)
    a, n = info.scans[0].data_offset, info.scans[0].data_size
    rng = random.Random(20240607)
    for _ in range(200):
        pos, bit = a + rng.randrange(n), rng.randrange(8)
        bad = bytearray(src)
        bad[pos] ^= 1 << bit
        if DC.djpeg_status(bytes(bad))[0] == 2:
            return src[:a + n // 2], bytes(bad)
    raise AssertionError("no flip the reference warns on")


def check_damaged(R):
    cut, flipped = damaged_sources()
    for jpeg, text in ((cut, "Premature end of input file"), (flipped, "Corrupt JPEG data: bad Huffman code")):
        rc, out, _ = R.client(True, "damaged", [jpeg])
        assert rc == 1, out
        assert "error_exit code=" in out and text in out, out
        assert "0 rows were delivered, 0 bytes of the client's buffer and its guard changed" in out, out
        assert "mozjpeg_hip:" in out, out
