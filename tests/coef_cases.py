"""The case list and helpers of the coefficient-reading tests (test_simt_coefs.py on the emulator, test_gpu_coefs.py on the chip):
mozjpeg_amd.decode_coefficients through the C ABI (mjh_decode_opts.raw_coefs, k_export_coefs), jpeg_read_coefficients of the
stand-alone libjpeg.so.62, and the reference's unchanged jpegtran on that library alone.

Every expected value comes from the reference at test time: tests/native/coef_dump (a client of jpeg_read_coefficients) and
oracle/_ref/jpegtran run with LD_LIBRARY_PATH at oracle/_ref.  Every comparison is exact equality.  A test module hands the directory
of the stand-alone library to djpeg_cases.Runner."""
import functools
import os
import subprocess
import tempfile

import numpy as np

import oracle_lib as O
import decode_cases as DC
import djpeg_cases as DJ
import transcode_cases as TC
import jpeg_writer as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COEF_DUMP = os.path.join(ROOT, "tests", "native", "coef_dump")

# 227x149 4:2:0 (partial iMCU in both directions, width in blocks != padded width); a restart every MCU; gray with restarts in
# blocks; non-interleaved; 4:4:4 RGB; every other sampling the decoder tests use; the smallest sizes; noise at quality 100 (large
# values); and a file with AC values beyond +-1023
SOURCES = ["revert", "q90_2x1_r1", "gray_r5b", "scans3_2x2_r2", "rgb", "s1x2", "s_mixed", "s4x1", "s_h1v2_h2v1", "1x1", "8x8", "17x9",
           "noise_q100", "big_ac"]


def have_tools():
    return DJ.have_tools() and os.path.exists(COEF_DUMP)


@functools.lru_cache(maxsize=None)
def big_ac_source():
    """a 40 x 24 4:2:2 file of tests/jpeg_writer.py with AC values up to +-16383 and DC values up to +-2047: none of the large ones
    could be coded again (jchuff.c refuses beyond +-1023), every one has a Huffman symbol and reads back as it is"""
    comps = [(1, 2, 1, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
    rng = np.random.default_rng(77)
    coefs = []
    for ci in range(3):
        rows, cols = W.padded_blocks(40, 24, comps, ci)
        a = rng.integers(-3, 4, (rows, cols, 64)) * (rng.random((rows, cols, 64)) < 0.2)
        a[..., 0] = rng.integers(-2047, 2048, (rows, cols))
        big = rng.random((rows, cols, 64)) < 0.03
        big[..., 0] = False
        a[big] = rng.choice([1024, -1024, 1500, -2047, 4095, -8000, 16383, -16383], int(big.sum()))
        coefs.append(a)
    q = {0: (0, [1] * 64), 1: (0, [2] * 64)}
    data, _ = W.write_jpeg(40, 24, comps, coefs, q, [dict(comps=[0, 1, 2], dc=[0, 1, 1], ac=[0, 1, 1], ri=0, shape="optimal")])
    return data


@functools.lru_cache(maxsize=None)
def source(name):
    return big_ac_source() if name == "big_ac" else DC.source(name)


def parse_dump(data):
    """coef_dump's file: per component two uint32 (blocks across, blocks down) and the real blocks -> [int16 [down, across, 64], ...]"""
    out, pos = [], 0
    while pos < len(data):
        w, h = np.frombuffer(data, np.uint32, 2, pos)
        pos += 8
        n = int(w) * int(h) * 64
        out.append(np.frombuffer(data, np.int16, n, pos).reshape(int(h), int(w), 64).copy())
        pos += n * 2
    assert pos == len(data)
    return out


def run_dump(libdir, argv, env=None):
    """(exit status, printed text, output file or None) of coef_dump with LD_LIBRARY_PATH at libdir; "@OUT@" in argv names the file"""
    with tempfile.TemporaryDirectory() as td:
        outp = os.path.join(td, "out.bin")
        e = dict(os.environ)
        O.set_preload(e)
        e.update(env or {})
        e["LD_LIBRARY_PATH"] = libdir
        r = subprocess.run([COEF_DUMP] + [outp if a == "@OUT@" else a for a in argv], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        data = open(outp, "rb").read() if os.path.exists(outp) else None
        return r.returncode, r.stdout.decode(errors="replace") + r.stderr.decode(errors="replace").replace(td, "TD"), data


def dump_files(libdir, scenario, files, extra=(), env=None, out=True):
    """coef_dump `scenario` on byte strings written to files"""
    with tempfile.TemporaryDirectory() as td:
        paths = []
        for i, f in enumerate(files):
            paths.append(os.path.join(td, "in%d.jpg" % i))
            with open(paths[-1], "wb") as fh:
                fh.write(f)
        rc, text, data = run_dump(libdir, [scenario] + paths + (["@OUT@"] if out else []) + list(extra), env)
        return rc, text.replace(td, "TD"), data


@functools.lru_cache(maxsize=None)
def reference(name):
    """the reference's coefficient arrays of a source: jpeg_read_coefficients of oracle/_ref/libjpeg.so.62"""
    rc, text, data = dump_files(O.REF_DIR, "dump", [source(name)])
    assert rc == 0 and data, "coef_dump on the reference's library: %d\n%s" % (rc, text)
    return parse_dump(data)


def same_arrays(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == np.int16 and y.dtype == np.int16 and np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------------
def check_parity(M, name):
    out = M.decode_coefficients([source(name)])[0]
    if isinstance(out, Exception):
        raise out
    ref = reference(name)
    assert same_arrays(out, ref), "%s, the reference %s" % ([a.shape for a in out], [a.shape for a in ref])
    if name == "big_ac":
        assert max(int(np.abs(a[..., 1:]).max()) for a in ref) == 16383        # the case is what it says


def both(R, scenario, files, extra=(), out=True):
    """the scenario on both libraries: same exit status, same text, same file"""
    ref = dump_files(O.REF_DIR, scenario, files, extra, out=out)
    ours = dump_files(R.sa, scenario, files, extra, env=R.extra, out=out)
    assert ours[1] == ref[1], "printed on the stand-alone library:\n%s\non the reference's:\n%s" % (ours[1], ref[1])
    assert ours[0] == ref[0], "exit status %d, the reference's %d" % (ours[0], ref[0])
    assert ours[2] == ref[2], "the output file differs"
    return ref


def check_dump_parity(R, name):
    ref = both(R, "dump", [source(name)], ["fields"])
    assert ref[0] == 0 and "after jpeg_read_coefficients" in ref[1]


# ---- 2. batching --------------------------------------------------------------------------------------------------------------------
def damaged():
    src = source("revert")
    info_a, info_n = scan0(src)
    return src[:info_a + info_n // 2] + src[info_a + info_n // 2 + 40:]          # 40 bytes of entropy data missing, every marker in place


def scan0(jpeg):
    import mozjpeg_amd as M
    info = M.jpeg_info(jpeg)
    return info.scans[0].data_offset, info.scans[0].data_size


def check_mixed_batch(M):
    names = ["revert", "gray_r5b", "8x8", "revert_opt", "rgb", "17x9", "s1x2", "1x1", "noise_q100", "scans3_2x2_r2", "revert", "s4x1", "big_ac"]
    files = [source(n) if n != "revert_opt" else TC.source("revert_opt") for n in names]
    prog = TC.cjpeg(TC.testorig(), ["-quality", "75"])
    files = files[:3] + [damaged()] + files[3:7] + [prog] + files[7:]
    names = names[:3] + [None] + names[3:7] + [None] + names[7:]
    outs = M.decode_coefficients(files, max_batch=4)
    assert len(outs) == len(files)
    for i, (n, o) in enumerate(zip(names, outs)):
        if n is None:
            assert isinstance(o, M.MjhError), i
            continue
        ref = reference(n) if n != "revert_opt" else reference("revert")          # (-optimize changes the tables, not the coefficients)
        assert not isinstance(o, Exception), "%s: %s" % (n, o)
        assert same_arrays(o, ref), n
    assert outs[3].code == M.EINVAL and "Corrupt" in str(outs[3])
    assert outs[8].code == M.EUNSUPPORTED and "progressive" in str(outs[8])


def check_alternating_calls(M):
    """a pixel call, a raw_coefs call, a raw_planes call on one encoder: every getter of the wrong kind is MJH_EINVAL"""
    src = source("revert")
    enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=2)
    L = M.lib()
    buf = np.empty(1 << 20, np.uint8)
    for _ in range(2):
        pix = enc.decode_host([src])[0]
        assert np.array_equal(pix, DC.reference("revert", "default"))
        assert L.mjh_get_coefs(enc._h, 0, 0, buf.ctypes.data, 64) == M.EINVAL
        assert L.mjh_get_coefs_device(enc._h, 0, None, None, None, None, None) == M.EINVAL
        co = enc.decode_host([src, src], coefficients=True)
        assert same_arrays(co[0], reference("revert")) and same_arrays(co[1], reference("revert"))
        assert enc.transcode_status(1)[0] == M.OK
        assert L.mjh_get_pixels(enc._h, 0, buf.ctypes.data, 4096) == M.EINVAL
        assert L.mjh_get_pixels_device(enc._h, None, None, None) == M.EINVAL
        assert L.mjh_get_plane(enc._h, 0, 0, buf.ctypes.data, 4096, 8, 8) == M.EINVAL
        assert L.mjh_get_planes_device(enc._h, 0, None, None, None, None, None) == M.EINVAL
        assert L.mjh_get_coefs_device(enc._h, 0, None, None, None, None, None) == M.OK        # any pointer may be NULL
        assert L.mjh_get_coefs(enc._h, 0, 0, buf.ctypes.data, 3) == M.EINVAL                  # a pitch below the width
        assert L.mjh_get_coefs(enc._h, 2, 0, buf.ctypes.data, 64) == M.EINVAL and L.mjh_get_coefs(enc._h, 0, 3, buf.ctypes.data, 64) == M.EINVAL
        base, stride, bpr, hib, wib = enc.coefficients_device(1)
        assert (bpr, hib, wib) == (15, 10, 15) and stride == hib * bpr * 128 and base
        assert enc.coefficients_device(0)[2:] == (30, 19, 29)                                 # 227 x 149: 29 blocks across, padded to 30
        # the caller's pitch: the real blocks land at it, nothing else is written
        wide = np.full((19, 40, 64), 0x5A5A, np.int16)
        assert L.mjh_get_coefs(enc._h, 0, 0, wide.ctypes.data, 40) == M.OK
        assert np.array_equal(wide[:, :29], reference("revert")[0]) and (wide[:, 29:] == 0x5A5A).all()
        pl = enc.decode_host([src], raw_planes=True)[0]
        assert len(pl) == 3
        assert L.mjh_get_coefs(enc._h, 0, 0, buf.ctypes.data, 64) == M.EINVAL
    # the options a raw_coefs call ignores, raw_planes among them; and a zeroed struct with raw_coefs alone
    o = M.decode_opts(color="gray", scale="1/8", dct="fast", fancy_upsampling=False, bottom_up=True, raw_planes=True, raw_coefs=True)
    assert same_arrays(enc.decode_host([src], opts=o)[0], reference("revert"))
    o = M.DecodeOpts(raw_coefs=1, dct_method=7, scale_num=3, scale_denom=8)
    assert same_arrays(enc.decode_host([src], opts=o)[0], reference("revert"))
    # a lossless transform on the encoder stays refused
    enc.close()
    enc = M.Encoder(M.params_from_jpeg(src, revert=True, transform="flip_h"), max_batch=1)
    try:
        enc.decode_host([src], coefficients=True)
        raise AssertionError("a transform together with raw_coefs was accepted")
    except M.MjhError as exc:
        assert exc.code == M.EUNSUPPORTED and "transform" in str(exc)
    enc.close()


def check_stale_buffer(M):
    """a batch of two, then a batch of one damaged file and one good one in the other order: the damaged file's slot holds zeros,
    not the batch before"""
    src, bad = source("revert"), damaged()
    enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=2)
    enc.decode_host([src, src], coefficients=True)
    res = enc.decode_host([bad, src], coefficients=True, errors="return")
    assert isinstance(res[0], M.MjhError) and res[0].code == M.EINVAL and res[1] is None
    return enc                          # (the device test looks at the buffer)


def check_profiling(M):
    src = source("revert")
    enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=1)
    enc.decode_host([src], coefficients=True)
    assert enc.transcode_stats()["ms"]["export"] == 0.0
    enc.set_profiling(1)
    enc.decode_host([src], coefficients=True)
    st = enc.transcode_stats()
    assert list(st["ms"]) == ["sync", "prefix", "store", "dc", "export"]          # appended behind the decoder's phases
    assert st["ms"]["export"] > 0.0 and st["ms"]["store"] > 0.0
    enc.decode_host([src])
    assert list(enc.transcode_stats()["ms"]) == ["sync", "prefix", "store", "dc"]    # a pixel call reports what it always did
    enc.close()


# ---- 3. round trip ------------------------------------------------------------------------------------------------------------------
ROUND_TRIP = [(s, w) for s in ("revert", "q90_2x1_r1", "gray_r5b", "scans3_2x2_r2", "rgb", "17x9", "noise_q100") for w in TC.SWITCHES]


def check_round_trip(M, src_name, sw_name):
    src = TC.source(src_name)
    co = M.decode_coefficients([src])[0]
    enc = M.Encoder(M.params_from_jpeg(src, **TC.SWITCHES[sw_name][0]), max_batch=1)
    try:
        out = enc.encode_coefficients_host(co)[0]
    finally:
        enc.close()
    if sw_name == "default" and len(src) < len(out):
        out = src                       # jpegtran's default gives the source back when recoding did not shrink it (as recompress() does)
    assert out == TC.reference(src_name, sw_name)


def check_big_ac_is_refused_by_the_encoder(M):
    src = source("big_ac")
    co = M.decode_coefficients([src])[0]
    enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=1)
    try:
        enc.encode_coefficients_host(co)
        raise AssertionError("values beyond +-1023 were coded")
    except M.MjhError as exc:
        assert "coefficient" in str(exc).lower()
    finally:
        enc.close()


# ---- 4. the unchanged jpegtran on the stand-alone library alone ------------------------------------------------------------------------
JPEGTRAN_CASES = {
    "copy_none": ("revert", ["-copy", "none"]), "optimize": ("revert", ["-copy", "none", "-optimize"]),
    "progressive": ("revert", ["-copy", "none", "-progressive"]), "restart2": ("q90_2x1_r1", ["-copy", "none", "-restart", "2"]),
    "rot90_trim": ("revert", ["-copy", "none", "-rotate", "90", "-trim"]), "flip_h": ("revert", ["-copy", "none", "-flip", "horizontal"]),
    "transpose": ("s_mixed", ["-copy", "none", "-transpose"]), "crop": ("revert", ["-copy", "none", "-crop", "100x80+17+9"]),
    "grayscale": ("scans3_2x2_r2", ["-copy", "none", "-grayscale"]), "copy_all_com": ("com", ["-copy", "all"]), "copy_all_icc": ("icc", ["-copy", "all"]),
    "crop_extend": ("revert", ["-copy", "none", "-crop", "300x80+0+0"]), "wipe": ("revert", ["-copy", "none", "-wipe", "32x32+16+16"]),
    "drop": ("revert", ["-copy", "none", "-drop", "+16+16", "@DROP@"]),
}


def _jt_source(name):
    if name == "com":
        return DJ.com_source()
    if name == "icc":
        return DJ.icc_source()[0]
    return source(name)


def jpegtran(R, ours, jpeg, args):
    """(exit status, output file or None, stderr) of the reference's jpegtran binary on one of the two libraries"""
    with tempfile.TemporaryDirectory() as td:
        inp, outp, drop = os.path.join(td, "in.jpg"), os.path.join(td, "out.jpg"), os.path.join(td, "drop.jpg")
        with open(inp, "wb") as f:
            f.write(jpeg)
        with open(drop, "wb") as f:
            f.write(TC.cjpeg(TC.testorig()[40:88, 60:124], ["-revert"]))           # 64 x 48, the source's sampling and tables
        r = R.run(ours, [TC.JPEGTRAN] + [drop if a == "@DROP@" else a for a in args] + ["-outfile", outp, inp])
        data = open(outp, "rb").read() if os.path.exists(outp) else None
        return r.returncode, data, r.stderr.decode(errors="replace").replace(td, "TD")


def check_jpegtran(R, case):
    name, args = JPEGTRAN_CASES[case]
    ref = jpegtran(R, False, _jt_source(name), args)
    assert ref[0] == 0 and ref[1], "the reference's jpegtran: %d %s" % (ref[0], ref[2][-500:])
    out = jpegtran(R, True, _jt_source(name), args)
    assert out[0] == ref[0], "exit status %d, the reference %d\n%s" % (out[0], ref[0], out[2][-2000:])
    assert out[1] == ref[1], "the output file differs (%s bytes, the reference %d)" % (out[1] and len(out[1]), len(ref[1]))


def check_jpegtran_refuses_progressive(R):
    out = jpegtran(R, True, TC.cjpeg(TC.testorig(), ["-quality", "75"]), ["-copy", "none"])
    assert out[0] == 1, "exit status %d\n%s" % (out[0], out[2])
    assert "mozjpeg_hip:" in out[2] and "omitted at compile time" in out[2], out[2]


# ---- 5. API scenarios -----------------------------------------------------------------------------------------------------------------
def check_two_files(R):
    ref = both(R, "two", [source("revert"), source("gray_r5b")])
    arrays = parse_dump(ref[2])
    assert same_arrays(arrays[:3], reference("revert")) and same_arrays(arrays[3:], reference("gray_r5b"))


def check_abbreviated(R):
    with tempfile.TemporaryDirectory() as td:
        t, i = os.path.join(td, "tables.jpg"), os.path.join(td, "image.jpg")
        r = R.run(False, [DJ.CLIENT, "mkabbrev", t, i])
        assert r.returncode == 0, r.stderr
        tables, image = open(t, "rb").read(), open(i, "rb").read()
    ref = both(R, "abbrev", [tables, image])
    assert ref[0] == 0 and "tables: jpeg_read_header returned 2" in ref[1]


def check_bad_state(R):
    ref = both(R, "badstate", [source("revert")], out=False)
    assert ref[0] == 1 and "Improper call to JPEG library in state" in ref[1]


def check_abort_then_reuse(R):
    ref = both(R, "abort", [source("q90_2x1_r1"), source("revert")])
    assert ref[0] == 0 and same_arrays(parse_dump(ref[2]), reference("revert"))


def check_zero_ac_and_write(R):
    ref = both(R, "zeroac", [source("revert")])
    assert ref[0] == 0 and ref[2][:2] == b"\xff\xd8"


# ---- 6. untrusted input ---------------------------------------------------------------------------------------------------------------
def check_truncated(M, step=97):
    src = source("revert")
    a, n = scan0(src)
    enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=1)
    cuts = list(range(a, a + n, step))
    for cut in cuts:
        for tail in (b"", b"\xff\xd9"):
            try:
                enc.decode_host([src[:cut] + tail], coefficients=True)
                raise AssertionError("a file cut at %d decoded" % cut)
            except M.MjhError as exc:
                assert exc.code == M.EINVAL
    assert same_arrays(enc.decode_host([src], coefficients=True)[0], reference("revert"))
    enc.close()
    return len(cuts)


def check_bit_flips(M, count=200):
    """the seeded flips of test_simt_transcode.py (same seed, same source).  What the case is for is the kernels' bounds: every
    flipped file runs on the emulator, whose device buffers end at unmapped pages, and must end in one of two ways -- MJH_EINVAL
    with the status set, or arrays.  Arrays are compared with the reference's wherever the reference reads the same bytes without a
    warning; where it warns it has substituted values of its own for the damaged part (zeros, a resynchronised DC), which no
    decoder is asked to reproduce, so those files are not compared.  The lower bound on compared files only keeps the case from
    passing empty: a flip inside entropy-coded data usually still decodes to a full scan (test_simt_decode.py measured 170 of these
    200 decoding to the reference's pixels and 30 failing), and half of the flips is far below that."""
    import random
    src = source("revert")
    a, n = scan0(src)
    rng = random.Random(20240607)
    enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=1)
    equal = failed = 0
    for _ in range(count):
        pos, bit = a + rng.randrange(n), rng.randrange(8)
        bad = bytearray(src)
        bad[pos] ^= 1 << bit
        bad = bytes(bad)
        try:
            out = enc.decode_host([bad], coefficients=True)[0]
        except M.MjhError as exc:
            assert exc.code == M.EINVAL
            failed += 1
            continue
        rc, text, data = dump_files(O.REF_DIR, "dump", [bad])
        if rc == 0 and "Corrupt" not in text and "Premature" not in text:
            assert same_arrays(out, parse_dump(data)), "flip of bit %d at %d" % (bit, pos)
            equal += 1
    print("bit flips: %d equal, %d failed" % (equal, failed))
    assert equal >= count // 2, "%d of %d flips gave the reference's arrays, %d failed" % (equal, count, failed)
    assert same_arrays(enc.decode_host([src], coefficients=True)[0], reference("revert"))
    enc.close()
