"""The cases and checkers of the four-component decode tests (Adobe-style CMYK and YCCK files): test_simt_cmyk.py runs them with the
kernels on the wave64 emulator, test_gpu_cmyk.py on the chip.

Sources are made at test time in two ways: with tests/jpeg_writer.py from small random coefficient arrays (every marker
combination the colour-space guess looks at, K sampled like Y and lower than Y, a 10-block MCU with a restart interval, four scans)
and with the reference's own TurboJPEG, tj3Compress8(TJPF_CMYK), "as an application writes them".  Every expected value comes from
the reference at test time -- oracle/_ref/libturbojpeg.so.0 through ctypes, oracle/_ref/djpeg, and tests/native/cmyk_client.c
linked to oracle/_ref/libjpeg.so.62 -- or is the array the writer was given; every comparison is exact equality."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import jpeg_writer as JW
import oracle_lib as O
import decode_cases as DC
import djpeg_cases as DJ
import tj_decompress_cases as TD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIENT_SRC = os.path.join(ROOT, "tests", "native", "cmyk_client.c")
REF_INC = os.path.join(O.REF_DIR, "include")

TJCS_CMYK, TJCS_YCCK = 3, 4
TJSAMP_444, TJSAMP_422, TJSAMP_420, TJSAMP_UNKNOWN = 0, 1, 2, -1
UNSUPPORTED_CONVERSION = "Unsupported color conversion request"


def have_tools():
    return TD.have_tools() and DJ.have_tools() and os.path.exists(os.path.join(REF_INC, "jpeglib.h"))


# ---- the reference's TurboJPEG ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tj():
    L = TD.load(TD.TJLIB)
    L.tj3Compress8.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.tj3Free.argtypes = [C.c_void_p]
    return L


def tj_compress(pixels, colorspace, subsamp, progressive=False, quality=90):
    """the file the reference's tj3Compress8 writes for [H, W, 4] CMYK pixels"""
    L = tj()
    h = L.tj3Init(TD.TJINIT_COMPRESS)
    try:
        for prm, v in ((TD.P_QUALITY, quality), (TD.P_SUBSAMP, subsamp), (TD.P_COLORSPACE, colorspace), (TD.P_PROGRESSIVE, int(progressive))):
            assert L.tj3Set(h, prm, v) == 0, TD.err(L, h)
        buf, size = C.c_void_p(), C.c_size_t()
        a = np.ascontiguousarray(pixels, np.uint8)
        assert L.tj3Compress8(h, a.ctypes.data, a.shape[1], 0, a.shape[0], TD.PF_CMYK, C.byref(buf), C.byref(size)) == 0, TD.err(L, h)
        data = C.string_at(buf, size.value)
        L.tj3Free(buf)
        return data
    finally:
        L.tj3Destroy(h)


def tj_header(L, jpeg):
    """(return value, {parameter: value}) of tj3DecompressHeader on library L"""
    h = L.tj3Init(TD.TJINIT_DECOMPRESS)
    try:
        rc = L.tj3DecompressHeader(h, jpeg, len(jpeg))
        return rc, {p: L.tj3Get(h, p) for p in TD.HEADER_PARAMS}, TD.err(L, h)
    finally:
        L.tj3Destroy(h)


def tj_pixels(jpeg, pf=TD.PF_CMYK, fancy=True, fast=False, bottom_up=False, scale=(1, 1)):
    """(return value, [H, W, C] pixels or None, error text) of the reference's tj3Decompress8"""
    L = tj()
    h = L.tj3Init(TD.TJINIT_DECOMPRESS)
    try:
        if L.tj3DecompressHeader(h, jpeg, len(jpeg)) != 0:
            return -1, None, TD.err(L, h)
        w, ht = L.tj3Get(h, TD.P_JPEGWIDTH), L.tj3Get(h, TD.P_JPEGHEIGHT)
        for prm, v in ((TD.P_FASTUPSAMPLE, int(not fancy)), (TD.P_FASTDCT, int(fast)), (TD.P_BOTTOMUP, int(bottom_up))):
            assert L.tj3Set(h, prm, v) == 0
        assert L.tj3SetScalingFactor(h, TD.ScalingFactor(*scale)) == 0
        sw, sh = TD.scaled(w, *scale), TD.scaled(ht, *scale)
        out = np.full((sh, sw, TD.PIXEL_SIZE[pf]), TD.FILL, np.uint8)
        rc = L.tj3Decompress8(h, jpeg, len(jpeg), out.ctypes.data, 0, pf)
        return rc, (out if rc == 0 else None), TD.err(L, h)
    finally:
        L.tj3Destroy(h)


# ---- sources of the writer ------------------------------------------------------------------------------------------------------------
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
LAYOUTS = {           # (h, v) of the four components
    "444": [(1, 1)] * 4,
    "2x2k": [(2, 2), (1, 1), (1, 1), (2, 2)],        # K sampled like Y: 10 blocks in an MCU
    "2x1": [(2, 1), (1, 1), (1, 1), (1, 1)],         # K sampled lower than Y
    "2x2": [(2, 2), (1, 1), (1, 1), (1, 1)],
    "2x2all": [(2, 2)] * 4,                          # 16 blocks: legal only with every component in a scan of its own
}
QTABLES = {0: (0, [3 + (i % 5) for i in range(64)]), 1: (0, [4 + (i % 7) for i in range(64)])}
ONE, FOUR, SPLIT = "one", "four", "split"
# name -> (width, height, layout, header, component ids, scans, restart interval)
WRITER_SOURCES = {
    "ycck444": (37, 29, "444", ("adobe", 2), (1, 2, 3, 4), ONE, 0),
    "ycck2x2k_r2": (37, 29, "2x2k", ("adobe", 2), (1, 2, 3, 4), ONE, 2),
    "ycck2x1": (37, 29, "2x1", ("adobe", 2), (1, 2, 3, 4), ONE, 0),
    "cmyk": (37, 29, "444", ("adobe", 0), (67, 77, 89, 75), ONE, 0),
    "cmyk2x2": (37, 29, "2x2", ("adobe", 0), (67, 77, 89, 75), ONE, 0),
    "nomarker": (37, 29, "444", None, (1, 2, 3, 4), ONE, 0),
    "jfif": (37, 29, "444", "jfif", (1, 2, 3, 4), ONE, 0),
    "scans4": (37, 29, "2x2k", ("adobe", 2), (1, 2, 3, 4), FOUR, 3),
    "scans4_16": (37, 29, "2x2all", ("adobe", 2), (1, 2, 3, 4), FOUR, 0),
    "scans2": (37, 29, "2x1", ("adobe", 2), (1, 2, 3, 4), SPLIT, 0),
    "17x9_2x2k": (17, 9, "2x2k", ("adobe", 2), (1, 2, 3, 4), ONE, 0),
    "1x1_2x2k": (1, 1, "2x2k", ("adobe", 2), (1, 2, 3, 4), ONE, 0),
    "3x40_2x2k": (3, 40, "2x2k", ("adobe", 2), (1, 2, 3, 4), ONE, 1),
    "17x9_2x1": (17, 9, "2x1", ("adobe", 2), (1, 2, 3, 4), ONE, 0),
    "1x1_2x1": (1, 1, "2x1", ("adobe", 2), (1, 2, 3, 4), ONE, 0),
    "3x40_2x1": (3, 40, "2x1", ("adobe", 2), (1, 2, 3, 4), ONE, 0),
}


def _comps(layout, ids):
    return [(ids[c], hv[0], hv[1], 0 if c in (0, 3) else 1) for c, hv in enumerate(LAYOUTS[layout])]


def _coefs(width, height, comps, seed):
    """small random blocks, zig-zag order, padded to whole MCUs: DC values that reach both ends of the sample range, some AC"""
    rng = np.random.default_rng(seed)
    out = []
    for ci in range(len(comps)):
        rows, cols = JW.padded_blocks(width, height, comps, ci)
        a = np.zeros((rows, cols, 64), np.int64)
        a[..., 0] = rng.integers(-230, 231, (rows, cols))
        a[..., 1:12] = rng.integers(-14, 15, (rows, cols, 11)) * (rng.random((rows, cols, 11)) < 0.5)
        a[..., 63] = rng.integers(-2, 3, (rows, cols))
        out.append(a)
    return out


def _scans(kind, ri):
    if kind == ONE:
        return [dict(comps=[0, 1, 2, 3], dc=[0, 1, 1, 0], ac=[0, 1, 1, 0], ri=ri)]
    if kind == FOUR:
        return [dict(comps=[c], dc=[c & 1], ac=[c & 1], ri=ri if c != 2 else 0) for c in range(4)]
    return [dict(comps=[0, 3], dc=[0, 1], ac=[0, 1], ri=ri), dict(comps=[1, 2], dc=[0, 0], ac=[1, 1], ri=ri)]


@functools.lru_cache(maxsize=None)
def written(name):
    """(file, coefficient arrays as the writer got them, components) of a writer source"""
    w, h, layout, header, ids, kind, ri = WRITER_SOURCES[name]
    comps = _comps(layout, ids)
    coefs = _coefs(w, h, comps, sorted(WRITER_SOURCES).index(name) + 1)
    data, _ = JW.write_jpeg(w, h, comps, coefs, QTABLES, _scans(kind, ri), sof=0, header=header)
    return data, coefs, comps


def expected_coefs(name):
    """the real blocks of every component in natural order: what jpeg_read_coefficients hands out"""
    _, coefs, comps = written(name)
    w, h = WRITER_SOURCES[name][:2]
    out = []
    for ci, a in enumerate(coefs):
        rows, cols = JW.real_blocks(w, h, comps, ci)
        nat = np.zeros((rows, cols, 64), np.int16)
        nat[..., ZIGZAG] = a[:rows, :cols]
        out.append(nat)
    return out


# ---- sources of the reference's TurboJPEG ---------------------------------------------------------------------------------------------
def cmyk_frame(width, height, seed):
    rgb = O.synthetic_frame(width, height, seed)
    k = O.synthetic_frame(width, height, seed + 11)[..., 1]
    return np.ascontiguousarray(np.concatenate([255 - rgb, k[..., None]], axis=-1))


TJ_SOURCES = {        # name -> (width, height, colour space, subsampling, progressive)
    "tj_ycck420": (37, 29, TJCS_YCCK, TJSAMP_420, False),
    "tj_ycck422": (37, 29, TJCS_YCCK, TJSAMP_422, False),
    "tj_ycck444": (17, 9, TJCS_YCCK, TJSAMP_444, False),
    "tj_cmyk444": (37, 29, TJCS_CMYK, TJSAMP_444, False),
    "tj_cmyk420": (37, 29, TJCS_CMYK, TJSAMP_420, False),
    "tj_ycck420_prog": (37, 29, TJCS_YCCK, TJSAMP_420, True),
}


@functools.lru_cache(maxsize=None)
def source(name):
    if name in WRITER_SOURCES:
        return written(name)[0]
    w, h, cs, sub, prog = TJ_SOURCES[name]
    return tj_compress(cmyk_frame(w, h, 3), cs, sub, prog)


PIXEL_SOURCES = [n for n in WRITER_SOURCES] + [n for n in TJ_SOURCES if not TJ_SOURCES[n][4]]
MODES = {        # name -> (decode()'s keywords, tj_pixels' keywords)
    "default": (dict(), dict()),
    "nosmooth": (dict(fancy_upsampling=False), dict(fancy=False)),
    "fast": (dict(dct="fast"), dict(fast=True)),
    "bottomup": (dict(bottom_up=True), dict(bottom_up=True)),
}
PIXEL_CASES = [(s, m) for s in PIXEL_SOURCES for m in MODES]
SCALED_SOURCES = ["ycck2x2k_r2", "ycck2x1", "17x9_2x2k", "3x40_2x1", "tj_ycck420"]
SCALED_CASES = [(s, d, f) for s in SCALED_SOURCES for d in (2, 4, 8) for f in (True, False)]


def case_id(c):
    return "-".join(str(v) for v in c)


@functools.lru_cache(maxsize=None)
def reference(name, mode="default", denom=1):
    rc, pix, text = tj_pixels(source(name), scale=(1, denom), **MODES[mode][1])
    assert rc == 0, "the reference's tj3Decompress8(TJPF_CMYK) on %s: %s" % (name, text)
    pix.setflags(write=False)
    return pix


def same(a, b):
    return not isinstance(a, Exception) and a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def decode_one(M, jpeg, **kw):
    out = M.decode([jpeg], **kw)[0]
    if isinstance(out, Exception):
        raise out
    return out


# ---- 0. the sources are what they are meant to be (the reference reads them) -------------------------------------------------------
def check_sources_are_read_by_the_reference():
    for name in PIXEL_SOURCES:
        status, pix = DC.djpeg_status(source(name), [])
        assert status == 0 and pix is not None and pix.shape[2] == 3, "%s: djpeg -pnm exits with %d" % (name, status)
        rc, _, text = tj_pixels(source(name), pf=TD.PF_RGB)
        assert rc == -1 and UNSUPPORTED_CONVERSION in text, "%s: tj3Decompress8(TJPF_RGB) of the reference: %d %s" % (name, rc, text)


# ---- 1. pixels ----------------------------------------------------------------------------------------------------------------------
def check_pixels(M, name, mode):
    ref = reference(name, mode)
    out = decode_one(M, source(name), **MODES[mode][0])
    assert same(out, ref), "%s %s: %s, the reference %s" % (name, mode, out.shape, ref.shape)
    assert same(decode_one(M, source(name), color="cmyk", **MODES[mode][0]), ref)


def check_scaled(M, name, denom, fancy):
    mode = "default" if fancy else "nosmooth"
    ref = reference(name, mode, denom)
    out = decode_one(M, source(name), scale=(1, denom), **MODES[mode][0])
    assert same(out, ref), "%s at 1/%d: %s, the reference %s" % (name, denom, out.shape, ref.shape)


def check_inverted_samples_stay_inverted(M):
    """a CMYK file's pixels are its planes interleaved (null_convert); a YCCK file's are not"""
    planes = M.decode_planes([source("cmyk")])[0]
    pix = decode_one(M, source("cmyk"))
    assert same(pix, reference("cmyk"))
    for c in range(4):
        assert np.array_equal(pix[..., c], planes[c][:29, :37])
    ycck = decode_one(M, source("ycck444"))
    p = M.decode_planes([source("ycck444")])[0]
    assert np.array_equal(ycck[..., 3], p[3][:29, :37]) and not np.array_equal(ycck[..., 0], p[0][:29, :37])


# ---- 2. coefficients and planes ---------------------------------------------------------------------------------------------------
COEF_SOURCES = ["ycck444", "ycck2x2k_r2", "ycck2x1", "cmyk", "scans4", "scans4_16", "scans2", "3x40_2x2k", "1x1_2x1"]
PLANE_SOURCES = ["ycck444", "ycck2x2k_r2", "ycck2x1", "cmyk2x2", "scans4", "17x9_2x1", "1x1_2x2k", "tj_ycck420"]


def check_coefficients(M, name):
    out = M.decode_coefficients([source(name)])[0]
    assert not isinstance(out, Exception), out
    exp = expected_coefs(name)
    assert len(out) == 4
    for c in range(4):
        assert same(out[c], exp[c]), "component %d: %s, written %s" % (c, out[c].shape, exp[c].shape)


@functools.lru_cache(maxsize=None)
def client():
    """tests/native/cmyk_client.c compiled against the reference's headers and linked to its libjpeg.so.62"""
    d = tempfile.mkdtemp(prefix="cmyk_client_")
    exe = os.path.join(d, "cmyk_client")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I" + REF_INC, "-o", exe, CLIENT_SRC, "-L" + O.REF_DIR, "-l:libjpeg.so.62"])
    return exe


def run_client(R, ours, scenario, jpeg, args=()):
    """(exit status, what it printed, its output file) of cmyk_client on the stand-alone library (ours) or the reference's"""
    with tempfile.TemporaryDirectory() as td:
        inp, outp = os.path.join(td, "in.jpg"), os.path.join(td, "out.bin")
        with open(inp, "wb") as f:
            f.write(jpeg)
        r = R.run(ours, [client(), scenario, inp, outp] + [str(a) for a in args])
        data = open(outp, "rb").read() if os.path.exists(outp) else None
        return r.returncode, r.stdout.decode(errors="replace"), data


REF_RUNNER = DJ.Runner(None)


@functools.lru_cache(maxsize=None)
def reference_planes(name):
    """the planes jpeg_read_raw_data of the reference's library gives: per component [height_in_blocks * 8, width_in_blocks * 8]"""
    jpeg = source(name)
    rc, text, data = run_client(REF_RUNNER, False, "raw", jpeg)
    assert rc == 0 and data is not None, text
    dims = [ln.split(", ")[2].split(" x ") for ln in text.splitlines() if ln.startswith("component ")]
    out, pos = [], 0
    for wb, hb in dims:
        wb, hb = int(wb), int(hb.split()[0])
        out.append(np.frombuffer(data, np.uint8, wb * 8 * hb * 8, pos).reshape(hb * 8, wb * 8))
        pos += wb * hb * 64
    assert pos == len(data) and len(out) == 4
    return out


def check_planes(M, name):
    L = tj()
    h = L.tj3Init(TD.TJINIT_DECOMPRESS)
    planes = [np.zeros(64 * 64, np.uint8) for _ in range(3)]
    ptrs = (C.c_void_p * 3)(*[q.ctypes.data for q in planes])
    jpeg = source(name)
    assert L.tj3DecompressToYUVPlanes8(h, jpeg, len(jpeg), ptrs, None) == -1       # (TurboJPEG has no planes of four components)
    assert not any(q.any() for q in planes)
    L.tj3Destroy(h)
    out = M.decode_planes([jpeg])[0]
    assert not isinstance(out, Exception), out
    ref = reference_planes(name)
    assert len(out) == 4
    for c in range(4):
        hh, ww = out[c].shape
        assert hh <= ref[c].shape[0] and ww <= ref[c].shape[1] and np.array_equal(out[c], ref[c][:hh, :ww]), "component %d" % c



# ---- 3. batches -------------------------------------------------------------------------------------------------------------------------
def damage(M, jpeg):
    """the file with 40 bytes of its entropy-coded data missing, every marker segment in place (scale_cases.damaged)"""
    info = M.jpeg_info(jpeg)
    a, n = info.scans[0].data_offset, info.scans[0].data_size
    assert n > 200
    return jpeg[:a + n // 2] + jpeg[a + n // 2 + 40:]


def check_batch_with_a_damaged_file(M):
    w, h, layout, header, ids, kind, ri = WRITER_SOURCES["ycck2x2k_r2"]
    comps = _comps(layout, ids)
    files = [JW.write_jpeg(w, h, comps, _coefs(w, h, comps, 100 + k), QTABLES, _scans(kind, ri), header=header)[0] for k in range(3)]
    refs = [tj_pixels(f)[1] for f in files]
    assert all(r is not None for r in refs) and not np.array_equal(refs[0], refs[2])
    bad = damage(M, files[1])
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True), max_batch=3)
    try:
        res = enc.decode_host([files[0], bad, files[2]], errors="return")
        assert isinstance(res[1], M.MjhError) and res[0] is None and res[2] is None, res      # nothing of such a batch is handed out
        with pytest.raises(M.MjhError):
            enc.get_pixels(1)
    finally:
        enc.close()
    out = M.decode([files[0], bad, files[2]])
    assert isinstance(out[1], M.MjhError)
    assert same(out[0], refs[0]) and same(out[2], refs[2])


def check_mixed_batch(M):
    """a YCbCr, a YCCK and a CMYK file of one size in one decode() call: input order, one group each"""
    import transcode_cases as TC
    ycc = TC.cjpeg(O.synthetic_frame(37, 29, 5), ["-revert", "-sample", "1x1"])
    files = [source("cmyk"), ycc, source("ycck444"), source("nomarker"), ycc, source("ycck444")]
    out = M.decode(files)
    assert same(out[0], reference("cmyk")) and same(out[2], reference("ycck444")) and same(out[3], reference("nomarker")) and same(out[5], reference("ycck444"))
    assert same(out[1], DC.djpeg(ycc, [])) and same(out[4], out[1])
    sigs = {M._signature(M.jpeg_info(f)) for f in files}
    assert len(sigs) == 4                                     # cmyk / nomarker differ in component ids; CMYK against YCCK in the colour space alone
    # through one encoder CMYK and YCCK files of one frame do not mix: the second is refused in its slot
    enc = M.Encoder(M.params_from_jpeg(source("ycck444"), revert=True), max_batch=2)
    try:
        res = enc.decode_host([source("ycck444"), source("nomarker")], errors="return")
        assert res[0] is None and isinstance(res[1], M.MjhError) and "colour space" in str(res[1]), res
    finally:
        enc.close()


# ---- 4. progressive -------------------------------------------------------------------------------------------------------------------
def check_progressive(M):
    jpeg = source("tj_ycck420_prog")
    assert b"\xff\xc2" in jpeg[:600]
    out = M.decode([jpeg])[0]
    assert isinstance(out, M.MjhError) and out.code == M.EUNSUPPORTED and "progressive" in str(out)
    rc, ref, text = tj_pixels(jpeg)
    assert rc == 0, text
    out = M.decode([jpeg], progressive_sources=True)[0]
    assert same(out, ref), out
    info = M.jpeg_info(jpeg, progressive_sources=True)
    assert info.num_components == 4 and info.jpeg_color_space == M.CS_YCCK and info.sof_type == 2


# ---- 5. what the probe reports, and refusals ---------------------------------------------------------------------------------------
def check_info(M):
    for name, cs in (("ycck444", M.CS_YCCK), ("cmyk", M.CS_CMYK), ("nomarker", M.CS_CMYK), ("jfif", M.CS_CMYK), ("tj_ycck420", M.CS_YCCK), ("tj_cmyk444", M.CS_CMYK)):
        info = M.jpeg_info(source(name))
        assert info.num_components == 4 and info.jpeg_color_space == cs, (name, info.jpeg_color_space)
        rc, prm, _ = tj_header(tj(), source(name))
        assert rc == 0 and prm[TD.P_COLORSPACE] == (TJCS_YCCK if cs == M.CS_YCCK else TJCS_CMYK)
    assert (M.CS_CMYK, M.CS_YCCK) == (4, 5)
    p = M.params_from_jpeg(source("ycck2x2k_r2"), revert=True)
    assert p.num_components == 4 and [p.h_samp_factor[c] for c in range(4)] == [2, 1, 1, 2]
    assert M.params_from_jpeg(source("cmyk"), revert=True).color_transform != p.color_transform


def _patched_sof(jpeg, comp, hv):
    """the file with the sampling byte of frame component `comp` replaced"""
    at = jpeg.index(b"\xff\xc0")
    b = bytearray(jpeg)
    b[at + 10 + 3 * comp + 1] = hv
    return bytes(b)


def two_component_file():
    comps = [(1, 1, 1, 0), (2, 1, 1, 0)]
    coefs = _coefs(16, 16, comps, 9)
    return JW.write_jpeg(16, 16, comps, coefs, QTABLES, [dict(comps=[0, 1], dc=[0, 0], ac=[0, 0], ri=0)], header=None)[0]


def lossless_four_component_file():
    """SOF3, four components of 8 bits, one scan: the frame and scan headers are enough for the probe to refuse it"""
    seg = lambda m, p: bytes([0xFF, m]) + (len(p) + 2).to_bytes(2, "big") + p
    frame = bytes([8, 0, 8, 0, 8, 4]) + b"".join(bytes([c + 1, 0x11, 0]) for c in range(4))
    dht = bytes([0]) + bytes([0, 1] + [0] * 14) + bytes([0])
    sos = bytes([4]) + b"".join(bytes([c + 1, 0]) for c in range(4)) + bytes([1, 0, 0])
    return b"\xff\xd8" + seg(0xC3, frame) + seg(0xC4, dht) + seg(0xDA, sos) + b"\x00" * 32 + b"\xff\xd9"


def check_refusals(M):
    # Adobe transform 1: the reference warns and goes on, this library names the code
    w, h, layout, _, ids, kind, ri = WRITER_SOURCES["ycck444"]
    comps = _comps(layout, ids)
    xf1 = JW.write_jpeg(w, h, comps, _coefs(w, h, comps, 77), QTABLES, _scans(kind, ri), header=("adobe", 1))[0]
    status, _ = DC.djpeg_status(xf1, [])
    assert status == 2                                        # (djpeg's exit status for a warning)
    for call in (M.jpeg_info, lambda f: decode_one(M, f)):
        with pytest.raises(M.MjhError) as ei:
            call(xf1)
        assert ei.value.code == M.EUNSUPPORTED and "Adobe color transform code 1" in str(ei.value), str(ei.value)
    # an interleaved scan of more than 10 blocks: 2x2 + 2x1 + 1x1 + 2x2 (the frame header of the 10-block file says so)
    big = _patched_sof(source("ycck2x2k_r2"), 1, 0x21)
    status, _ = DC.djpeg_status(big, [])
    assert status == 1
    out = M.decode([big])[0]
    assert isinstance(out, M.MjhError) and out.code == M.EINVAL and "JERR_BAD_MCU_SIZE" in str(out), out
    # colour conversions the reference has none of
    for kw in (dict(color="gray"), dict(color="rgb"), dict(color="rgb565")):
        out = M.decode([source("ycck444"), source("ycck444")], **kw)
        for o in out:
            assert isinstance(o, M.MjhError) and o.code == M.EUNSUPPORTED and UNSUPPORTED_CONVERSION in str(o), (kw, o)
    import transcode_cases as TC
    ycc = TC.cjpeg(O.synthetic_frame(37, 29, 5), ["-revert"])
    gray = TC.cjpeg(O.synthetic_frame(37, 29, 5), ["-revert", "-grayscale"])
    out = M.decode([ycc, source("ycck444"), gray], color="cmyk")
    assert same(out[1], reference("ycck444"))
    for o in (out[0], out[2]):
        assert isinstance(o, M.MjhError) and o.code == M.EUNSUPPORTED and UNSUPPORTED_CONVERSION in str(o), o
    for f in (ycc, gray):                                      # (the reference says the same)
        rc, _, text = tj_pixels(f, pf=TD.PF_CMYK)
        assert rc == -1 and UNSUPPORTED_CONVERSION in text, text
    with pytest.raises(M.MjhError) as ei:
        M.decode([source("ycck444")], color="cmyk", pixel_size=3)
    assert ei.value.code == M.EINVAL
    with pytest.raises(M.MjhError) as ei:
        M.decode([source("ycck444")], layout="cmyk")
    assert ei.value.code == M.EINVAL
    # two components
    with pytest.raises(M.MjhError) as ei:
        M.jpeg_info(two_component_file())
    assert ei.value.code == M.EUNSUPPORTED and "2 components" in str(ei.value)
    # four components in a lossless file
    with pytest.raises(M.MjhError) as ei:
        M.jpeg_info(lossless_four_component_file(), lossless_sources=True)
    assert ei.value.code == M.EUNSUPPORTED and "4 components" in str(ei.value) and "lossless" in str(ei.value), str(ei.value)
    out = M.decode([lossless_four_component_file()], lossless_sources=True)[0]
    assert isinstance(out, M.MjhError) and out.code == M.EUNSUPPORTED


def check_nothing_is_written(M):
    """four-component files are decoded, not written: every call that would write one says so"""
    src = source("ycck2x1")
    out = M.recompress([src, source("cmyk")])
    for o in out:
        assert isinstance(o, M.MjhError) and o.code == M.EUNSUPPORTED and "decoded, not written" in str(o), o
    out = M.recompress([src], transform="rot90")
    assert isinstance(out[0], M.MjhError) and out[0].code == M.EUNSUPPORTED and "decoded, not written" in str(out[0]), out[0]
    enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=1)
    try:
        calls = [lambda: enc.transcode_host([src]), lambda: enc.encode_host(np.zeros((1, 29, 37, 4), np.uint8)),
                 lambda: enc.encode_coefficients_host([np.zeros((hb, wb, 64), np.int16) for wb, hb in (enc.geometry(c)[:2] for c in range(4))]),
                 lambda: enc.set_transform(transform="flip_h")]
        for k, call in enumerate(calls):
            with pytest.raises(M.MjhError) as ei:
                call()
            assert ei.value.code == M.EUNSUPPORTED and "decoded, not written" in str(ei.value), (k, str(ei.value))
        assert same(enc.decode_host([src])[0], reference("ycck2x1"))      # and the encoder still decodes
    finally:
        enc.close()
    # parameters of four components made any other way create nothing
    p = M.make_params(37, 29)
    p.num_components = 4
    with pytest.raises(M.MjhError) as ei:
        M.Encoder(p, max_batch=1)
    assert ei.value.code == M.EUNSUPPORTED


# ---- 6. the TurboJPEG-signature library next to the reference's (S, R: the two libraries, tj_decompress_cases.load) ----------------
TJ_HEADER_SOURCES = ["ycck444", "ycck2x2k_r2", "ycck2x1", "cmyk", "cmyk2x2", "nomarker", "jfif", "scans4", "scans4_16", "1x1_2x1", "tj_ycck420", "tj_ycck422", "tj_cmyk444"]


@TD.with_pair
def check_tj_headers(p):
    seen = set()
    for name in TJ_HEADER_SOURCES:
        src = source(name)
        assert p.same("tj3DecompressHeader", src, len(src)) == 0, name
        for prm in TD.HEADER_PARAMS:
            p.same("tj3Get", prm)
        seen.add((p.R.tj3Get(p.hr, TD.P_COLORSPACE), p.R.tj3Get(p.hr, TD.P_SUBSAMP)))
        outs = []
        for L, h in ((p.S, p.hs), (p.R, p.hr)):
            v = [C.c_int(-5) for _ in range(4)]
            outs.append((L.tjDecompressHeader3(h, src, len(src), *[C.byref(x) for x in v]), [x.value for x in v]))
        # (a file without a TJSAMP fails the legacy call in both; the reference returns before it stores the colour space)
        assert outs[0][0] == outs[1][0] == (-1 if outs[1][1][2] == TJSAMP_UNKNOWN else 0) and outs[0][1][:3] == outs[1][1][:3], (name, outs)
        assert outs[0][0] == -1 or outs[0][1] == outs[1][1], (name, outs)
    # the cases are worth something: both colour spaces, known subsamplings and a K sampled unlike Y
    assert {(TJCS_YCCK, TJSAMP_444), (TJCS_YCCK, TJSAMP_420), (TJCS_YCCK, TJSAMP_422), (TJCS_YCCK, TJSAMP_UNKNOWN), (TJCS_CMYK, TJSAMP_444), (TJCS_CMYK, TJSAMP_UNKNOWN)} <= seen, seen


def _tj_options(p, name):
    src = source(name)
    for sf in ((1, 1), (1, 2), (1, 4), (1, 8)):
        for extra in (None, 5):
            for bottom_up, fast_up, fast_dct in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
                p.set(bottomup=bottom_up, fastupsample=fast_up, fastdct=fast_dct)
                p.pixels(src, TD.PF_CMYK, extra, sf)
    p.set(bottomup=0, fastupsample=0, fastdct=0)
    top = p.pixels(src, TD.PF_CMYK).copy()
    w, h, _ = p.size(src)
    assert np.array_equal(top[:w * h * 4].reshape(h, w, 4), reference(name))
    p.set(bottomup=1)
    assert np.array_equal(p.pixels(src, TD.PF_CMYK)[:w * h * 4].reshape(h, w, 4), top[:w * h * 4].reshape(h, w, 4)[::-1])
    p.set(bottomup=0)


@TD.with_pair
def check_tj_pixels_ycck(p):
    _tj_options(p, "ycck2x2k_r2")
    _tj_options(p, "tj_ycck420")


@TD.with_pair
def check_tj_pixels_k_lower(p):
    _tj_options(p, "ycck2x1")
    _tj_options(p, "3x40_2x1")


@TD.with_pair
def check_tj_pixels_cmyk(p):
    _tj_options(p, "cmyk")
    _tj_options(p, "tj_cmyk420")
    for name in ("nomarker", "jfif", "scans4", "scans4_16", "1x1_2x2k", "17x9_2x1"):
        p.pixels(source(name), TD.PF_CMYK)


@TD.with_pair
def check_tj_legacy(p):
    src = source("tj_ycck420")
    for flags in (0, TD.FLAG_FASTDCT, TD.FLAG_BOTTOMUP | TD.FLAG_FASTUPSAMPLE):
        for width, height in ((0, 0), (37, 29), (19, 15), (5, 4)):                # full, full, 1/2, 1/8
            a = np.full((37 * 29 * 4 + 64,), TD.FILL, np.uint8)
            b = a.copy()
            ra = p.S.tjDecompress2(p.hs, src, len(src), a.ctypes.data, width, 0, height, TD.PF_CMYK, flags)
            rb = p.R.tjDecompress2(p.hr, src, len(src), b.ctypes.data, width, 0, height, TD.PF_CMYK, flags)
            assert ra == rb == 0 and np.array_equal(a, b), (flags, width, height, ra, rb, TD.err(p.S, p.hs))


@TD.with_pair
def check_tj_refusals(p):
    import transcode_cases as TC
    buf = np.full((37 * 29 * 4 + 64,), TD.FILL, np.uint8)
    ref = buf.copy()
    for name in ("ycck444", "cmyk", "tj_ycck420"):
        src = source(name)
        for pf in range(11):                                              # every format but TJPF_CMYK
            ra, rb = p.both("tj3Decompress8", src, len(src), buf.ctypes.data, 0, pf)
            assert ra == rb == -1, (name, pf, ra, rb)
            assert UNSUPPORTED_CONVERSION in TD.err(p.S, p.hs) and UNSUPPORTED_CONVERSION in TD.err(p.R, p.hr), (TD.err(p.S, p.hs), TD.err(p.R, p.hr))
            assert (buf == TD.FILL).all()
        p.pixels(src, TD.PF_CMYK)                                         # the same handles still decode it
    for src in (TC.cjpeg(O.synthetic_frame(37, 29, 5), ["-revert"]), TC.cjpeg(O.synthetic_frame(37, 29, 5), ["-revert", "-grayscale"])):
        ra = p.S.tj3Decompress8(p.hs, src, len(src), buf.ctypes.data, 0, TD.PF_CMYK)
        rb = p.R.tj3Decompress8(p.hr, src, len(src), ref.ctypes.data, 0, TD.PF_CMYK)
        assert ra == rb == -1 and UNSUPPORTED_CONVERSION in TD.err(p.S, p.hs) and UNSUPPORTED_CONVERSION in TD.err(p.R, p.hr)
        assert "CMYK" in TD.err(p.S, p.hs) and (buf == TD.FILL).all()
    # planar YUV output: the reference has none for four components, whatever the subsampling says
    planes = [np.full((64 * 64,), TD.FILL, np.uint8) for _ in range(3)]
    ptrs = (C.c_void_p * 3)(*[q.ctypes.data for q in planes])
    big = np.full((64 * 64 * 4,), TD.FILL, np.uint8)
    for name in ("tj_ycck420", "ycck444", "ycck2x1", "cmyk"):
        src = source(name)
        ra, rb = p.both("tj3DecompressToYUVPlanes8", src, len(src), ptrs, None)
        assert ra == rb == -1, (name, ra, rb)
        assert TD.err(p.S, p.hs) == TD.err(p.R, p.hr), (TD.err(p.S, p.hs), TD.err(p.R, p.hr))
        ra, rb = p.both("tj3DecompressToYUV8", src, len(src), big.ctypes.data, 4)
        assert ra == rb == -1, (name, ra, rb)
        ra, rb = p.both("tjDecompressToYUV2", src, len(src), big.ctypes.data, 0, 4, 0, 0)
        assert ra == rb == -1, (name, ra, rb)
        assert all((q == TD.FILL).all() for q in planes) and (big == TD.FILL).all()
    # Adobe transform 1: the reference warns (-1 with the pixels written), this library names the code and writes nothing
    w, h, layout, _, ids, kind, ri = WRITER_SOURCES["ycck444"]
    comps = _comps(layout, ids)
    xf1 = JW.write_jpeg(w, h, comps, _coefs(w, h, comps, 77), QTABLES, _scans(kind, ri), header=("adobe", 1))[0]
    ra = p.S.tj3Decompress8(p.hs, xf1, len(xf1), buf.ctypes.data, 0, TD.PF_CMYK)
    rb = p.R.tj3Decompress8(p.hr, xf1, len(xf1), ref.ctypes.data, 0, TD.PF_CMYK)
    assert ra == rb == -1 and "Adobe color transform code 1" in TD.err(p.S, p.hs) and "Adobe color transform code 1" in TD.err(p.R, p.hr)
    assert (buf == TD.FILL).all()


TJ_CHECKS = {
    "headers": check_tj_headers,
    "pixels_ycck": check_tj_pixels_ycck,
    "pixels_k_lower": check_tj_pixels_k_lower,
    "pixels_cmyk": check_tj_pixels_cmyk,
    "legacy": check_tj_legacy,
    "refusals": check_tj_refusals,
}


def main(shim_path):
    """every TurboJPEG check against the library at shim_path; prints {"name": "ok" | traceback} (test_simt_cmyk.py's child process)"""
    import json
    import traceback
    S, R = TD.load(shim_path), TD.load(TD.TJLIB)
    res = {}
    for name, fn in TJ_CHECKS.items():
        try:
            fn(S, R)
            res[name] = "ok"
        except BaseException:
            res[name] = traceback.format_exc()
    print("CMYK_TJ_RESULTS " + json.dumps(res))


# ---- 7. the stand-alone libjpeg.so.62 under the unchanged djpeg and under cmyk_client (R: djpeg_cases.Runner) ---------------------
DJPEG_SOURCES = ["ycck2x2k_r2", "tj_ycck420", "cmyk"]
DJPEG_SWITCHES = {"ppm": [], "nosmooth": ["-nosmooth"], "scale2": ["-scale", "1/2"], "dctfast": ["-dct", "fast"], "bmp": ["-bmp"]}
DJPEG_PAIRS = [(s, k) for s in DJPEG_SOURCES for k in DJPEG_SWITCHES]
_djpeg_ref = {}


def check_djpeg(R, name, switches):
    """the unchanged djpeg on the stand-alone library == on the reference's: output file and exit status"""
    key = (name, tuple(switches))
    if key not in _djpeg_ref:
        _djpeg_ref[key] = R.djpeg(False, source(name), list(switches))
    ref = _djpeg_ref[key]
    assert ref[0] == 0 and ref[1], "the reference's djpeg: %d %s" % (ref[0], ref[2][-500:])
    out = R.djpeg(True, source(name), list(switches))
    assert out[0] == ref[0], "exit status %d, the reference %d\n%s" % (out[0], ref[0], out[2].decode(errors="replace")[-2000:])
    assert out[1] == ref[1], "the output file differs"


def check_djpeg_refused_conversions(R):
    for name in ("ycck2x2k_r2", "cmyk"):
        for switches in (["-grayscale"], ["-rgb"], ["-rgb565", "-bmp"]):
            ref = R.djpeg(False, source(name), switches)
            out = R.djpeg(True, source(name), switches)
            assert out[0] == ref[0] == 1, (name, switches, out[0], ref[0])
            assert UNSUPPORTED_CONVERSION.encode() in out[2] and UNSUPPORTED_CONVERSION.encode() in ref[2], (out[2], ref[2])


CLIENT_SOURCES = ["ycck2x2k_r2", "ycck2x1", "cmyk2x2", "scans4", "1x1_2x2k"]


def check_client(R, name):
    """jpeg_read_raw_data and jpeg_read_scanlines(JCS_CMYK) of the stand-alone library: what is printed and written == the reference's"""
    for scenario, args in (("raw", ()), ("pixels", (-1,)), ("pixels", (4,))):
        ref = run_client(R, False, scenario, source(name), args)
        assert ref[0] == 0 and ref[2], ref[1]
        out = run_client(R, True, scenario, source(name), args)
        assert out[0] == 0 and out[1] == ref[1], "printed on the stand-alone library:\n%s\non the reference's:\n%s" % (out[1], ref[1])
        assert out[2] == ref[2], "%s %s: the output file differs" % (scenario, args)
    w, h = WRITER_SOURCES[name][:2]
    assert np.array_equal(np.frombuffer(run_client(R, True, "pixels", source(name), (-1,))[2], np.uint8).reshape(h, w, 4), reference(name))
    for cs in (1, 2, 3, 16):                                  # JCS_GRAYSCALE, JCS_RGB, JCS_YCbCr, JCS_RGB565
        ref = run_client(R, False, "pixels", source(name), (cs,))
        out = run_client(R, True, "pixels", source(name), (cs,))
        assert out[0] == ref[0] == 1 and UNSUPPORTED_CONVERSION in out[1] and UNSUPPORTED_CONVERSION in ref[1], (cs, out[1], ref[1])


def check_read_coefficients(R, name):
    """jpeg_read_coefficients of the stand-alone library (tests/native/coef_dump on both libraries): four arrays, the reference's"""
    import coef_cases as CC
    if not CC.have_tools():
        pytest.skip("tests/native/coef_dump not built")
    ours = CC.both(R, "dump", [source(name)], ("fields",))
    arrays = CC.parse_dump(ours[2])
    assert len(arrays) == 4
    if name in WRITER_SOURCES:
        for a, e in zip(arrays, expected_coefs(name)):
            assert same(a, e)


if __name__ == "__main__":
    import sys
    main(sys.argv[1])
