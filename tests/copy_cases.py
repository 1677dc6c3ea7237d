"""The cases of the marker-copy tests (test_simt_copy.py on the emulator, test_gpu_copy.py on the chip): re-compression with
COM / APPn markers kept (jpegtran -copy comments / all / icc, -icc FILE) and ICC profiles on encode (cjpeg -icc FILE).

Sources are made at test time by the reference's cjpeg -revert and get their markers by byte surgery here; every expected byte
comes from the reference's jpegtran / cjpeg (oracle/_ref) at test time, and every comparison is of whole files."""
import functools
import os
import struct
import tempfile

import numpy as np

import oracle_lib as O
import transcode_cases as TC

SOI, EOI = b"\xff\xd8", b"\xff\xd9"
COM, APP0 = 0xFE, 0xE0

# jpegtran's coding switches: name -> (keywords of recompress, the program's arguments)
SWITCHES = {"revert": (dict(revert=True), ["-revert"]), "revert_opt": (dict(revert=True, optimize=True), ["-revert", "-optimize"]),
            "default": (dict(), [])}
COPIES = ["none", "comments", "all", "icc"]


def have_tools():
    return TC.have_tools()


def seg(code, data=b""):
    """one marker segment: FF xx, length, data"""
    assert len(data) <= 65533
    return bytes([0xFF, code]) + struct.pack(">H", len(data) + 2) + bytes(data)


def blob(n, seed):
    """n pseudo-random bytes (0xFF among them: marker data is not stuffed)"""
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def icc_segments(profile, per=65519):
    """the APP2 segments an ICC profile travels in"""
    parts = [profile[o:o + per] for o in range(0, len(profile), per)]
    return b"".join(seg(0xE2, b"ICC_PROFILE\0" + bytes([k + 1, len(parts)]) + p) for k, p in enumerate(parts))


@functools.lru_cache(maxsize=None)
def base(name):
    """a source without markers of its own beyond the JFIF APP0"""
    if name == "16x16":
        return TC.cjpeg(O.synthetic_frame(16, 16, 9), ["-revert"])
    if name == "16x16b":
        return TC.cjpeg(O.synthetic_frame(16, 16, 10), ["-revert", "-optimize"])
    if name == "16x16_rgb":
        return TC.cjpeg(O.synthetic_frame(16, 16, 9), ["-revert", "-rgb"])
    if name == "16x16_scans3":
        return TC.cjpeg(O.synthetic_frame(16, 16, 9), ["-revert"], script=TC.SCRIPT_3)
    if name == "16x16_prog":
        return TC.cjpeg(O.synthetic_frame(16, 16, 9), ["-revert", "-progressive"])
    return TC.source({"17x9": "17x9", "227x149": "revert"}[name])


def behind_app0(jpeg, segments):
    """the segments right behind the file's first marker segment (its JFIF APP0 / Adobe APP14)"""
    assert jpeg[:2] == SOI and jpeg[2] == 0xFF and jpeg[3] in (0xE0, 0xEE)
    end = 4 + struct.unpack(">H", jpeg[4:6])[0]
    return jpeg[:end] + segments + jpeg[end:]


def without_app0(jpeg, segments):
    """the segments in place of the file's JFIF APP0: the file begins SOI + segments"""
    assert jpeg[:4] == SOI + b"\xff\xe0"
    end = 4 + struct.unpack(">H", jpeg[4:6])[0]
    return SOI + segments + jpeg[end:]


def exif(big_endian, width, height, truncated=False):
    """an APP1 Exif segment: IFD0 = { Orientation, ExifSubIFD pointer }, ExifSubIFD = { ExifVersion, ExifImageWidth, ExifImageHeight }
    (the dimensions as SHORT, so that a rewrite changes their type as well).  truncated: the segment ends inside the ExifSubIFD,
    behind its first entry."""
    e = ">" if big_endian else "<"
    entry = lambda tag, typ, count, value: struct.pack(e + "HHI", tag, typ, count) + value
    short = lambda v: struct.pack(e + "H", v) + b"\0\0"
    sub_off = 8 + 2 + 2 * 12 + 4
    tiff = (b"MM" if big_endian else b"II") + struct.pack(e + "HI", 42, 8)
    tiff += struct.pack(e + "H", 2) + entry(0x0112, 3, 1, short(6)) + entry(0x8769, 4, 1, struct.pack(e + "I", sub_off)) + struct.pack(e + "I", 0)
    assert len(tiff) == sub_off
    tiff += struct.pack(e + "H", 3) + entry(0x9000, 7, 4, b"0230") + entry(0xA002, 3, 1, short(width)) + entry(0xA003, 3, 1, short(height))
    tiff += struct.pack(e + "I", 0)
    if truncated:
        tiff = tiff[:sub_off + 2 + 12 + 4]
    return seg(0xE1, b"Exif\0\0" + tiff)


def segments_of(jpeg):
    """[(code, data)] of the marker segments in front of the first SOS"""
    out, pos = [], 2
    while jpeg[pos + 1] != 0xDA:
        n = struct.unpack(">H", jpeg[pos + 2:pos + 4])[0]
        out.append((jpeg[pos + 1], jpeg[pos + 4:pos + 2 + n]))
        pos += 2 + n
    return out


ICC_IN_FILE = blob(700, 21)        # the profile the rich source carries, in two segments
ICC_GIVEN = blob(3000, 22)         # the profile of -icc FILE


@functools.lru_cache(maxsize=None)
def rich():
    """one 16x16 source with a COM, an Exif APP1 that is not the first marker, an APP12, an ICC profile in two APP2 segments, an
    empty COM and a JFXX APP0"""
    s = seg(COM, b"a comment") + exif(False, 16, 16) + seg(0xEC, b"Ducky\0" + blob(40, 1)) + icc_segments(ICC_IN_FILE, per=400)
    s += seg(COM) + seg(APP0, b"JFXX\0\x10" + blob(17, 2))
    return behind_app0(base("16x16"), s)


def reference(jpeg, copy, sw="revert", icc=None, extra=()):
    """the reference's jpegtran -copy <copy> [-icc FILE] + switches on the file"""
    args = ["-copy", copy] + SWITCHES[sw][1] + list(extra)
    if icc is None:
        return O.ref_jpegtran(jpeg, args)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "profile.icc")
        with open(path, "wb") as f:
            f.write(icc)
        return O.ref_jpegtran(jpeg, args + ["-icc", path])


def run(M, files, copy, sw="revert", icc=None, **kw):
    """recompress() on the files; an MjhError in a slot is raised"""
    single = isinstance(files, (bytes, bytearray))
    out = M.recompress([files] if single else list(files), copy=copy, icc=icc, **dict(SWITCHES[sw][0], **kw))
    if single:
        if isinstance(out[0], Exception):
            raise out[0]
        return out[0]
    return out


def same(out, ref, what=""):
    assert not isinstance(out, Exception), "%s: %s" % (what, out)
    if out != ref:
        k = next((i for i in range(min(len(out), len(ref))) if out[i] != ref[i]), min(len(out), len(ref)))
        raise AssertionError("%s: %d bytes, the reference %d; first difference at byte %d" % (what, len(out), len(ref), k))


# ---- 1. modes ---------------------------------------------------------------------------------------------------------------------
MODE_CASES = [(c, s, i) for c in COPIES for s in SWITCHES for i in (False, True)]


def check_mode(M, copy, sw, with_icc):
    icc = ICC_GIVEN if with_icc else None
    same(run(M, rich(), copy, sw, icc), reference(rich(), copy, sw, icc), "copy=%s %s icc=%s" % (copy, sw, with_icc))
    if copy == "none" and not with_icc:      # today's output, through today's keywords
        out = M.recompress([rich()], **SWITCHES[sw][0])[0]
        same(out, O.ref_jpegtran(rich(), ["-copy", "none"] + SWITCHES[sw][1]), "no keyword")


# ---- 2. every shift ---------------------------------------------------------------------------------------------------------------
def check_every_shift(M, behind_app7):
    """a COM of every data length 0..33 (every shift modulo 16, twice), all files in one batch; behind_app7: the COM stands behind
    a 5-byte APP7, so that where its bytes lie in the source varies as well"""
    lead = seg(0xE7, b"seven") if behind_app7 else b""
    files = [behind_app0(base("16x16"), lead + seg(COM, blob(n, 100 + n))) for n in range(34)]
    outs = run(M, files, "all", max_batch=34)
    for n, (f, o) in enumerate(zip(files, outs)):
        same(o, reference(f, "all"), "COM of %d bytes" % n)


# ---- 3. Exif first ----------------------------------------------------------------------------------------------------------------
def exif_first(name, big_endian, truncated=False, extra=b""):
    w, h = {"16x16": (16, 16), "227x149": (227, 149)}[name]
    return without_app0(base(name), exif(big_endian, w, h, truncated) + extra)


def check_exif_first(M, big_endian):
    src = exif_first("16x16", big_endian, extra=seg(COM, b"x"))
    out = run(M, src, "all")
    same(out, reference(src, "all"), "plain")
    assert out[:4] == SOI + b"\xff\xe1" and segments_of(out)[0][1] == segments_of(src)[0][1]      # no JFIF, nothing rewritten
    out = run(M, src, "all", transform="rot90")        # 16x16 stays 16x16: nothing to rewrite
    same(out, reference(src, "all", extra=["-rotate", "90"]), "rot90 of a square")
    big = exif_first("227x149", big_endian)
    for kw, extra in ((dict(transform="rot90"), ["-rotate", "90"]), (dict(crop="100x80+16+8"), ["-crop", "100x80+16+8"])):
        out = run(M, big, "all", **kw)
        same(out, reference(big, "all", extra=extra), str(kw))
        assert segments_of(out)[0][0] == 0xE1 and segments_of(out)[0][1] != segments_of(big)[0][1]   # the dimensions were rewritten
    same(run(M, big, "comments", transform="rot90"), reference(big, "comments", extra=["-rotate", "90"]), "comments")
    assert run(M, big, "comments", transform="rot90")[2:4] == b"\xff\xe0"                            # JFIF stays, APP1 is not saved


def check_exif_truncated(M):
    for be in (False, True):
        src = exif_first("227x149", be, truncated=True)
        out = run(M, src, "all", transform="rot90")
        same(out, reference(src, "all", extra=["-rotate", "90"]), "truncated IFD")
        assert segments_of(out)[0] == segments_of(src)[0]


def check_exif_behind_jfif(M):
    src = behind_app0(base("227x149"), exif(False, 227, 149))
    out = run(M, src, "all", transform="rot90")
    same(out, reference(src, "all", extra=["-rotate", "90"]), "JFIF, then Exif")
    segs = segments_of(out)
    assert segs[0][0] == APP0 and segs[1] == segments_of(src)[1]


# ---- 4. markers behind the first SOS ----------------------------------------------------------------------------------------------
def check_markers_behind_sos(M):
    src = base("16x16_scans3")
    info = M.jpeg_info(src)
    assert info.num_scans == 3
    cut = info.scans[0].data_offset + info.scans[0].data_size          # the end of the first scan's data
    src = src[:cut] + seg(COM, b"between the scans") + src[cut:-2] + seg(0xE5, b"in front of EOI") + EOI
    assert [m for m, _ in M.jpeg_markers(src, "all")] == [APP0, COM, 0xE5]
    for sw in ("revert", "revert_opt"):
        out = run(M, src, "all", sw)
        same(out, reference(src, "all", sw), sw)
        assert [c for c, _ in segments_of(out)][:3] == [APP0, COM, 0xE5]


# ---- 5. Adobe ---------------------------------------------------------------------------------------------------------------------
def check_adobe(M):
    rgb = behind_app0(base("16x16_rgb"), seg(COM, b"rgb"))
    assert rgb[2:4] == b"\xff\xee"
    out = run(M, rgb, "all")
    same(out, reference(rgb, "all"), "an -rgb source")
    assert [c for c, _ in segments_of(out)][:2] == [0xEE, COM]           # the encoder's APP14, the source's rejected
    ycc = behind_app0(base("16x16"), seg(0xEE, b"Adobe\0\x64\0\0\0\0\x01"))      # transform 1: YCbCr, as the JFIF marker says
    same(run(M, ycc, "all"), reference(ycc, "all"), "a YCbCr source with an Adobe APP14")
    assert (0xEE, b"Adobe\0\x64\0\0\0\0\x01") in segments_of(run(M, ycc, "all"))


# ---- 6. large ---------------------------------------------------------------------------------------------------------------------
def check_large(M):
    big = behind_app0(base("16x16"), b"".join(seg(0xE3 + k, blob(65533, 40 + k)) for k in range(3)))
    ref = reference(big, "all")
    same(run(M, big, "all", max_batch=1), ref, "alone: the file exceeds the arena")
    plain = [base("16x16"), behind_app0(base("16x16"), seg(COM, b"plain")), base("16x16b")]
    outs = run(M, [plain[0], big, plain[1], plain[2]], "all", max_batch=4)
    four = [plain[0], big, plain[1], plain[2]]
    for f, o in zip(four, outs):
        same(o, reference(f, "all"), "in a batch of four")
    # which path each took: collect() hands out the arena alone
    for max_batch, files in ((1, [big]), (4, four)):
        enc = M.Encoder(M.params_from_jpeg(big, revert=True), max_batch=max_batch)
        try:
            enc.set_copy("all")
            enc.submit_transcode(files)
            if max_batch == 1:
                with pytest_raises(M, M.ETOOSMALL, "does not fit"):
                    enc.collect()
                assert enc.jpeg_size(0) == len(ref) and enc.get_jpeg(0) == ref
            else:
                assert enc.collect() == [reference(f, "all") for f in four]
        finally:
            enc.close()


# ---- 7. batch ---------------------------------------------------------------------------------------------------------------------
def check_batch(M, progressive_sources):
    a = rich()
    b = behind_app0(base("16x16b"), seg(0xED, b"Photoshop 3.0\0" + blob(31, 5)))
    c = base("16x16")
    d = exif_first("16x16", True)
    info = M.jpeg_info(c)
    o, n = info.scans[0].data_offset, info.scans[0].data_size
    bad = behind_app0(c[:o + n // 2] + c[o + n // 2 + 8:], seg(COM, b"damaged"))      # entropy-coded bytes missing, every marker in place
    files = [a, b, bad, c, d]
    if progressive_sources:
        files.append(behind_app0(base("16x16_prog"), seg(COM, b"progressive") + icc_segments(ICC_IN_FILE)))
    outs = run(M, files, "all", "revert_opt", max_batch=8, progressive_sources=progressive_sources)
    for k, (f, r) in enumerate(zip(files, outs)):
        if k == 2:
            assert isinstance(r, M.MjhError) and r.code == M.EINVAL, r
        else:
            same(r, reference(f, "all", "revert_opt"), "file %d" % k)


# ---- 8. encode side ---------------------------------------------------------------------------------------------------------------
ENCODE_CASES = {
    "baseline": (dict(baseline=True), O.ref_switches(baseline=True)),
    "progressive": (dict(), O.ref_switches()),
    "arithmetic": (dict(arithmetic=True), O.ref_switches(arithmetic=True)),
    "lossless": (dict(revert=True, lossless=(1, 0)), ["-revert", "-lossless", "1,0"]),
}


def cjpeg_icc(img, args, icc):
    if icc is None:
        return TC.cjpeg(img, args)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "profile.icc")
        with open(path, "wb") as f:
            f.write(icc)
        return TC.cjpeg(img, list(args) + ["-icc", path])


def check_encode(M, name):
    kw, args = ENCODE_CASES[name]
    frames = np.stack([O.synthetic_frame(16, 16, 31), O.synthetic_frame(16, 16, 32)])
    enc = M.Encoder(M.make_params(16, 16, **kw), max_batch=2)
    try:
        plain = [cjpeg_icc(f, args, None) for f in frames]
        assert enc.encode_host(frames) == plain
        for n in (3000, 70000):                       # one segment, two segments
            icc = blob(n, n)
            enc.set_icc_profile(icc)
            outs = enc.encode_host(frames)
            for f, o in zip(frames, outs):
                same(o, cjpeg_icc(f, args, icc), "%s, a profile of %d bytes" % (name, n))
            assert enc.jpeg_size(1) == len(outs[1])
        enc.set_icc_profile(None)
        assert enc.encode_host(frames) == plain
    finally:
        enc.close()


def check_encode_without_hand_over(M):
    """the entry points whose files are fetched from device memory one by one (planes in): no hand-over kernel runs, the profile is
    put in on the host.  Expected: the encoder's own file without a profile, with the APP2 segments behind its SOI + JFIF APP0 --
    where check_encode shows cjpeg -icc puts them."""
    planes = [np.stack([O.synthetic_frame(w, w, 40 + k)[:, :, 0] for k in range(2)]) for w in (16, 8, 8)]
    enc = M.Encoder(M.make_params(16, 16, baseline=True), max_batch=2)
    try:
        plain = enc.encode_planes_host(planes)
        assert all(p[2:4] == b"\xff\xe0" and p[20:22] == b"\xff\xdb" for p in plain)
        icc = blob(70000, 7)
        enc.set_icc_profile(icc)
        outs = enc.encode_planes_host(planes)
        for p, o in zip(plain, outs):
            same(o, p[:20] + icc_segments(icc) + p[20:], "planes in")
        assert [enc.jpeg_size(i) for i in range(2)] == [len(o) for o in outs]
        enc.set_icc_profile(None)
        assert enc.encode_planes_host(planes) == plain
    finally:
        enc.close()


# ---- 9. API -----------------------------------------------------------------------------------------------------------------------
def check_jpeg_markers(M):
    codes = lambda mode: [m for m, _ in M.jpeg_markers(rich(), mode)]
    assert codes("none") == [] and codes("comments") == [COM, COM] and codes("icc") == [0xE2, 0xE2]
    assert codes("all") == [APP0, COM, 0xE1, 0xEC, 0xE2, 0xE2, COM, APP0] and codes("all_except_icc") == [APP0, COM, 0xE1, 0xEC, COM, APP0]
    assert codes(2) == codes("all")
    got = M.jpeg_markers(rich(), "all")
    assert got[1] == (COM, b"a comment") and got[6] == (COM, b"") and got[7][1][:5] == b"JFXX\0"
    assert b"".join(d[14:] for m, d in got if m == 0xE2) == ICC_IN_FILE
    with pytest_raises(M, M.EINVAL, "8 markers"):
        M.jpeg_markers(rich(), "all", cap=3)
    assert len(M.jpeg_markers(rich(), "all", cap=8)) == 8
    with pytest_raises(M, M.EINVAL, "copy mode"):
        M.jpeg_markers(rich(), 9)
    prog = behind_app0(base("16x16_prog"), seg(COM, b"p"))
    with pytest_raises(M, M.EUNSUPPORTED, "progressive"):      # refused as the probe refuses it
        M.jpeg_markers(prog, "all")
    assert M.jpeg_markers(prog, "comments", progressive_sources=True) == [(COM, b"p")]


class pytest_raises:
    """with pytest_raises(M, code, word): the block raises MjhError with that code and the word in its text"""

    def __init__(self, M, code, word):
        self.M, self.code, self.word = M, code, word

    def __enter__(self):
        return self

    def __exit__(self, typ, exc, tb):
        assert typ is not None and issubclass(typ, self.M.MjhError), "no MjhError was raised"
        assert exc.code == self.code and self.word in str(exc), exc
        return True


def check_encoder_api(M):
    import ctypes as C
    src = rich()
    enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=1)
    try:
        base_ptr, stride, sizes = C.c_void_p(), C.c_size_t(), C.c_void_p()
        view = lambda: M.lib().mjh_get_output_device(enc._h, C.byref(base_ptr), C.byref(stride), C.byref(sizes))
        assert enc.transcode_host([src]) == [reference(src, "none")]
        assert view() == M.OK and base_ptr.value
        with pytest_raises(M, M.EINVAL, "copy mode"):
            enc.set_copy(5)
        with pytest_raises(M, M.EINVAL, "copy mode"):
            enc.set_copy("everything")
        enc.set_copy("comments")
        assert view() == M.EUNSUPPORTED and b"hand-over" in M.lib().mjh_last_error()
        assert enc.transcode_host([src]) == [reference(src, "comments")]
        assert enc.jpeg_size(0) == len(reference(src, "comments"))
        enc.set_copy("none")
        assert view() == M.OK
        with pytest_raises(M, M.EINVAL, "0 bytes"):
            enc.set_icc_profile(b"")
        with pytest_raises(M, M.EINVAL, "256"):
            enc.set_icc_profile(bytes(255 * 65519 + 1))
        enc.set_icc_profile(bytes(1000))
        assert view() == M.EUNSUPPORTED
        enc.set_icc_profile(None)
        assert view() == M.OK
        assert enc.transcode_host([src]) == [reference(src, "none")]
    finally:
        enc.close()
