"""The case lists and checks of the lossless-decoder tests (test_simt_lossless_decode.py on the emulator, test_gpu_lossless_decode.py
on the chip).

Sources are made at test time by the reference: `oracle/_ref/cjpeg -revert -lossless psv,pt [-precision N] [-restart R] [-scans FILE]`
on the images of lossless_cases.image().  The expected samples are the payload of `oracle/_ref/djpeg -pnm` on that file, compared
for exact equality including shape and dtype, and -- independently -- (image >> pt) << pt, which the reference satisfies on its
own.  Nothing expected comes from the code under test."""
import ctypes
import functools
import os
import struct
import subprocess
import tempfile

import numpy as np

import lossless_cases as LC
import lossless_script_cases as LS
import oracle_lib as O

DJPEG = os.path.join(O.REF_DIR, "djpeg")


def have_tools():
    return os.path.exists(LC.CJPEG) and os.path.exists(DJPEG)


def parse_pnm(data):
    """[H, W] (P5) or [H, W, 3] (P6) of a binary PNM file: uint8 for maxval 255, uint16 (the file holds big-endian words) above"""
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
    assert magic in (b"P5", b"P6") and maxval in (255, 4095, 65535), (magic, maxval)
    c = 3 if magic == b"P6" else 1
    dt = np.dtype(np.uint8) if maxval == 255 else np.dtype(">u2")
    assert len(data) == pos + w * h * c * dt.itemsize
    a = np.frombuffer(data, dt, w * h * c, pos).astype(np.uint8 if maxval == 255 else np.uint16)
    return a.reshape((h, w, 3) if c == 3 else (h, w))


def djpeg_run(jpeg, args=()):
    """(exit status, samples or None, stderr) of the reference's djpeg -pnm"""
    with tempfile.TemporaryDirectory() as td:
        inp, outp = os.path.join(td, "in.jpg"), os.path.join(td, "out.pnm")
        with open(inp, "wb") as f:
            f.write(jpeg)
        r = subprocess.run([DJPEG, "-pnm"] + list(args) + ["-outfile", outp, inp], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        pix = None
        if r.returncode == 0 and os.path.exists(outp):
            with open(outp, "rb") as f:
                pix = parse_pnm(f.read())
        return r.returncode, pix, r.stderr.decode(errors="replace")


def djpeg(jpeg, args=()):
    status, pix, err = djpeg_run(jpeg, args)
    assert status == 0 and pix is not None, "djpeg exited with %d: %s" % (status, err)
    return pix


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


# ---- the cases.  A plain case is lossless_cases' tuple (kind, h, w, comps, precision, psv, pt, restart rows); a script case has the
# name of a script of lossless_script_cases in place of (psv, pt).
def _geometry():
    out = [("random", 1, 1, 3, 8, 1, 0, None), ("random", 1, 37, 1, 8, 2, 0, None), ("random", 53, 1, 3, 8, 3, 0, None),
           ("random", 1, 1, 1, 16, 7, 0, None), ("random", 2, 1, 1, 8, 5, 0, None)]
    k = 0
    for w in (63, 64, 65, 130):            # the wave and the 8-column chunk / 512-column tile edges
        for h in (2, 64, 65, 130):         # the 63-row strips of the wavefront and their hand-over
            out.append(("random", h, w, 3 if k % 2 else 1, 8, 1 + k % 7, 0, None))
            k += 1
    return out


GEOMETRY = _geometry()
# every predictor on 65 x 65 and 130 x 3, gray and RGB; and on 3 x 130, where a column crosses two strip hand-overs
PREDICTORS = [("random", h, w, c, 8, psv, 0, None) for psv in range(1, 8) for (h, w) in ((65, 65), (3, 130)) for c in (1, 3)] + \
             [("random", 130, 3, 1, 8, psv, 0, None) for psv in range(2, 8)]
# one row per interval, 3 rows on 29 (a short last interval), none; a predictor of every class (the scan, the linear ones, the shifted ones)
RESTARTS = [("smooth" if psv == 4 else "random", 29, 47, c, 8, psv, 0, r) for psv in (1, 4, 6) for r in (1, 3, None) for c in (1, 3)] + \
           [("random", 140, 20, 1, 8, 7, 0, 70)]          # an interval longer than a strip
PRECISIONS = [("random", 21, 33, 3, 8, 1, 0, None), ("random", 21, 33, 1, 8, 5, 7, None),
              ("random", 21, 33, 1, 12, 2, 0, None), ("random", 21, 33, 3, 12, 6, 11, 2),
              ("random", 19, 25, 3, 16, 4, 0, None), ("random", 19, 25, 1, 16, 7, 15, None), ("smooth", 19, 25, 3, 16, 3, 3, 5),
              ("extreme", 11, 41, 3, 16, 1, 0, None), ("extreme", 11, 41, 1, 16, 1, 0, 1), ("extreme", 9, 40, 1, 12, 7, 0, None),
              ("extreme", 9, 40, 3, 12, 7, 1, 2)]
SCRIPTS = [("smooth", 29, 47, 3, 8, "each", None), ("random", 29, 47, 3, 8, "each_mixed", None), ("random", 29, 47, 3, 8, "two_one", 1),
           ("smooth", 67, 70, 3, 8, "one_two", 2), ("random", 21, 33, 3, 12, "each_mixed", 3), ("random", 19, 25, 3, 16, "two_one", None),
           ("random", 19, 25, 1, 16, "gray_one", 5), ("random", 70, 9, 3, 8, "each_mixed", None)]
SYNC_CASE = ("random", 31, 1300, 3, 8, 1, 0, None)


def case_id(c):
    return LC.case_id(c) if isinstance(c[5], int) else LS.case_id(c)


@functools.lru_cache(maxsize=None)
def case_image(c):
    kind, h, w, comps, prec = c[:5]
    return LC.image(kind, h, w, comps, prec, seed=h * 131 + w)


@functools.lru_cache(maxsize=None)
def source(c):
    """the reference's file of a case"""
    a = case_image(c)
    if isinstance(c[5], int):
        f = LC.reference(a, c[5], c[6], c[4], c[7])
    else:
        f = LS.reference(a, LS.script_of(c[5]), c[4], c[6])
    assert isinstance(f, bytes), f
    return f


def point_transforms(c):
    """per component"""
    if isinstance(c[5], int):
        return [c[6]] * c[3]
    pts = [0] * c[3]
    for comps, _, al in LS.script_of(c[5]):
        for ci in comps:
            pts[ci] = al
    return pts


def shifted(a, pts):
    """(image >> pt) << pt per component, in the shape decode() returns"""
    out = a.copy()
    for ci, pt in enumerate(pts):
        out[:, :, ci] = (a[:, :, ci] >> pt) << pt
    return out[:, :, 0] if a.shape[2] == 1 else out


@functools.lru_cache(maxsize=None)
def expected(c):
    """djpeg's samples of the case's file; they are the image's own, point-transformed"""
    ref = djpeg(source(c))
    assert same(ref, shifted(case_image(c), point_transforms(c))), "the reference does not return the image: %s" % case_id(c)
    ref.setflags(write=False)
    return ref


def decode1(M, f, **kw):
    out = M.decode([f], lossless_sources=True, **kw)
    assert len(out) == 1
    if isinstance(out[0], Exception):
        raise out[0]
    return out[0]


def check_case(M, c):
    out = decode1(M, source(c))
    ref = expected(c)
    assert same(out, ref), "%s: %s %s, the reference %s %s, first difference at %s" % (
        case_id(c), out.shape, out.dtype, ref.shape, ref.dtype, np.argwhere(out != ref)[:1].tolist() if out.shape == ref.shape else "-")


# ---- files the reference's encoder does not write: marker segments patched by hand -----------------------------------------------
def segments(jpeg):
    """[(marker code, offset of the 0xFF, segment length with the two length bytes)] up to and including the first SOS"""
    out, pos = [], 2
    while pos + 4 <= len(jpeg):
        assert jpeg[pos] == 0xFF
        m, ln = jpeg[pos + 1], struct.unpack(">H", jpeg[pos + 2:pos + 4])[0]
        out.append((m, pos, ln))
        if m == 0xDA:
            break
        pos += 2 + ln
    return out


def all_segments(jpeg, info_scans):
    """every marker segment of a file of several scans: the walk of segments() resumed behind every scan's data"""
    out, start = [], 2
    for s in list(info_scans) + [None]:
        pos = start
        while pos + 4 <= len(jpeg) and jpeg[pos + 1] != 0xD9:
            m, ln = jpeg[pos + 1], struct.unpack(">H", jpeg[pos + 2:pos + 4])[0]
            out.append((m, pos, ln))
            pos += 2 + ln
            if m == 0xDA:
                break
        if s is None:
            break
        start = s.data_offset + s.data_size
    return out


def with_dri(jpeg, interval):
    """the file with its DRI set to `interval` MCUs (there must be one)"""
    b = bytearray(jpeg)
    (pos,) = [p for m, p, _ in segments(jpeg) if m == 0xDD]
    b[pos + 4:pos + 6] = struct.pack(">H", interval)
    return bytes(b)


def with_sof(jpeg, marker=None, sampling0=None):
    b = bytearray(jpeg)
    (pos,) = [p for m, p, _ in segments(jpeg) if m == 0xC3]
    if marker is not None:
        b[pos + 1] = marker
    if sampling0 is not None:
        b[pos + 11] = sampling0             # Hi / Vi of the first component
    return bytes(b)


def with_table_slots(M, jpeg):
    """a file of one scan per component whose scans k = 0, 1, 2 define and name DC table k (cjpeg uses slot 0 throughout)"""
    scans = M.jpeg_info(jpeg, lossless_sources=True).lossless_scans
    b = bytearray(jpeg)
    k = -1
    for m, pos, ln in all_segments(jpeg, scans):
        if m == 0xC4:
            k += 1
            assert b[pos + 4] == 0x00
            b[pos + 4] = k                  # Tc = 0, Th = k
        elif m == 0xDA:
            assert b[pos + 4] == 1 and b[pos + 6] == 0x00
            b[pos + 6] = k << 4             # Td = k
    assert k == 2
    return bytes(b)


def check_table_slots(M):
    c = ("random", 29, 47, 3, 8, "each_mixed", None)
    f = with_table_slots(M, source(c))
    assert f != source(c)
    info = M.jpeg_info(f, lossless_sources=True)
    assert [s.dc_tbl_no[0] for s in info.lossless_scans] == [0, 1, 2]
    assert same(decode1(M, f), djpeg(f)) and same(djpeg(f), expected(c))


# ---- what the probe reports ---------------------------------------------------------------------------------------------------------
def check_probe(M):
    c = ("random", 21, 33, 3, 12, "each_mixed", 3)
    info = M.jpeg_info(source(c), lossless_sources=True)
    assert (info.sof_type, info.data_precision, info.num_scans, info.num_components) == (3, 12, 0, 3)
    assert (info.image_width, info.image_height, info.jpeg_color_space) == (33, 21, M.CS_RGB)
    script = LS.script_of("each_mixed")
    assert [(tuple(s.component_index[:s.comps_in_scan]), s.Ss, s.Se, s.Ah, s.Al) for s in info.lossless_scans] == [(comps, ss, 0, 0, al) for comps, ss, al in script]
    assert all(s.restart_interval == 3 * 33 for s in info.lossless_scans)
    assert (info.lossless_psv, info.lossless_pt) == script[0][1:]
    both = M.jpeg_info(source(c), progressive_sources=True, lossless_sources=True)
    assert both.sof_type == 3 and len(both.lossless_scans) == 3 and both.prog_scans == []
    # the parameters of such a file are the lossless ones of its first scan
    p = M.params_from_jpeg(source(c), revert=True, lossless_sources=True)
    assert (p.image_width, p.image_height, p.num_components, p.data_precision, p.color_transform) == (33, 21, 3, 12, M.COLOR_NONE)
    assert p.num_scans == 1 and (p.scan_info[0].comps_in_scan, p.scan_info[0].Ss, p.scan_info[0].Se, p.scan_info[0].Ah, p.scan_info[0].Al) == (3, 5, 0, 0, 0)
    g = M.params_from_jpeg(source(("random", 19, 25, 1, 16, 7, 15, None)), revert=True, lossless_sources=True)
    assert (g.num_components, g.input_components, g.data_precision, g.scan_info[0].Ss, g.scan_info[0].Al) == (1, 1, 16, 7, 15)
    # a sequential or progressive file gives the same result with or without the bit
    import transcode_cases as TC
    for name, prog in (("revert", False), ("progressive", True)):
        f = TC.source(name) if not prog else TC.cjpeg(TC.testorig(), TC.REFUSALS["progressive"][0])
        a, b = M.jpeg_info(f, progressive_sources=prog), M.jpeg_info(f, progressive_sources=prog, lossless_sources=True)
        assert bytes(a) == bytes(b) and (b.lossless_psv, b.lossless_pt) == (0, 0) and b.lossless_scans == []


# ---- synchronisation ----------------------------------------------------------------------------------------------------------------
def check_sync(M):
    """a noise file whose one entropy-coded segment spans many subsequences"""
    f = source(SYNC_CASE)
    info = M.jpeg_info(f, lossless_sources=True)
    assert len(info.lossless_scans) == 1 and info.lossless_scans[0].restart_markers == 0
    enc = M.Encoder(M.params_from_jpeg(info, revert=True), max_batch=1)
    try:
        enc.set_sources(progressive=False, lossless=True)
        out = enc.decode_host([f])[0]
        st = enc.transcode_stats()
        assert 0 < st["subseq"] and 64 * st["subseq"] < info.lossless_scans[0].data_size and st["rounds"] > 1, st
        assert same(out, expected(SYNC_CASE))
    finally:
        enc.close()


# ---- batches -----------------------------------------------------------------------------------------------------------------------
BATCH = [("random", 29, 47, 3, 8, 1, 0, None), ("random", 29, 47, 3, 8, 7, 2, 1), ("random", 29, 47, 3, 8, "each_mixed", None),
         ("random", 29, 47, 3, 8, 4, 0, 3), ("random", 29, 47, 3, 8, "two_one", 1)]


def check_batch(M):
    """5 files of one geometry that differ in predictor, point transform, script and restart interval, 4 per call: two calls"""
    files = [source(c) for c in BATCH]
    assert len(set(files)) == 5
    out = M.decode(files, lossless_sources=True, max_batch=4)
    for c, o in zip(BATCH, out):
        assert not isinstance(o, Exception), (case_id(c), o)
        assert same(o, expected(c)), case_id(c)


def check_encoder_reuse(M):
    """one encoder, a call with one set of predictors, then another"""
    enc = M.Encoder(M.params_from_jpeg(source(BATCH[0]), revert=True, lossless_sources=True), max_batch=3)
    try:
        enc.set_sources(progressive=False, lossless=True)
        for part in (BATCH[:3], BATCH[3:], BATCH[1:2]):
            out = enc.decode_host([source(c) for c in part])
            for c, o in zip(part, out):
                assert same(o, expected(c)), case_id(c)
    finally:
        enc.close()


def check_mixed_kinds(M):
    """a lossless file and a sequential file of another geometry through one decode() call"""
    import decode_cases as DC
    import transcode_cases as TC
    seq = TC.source("revert")
    c = BATCH[1]
    out = M.decode([source(c), seq], lossless_sources=True)
    assert same(out[0], expected(c))
    assert same(out[1], DC.djpeg(seq))


# ---- layouts -----------------------------------------------------------------------------------------------------------------------
LAYOUT_CASES = [("random", 21, 33, 3, 8, 5, 0, None), ("random", 19, 25, 3, 16, 4, 0, None)]


def check_layouts(M, c):
    """the reference's RGB rearranged; the fourth sample is the sample maximum (_MAXJSAMPLE, jdcolext.c)"""
    rgb = expected(c)
    top = (1 << c[4]) - 1
    f = source(c)
    for layout in ("bgrx", "xrgb", "bgr", "rgbx"):
        px, off = M.PIXEL_LAYOUTS[layout]
        out = decode1(M, f, layout=layout)
        assert out.shape == rgb.shape[:2] + (px,) and out.dtype == rgb.dtype, layout
        for k in range(3):
            assert np.array_equal(out[:, :, off[k]], rgb[:, :, k]), layout
        if px == 4:
            assert (out[:, :, 6 - sum(off)] == top).all(), layout
    assert same(decode1(M, f, bottom_up=True), rgb[::-1])
    assert same(decode1(M, f, layout="bgrx", bottom_up=True)[:, :, :3], rgb[::-1, :, ::-1])
    g = ("random", 21, 33, 1, 12, 2, 0, None)
    assert same(decode1(M, source(g), bottom_up=True), expected(g)[::-1])


def check_ignored_options(M):
    """djpeg leaves a lossless file at full size whatever -scale, -nosmooth and -dct say"""
    c = LAYOUT_CASES[0]
    ref = expected(c)
    assert same(djpeg(source(c), ["-scale", "1/2", "-nosmooth", "-dct", "fast"]), ref)
    assert same(decode1(M, source(c), scale="1/2", fancy_upsampling=False, dct="fast"), ref)


DEVICE_CASES = [(("random", 21, 33, 1, 8, 5, 7, None), {}), (("random", 21, 33, 1, 12, 2, 0, None), {}), (("random", 21, 33, 3, 8, 5, 0, None), {}),
                (("random", 19, 25, 3, 16, 4, 0, None), {}), (("random", 19, 25, 3, 16, 4, 0, None), dict(layout="xrgb")),
                (("random", 21, 33, 3, 8, 5, 0, None), dict(layout="bgrx"))]


def check_pixels_device(M, read_device):
    """mjh_get_pixels_device against mjh_get_pixels at 1, 2, 3, 6, 8 and 4 bytes per pixel: rows of whole groups of four pixels, 16-byte
    aligned.  read_device(pointer, bytes) -> bytes"""
    seen = set()
    for c, kw in DEVICE_CASES:
        f = source(c)
        enc = M.Encoder(M.params_from_jpeg(f, revert=True, lossless_sources=True), max_batch=2)
        try:
            enc.set_sources(progressive=False, lossless=True)
            host = enc.decode_host([f, f], **kw)
            enc.submit_decode([f, f], **kw)
            enc.wait_decode()
            ptr, pitch, stride, st = enc.pixels_device()
            h, w, px = st["height"], st["width"], st["pixel_size"]
            seen.add(px)
            assert (h, w) == c[1:3] and px == host[0].itemsize * (host[0].shape[2] if host[0].ndim == 3 else 1)
            assert pitch == (px * ((w + 3) & ~3) + 15) & ~15 and stride == pitch * h and ptr % 16 == 0
            raw = np.frombuffer(read_device(ptr, 2 * stride), np.uint8).reshape(2, h, pitch)
            for i in range(2):
                got = np.ascontiguousarray(raw[i, :, :w * px]).view(host[i].dtype).reshape(host[i].shape)
                assert np.array_equal(got, host[i]), (case_id(c), kw, i)
        finally:
            enc.close()
    assert seen == {1, 2, 3, 4, 6, 8}


# ---- opt-in and refusals ------------------------------------------------------------------------------------------------------------
def _refused(M, x, code, word):
    assert isinstance(x, M.MjhError) and x.code == code and word.lower() in str(x).lower(), (x, code, word)


def _raises(M, fn, code, word):
    try:
        fn()
    except M.MjhError as exc:
        _refused(M, exc, code, word)
        return
    raise AssertionError("not refused (%s)" % word)


def check_default_refusals(M):
    """without the keyword a lossless file is answered as before the feature: EUNSUPPORTED with the word lossless"""
    f = source(BATCH[0])
    _raises(M, lambda: M.jpeg_info(f), M.EUNSUPPORTED, "lossless source file (SOF3)")
    _raises(M, lambda: M.jpeg_info(f, progressive_sources=True), M.EUNSUPPORTED, "lossless source file (SOF3)")
    _raises(M, lambda: M.params_from_jpeg(f, revert=True), M.EUNSUPPORTED, "lossless")
    for fn in (M.decode, M.decode_planes, M.decode_coefficients, M.recompress):
        _refused(M, fn([f])[0], M.EUNSUPPORTED, "lossless")
        _refused(M, fn([f], progressive_sources=True)[0], M.EUNSUPPORTED, "lossless")


def check_refusals(M):
    """with the keyword: what stays refused, each with its code and word"""
    rgb, gray = source(BATCH[0]), source(("random", 21, 33, 1, 8, 5, 7, None))
    kw = dict(lossless_sources=True)
    _refused(M, M.decode([rgb], color="gray", **kw)[0], M.EUNSUPPORTED, "color conversion")
    _refused(M, M.decode([gray], color="rgb", **kw)[0], M.EUNSUPPORTED, "color conversion")
    _refused(M, M.decode([rgb], color="rgb565", **kw)[0], M.EUNSUPPORTED, "RGB565")
    _refused(M, M.decode([gray], color="rgb565", **kw)[0], M.EUNSUPPORTED, "RGB565")
    _refused(M, M.decode_planes([rgb], **kw)[0], M.EUNSUPPORTED, "raw_planes")
    _refused(M, M.decode_coefficients([rgb], **kw)[0], M.EUNSUPPORTED, "raw_coefs")
    _refused(M, M.recompress([rgb], **kw)[0], M.EUNSUPPORTED, "lossless source file (SOF3)")
    # the reference's djpeg refuses the conversions in these words
    for f, sw in ((rgb, "-grayscale"), (gray, "-rgb"), (rgb, "-rgb565")):
        status, _, err = djpeg_run(f, [sw])
        assert status != 0 and "Unsupported color conversion request" in err, (sw, err)
    # the library itself: a lossless encoder re-compresses nothing, a DCT encoder takes no lossless file
    enc = M.Encoder(M.params_from_jpeg(rgb, revert=True, lossless_sources=True), max_batch=1)
    try:
        enc.set_sources(progressive=False, lossless=True)
        _raises(M, lambda: enc.transcode_host([rgb]), M.EINVAL, "lossless encoder")
    finally:
        enc.close()
    # an encoder for such files that set_sources was not called on still refuses them
    enc = M.Encoder(LC.params(M, case_image(BATCH[0]), 1, 0, 8), max_batch=1)
    try:
        _raises(M, lambda: enc.decode_host([rgb]), M.EUNSUPPORTED, "lossless source file (SOF3)")
    finally:
        enc.close()
    import transcode_cases as TC
    seq = TC.source("revert")
    enc = M.Encoder(M.params_from_jpeg(seq, revert=True), max_batch=2)
    try:
        enc.set_sources(progressive=True, lossless=True)
        for call in (lambda: enc.transcode_host([rgb, seq]), lambda: enc.decode_host([rgb, seq])):
            _raises(M, call, M.EUNSUPPORTED, "lossless source file (SOF3)")
    finally:
        enc.close()
    # a restart interval that is not whole rows: JERR_BAD_RESTART in the reference (jddiffct.c), MJH_EINVAL here
    r3 = source(("random", 29, 47, 3, 8, 4, 0, 3))
    bad = with_dri(r3, 3 * 47 + 1)
    status, _, err = djpeg_run(bad)
    assert status != 0 and "Invalid restart interval" in err, err
    _refused(M, M.decode([bad], **kw)[0], M.EINVAL, "Invalid restart interval")
    _raises(M, lambda: M.jpeg_info(bad, lossless_sources=True), M.EINVAL, "JERR_BAD_RESTART")
    # arithmetic-coded lossless, a subsampled component, a precision the reference refuses, a predictor outside 1..7
    _refused(M, M.decode([with_sof(rgb, marker=0xCB)], **kw)[0], M.EUNSUPPORTED, "arithmetic")
    _refused(M, M.decode([with_sof(rgb, sampling0=0x21)], **kw)[0], M.EUNSUPPORTED, "subsampled")
    _refused(M, M.decode([with_sof(gray, sampling0=0x21)], **kw)[0], M.EUNSUPPORTED, "subsampled")
    b = bytearray(rgb)
    (pos,) = [p for m, p, _ in segments(rgb) if m == 0xC3]
    b[pos + 4] = 10
    _refused(M, M.decode([bytes(b)], **kw)[0], M.EINVAL, "JERR_BAD_PRECISION")
    b = bytearray(rgb)
    (pos, ln), = [(p, n) for m, p, n in segments(rgb) if m == 0xDA]
    b[pos + 2 + ln - 3] = 8                # Ss
    _refused(M, M.decode([bytes(b)], **kw)[0], M.EINVAL, "JERR_BAD_PROGRESSION")
    # files of one call agree in size, component count and precision
    enc = M.Encoder(M.params_from_jpeg(rgb, revert=True, lossless_sources=True), max_batch=2)
    try:
        enc.set_sources(progressive=False, lossless=True)
        for other, word in ((source(("random", 21, 33, 3, 8, 1, 0, None)), "image size"), (source(("random", 29, 47, 1, 8, 1, 0, None)), "number of components"),
                            (LC.reference(LC.image("random", 29, 47, 3, 12, 5), 1, 0, 12), "data precision")):
            res = enc.decode_host([rgb, other], errors="return")
            assert res[0] is None
            _refused(M, res[1], M.EINVAL, word)
    finally:
        enc.close()


# ---- untrusted input (the emulator file only: its device buffers end at unmapped pages) --------------------------------------------------
def without_longest_code(jpeg):
    """the file with the symbol of the longest code taken out of its (only) Huffman table: an optimal table holds exactly the
    categories that occur, so the data then holds a code no table entry exists for"""
    (pos, ln), = [(p, n) for m, p, n in segments(jpeg) if m == 0xC4]
    bits = bytearray(jpeg[pos + 5:pos + 21])
    vals = jpeg[pos + 21:pos + 2 + ln]
    assert sum(bits) == len(vals) and len(vals) > 2
    last = max(i for i in range(16) if bits[i])
    bits[last] -= 1
    seg = b"\xff\xc4" + struct.pack(">H", ln - 1) + jpeg[pos + 4:pos + 5] + bytes(bits) + vals[:-1]
    return jpeg[:pos] + seg + jpeg[pos + 2 + ln:]


def damaged_files(M):
    c = ("random", 29, 47, 3, 8, 6, 0, None)
    f = source(c)
    s = M.jpeg_info(f, lossless_sources=True).lossless_scans[0]
    a, n = s.data_offset, s.data_size
    out = {"cut_40": f[:a + n // 2] + f[a + n // 2 + 40:],
           "end_in_last_row": f[:a + n - 12] + b"\xff\xd9",
           "missing_code": without_longest_code(f)}
    r = source(("random", 29, 47, 3, 8, 6, 0, 3))
    b = bytearray(r)
    at = r.index(b"\xff\xd1", M.jpeg_info(r, lossless_sources=True).lossless_scans[0].data_offset)
    b[at + 1] = 0xD3
    out["rst_out_of_sequence"] = bytes(b)
    return c, out


def check_damaged(M):
    """each gives an error for that file and the right samples for the other file of the batch"""
    c, files = damaged_files(M)
    good = BATCH[3]
    for name, f in files.items():
        out = M.decode([f, source(good)], lossless_sources=True, max_batch=2)
        _refused(M, out[0], M.EINVAL, "Corrupt JPEG data")
        assert same(out[1], expected(good)), name
        out = M.decode([source(good), f], lossless_sources=True, max_batch=2)
        _refused(M, out[1], M.EINVAL, "Corrupt JPEG data")
        assert same(out[0], expected(good)), name
    # a damaged file's slot of the device buffer holds zeros
    enc = M.Encoder(M.params_from_jpeg(source(good), revert=True, lossless_sources=True), max_batch=2)
    try:
        enc.set_sources(progressive=False, lossless=True)
        enc.submit_decode([files["cut_40"], source(good)])
        try:
            enc.wait_decode()
            raise AssertionError("a damaged batch was reported clean")
        except M.MjhError as exc:
            _refused(M, exc, M.EINVAL, "file 0")
        ptr, pitch, stride, st = enc.pixels_device()
        assert not any(ctypes.string_at(ptr, stride))
        second = np.frombuffer(ctypes.string_at(ptr + stride, stride), np.uint8).reshape(st["height"], pitch)[:, :st["width"] * 3].reshape(expected(good).shape)
        assert np.array_equal(second, expected(good))
    finally:
        enc.close()
