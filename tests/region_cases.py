"""The case list and helpers of the region-decode tests (test_simt_decode_region.py on the emulator, test_gpu_decode_region.py on
the chip): mjh_decode_opts.crop_x / crop_y / crop_w / crop_h, the reference's jpeg_crop_scanline + jpeg_skip_scanlines as
djpeg -crop WxH+X+Y drives them; k_idct_region, k_idct_region_scaled, k_upcolor_region and k_upcolor_565_region of mjh_idct.hip,
and the restart segments a region leaves out of the Huffman decoder.

Sources are those of scale_cases.py; the expected pixels always come from the reference's djpeg at test time
(oracle/_ref/djpeg -crop WxH+X+Y + switches), and every comparison is exact equality, shape and dtype included."""
import functools
import os
import subprocess
import tempfile

import numpy as np

import decode_cases as DC
import oracle_lib as O
import scale_all_cases as SA
import scale_cases as SC
import tj_decompress_cases as TD
import transcode_cases as TC

have_tools = SC.have_tools

SOURCES = ["revert", "s_mixed", "q90_2x1_r1", "s1x2", "gray_r5b", "17x9_2x1", "8x8_2x1", "1x1"]
# the region shapes, each the smallest at which its index path can go wrong (region_of makes the numbers from the file's geometry)
SHAPES = ["full", "right_edge", "x_aligned", "x_unaligned", "partial_mcu", "w1", "h1", "in_mcu", "y_on", "y_above", "y_below", "y0", "bottom", "chroma_w1"]

# mode -> (keywords of mozjpeg_amd.decode, djpeg's switches, the IDCT size k)
MODES = {
    "default": (dict(), [], 8),
    "nosmooth": (dict(fancy_upsampling=False), ["-nosmooth"], 8),
    "grayscale": (dict(color="gray"), ["-grayscale"], 8),
    "rgb": (dict(color="rgb"), ["-rgb"], 8),
    "fast": (dict(dct="fast"), ["-dct", "fast"], 8),
    "scale1_2": (dict(scale="1/2"), ["-scale", "1/2"], 4),
    "scale1_4": (dict(scale=(1, 4)), ["-scale", "1/4"], 2),
    "scale1_8": (dict(scale="1/8"), ["-scale", "1/8"], 1),
    "scale1_2_nosmooth": (dict(scale="1/2", fancy_upsampling=False), ["-scale", "1/2", "-nosmooth"], 4),
}
CASES = [(s, m) for s in SOURCES for m in ("default", "nosmooth", "fast", "scale1_2", "scale1_4", "scale1_8")]
CASES += [(s, "grayscale") for s in ("revert", "s_mixed", "q90_2x1_r1")]
CASES += [("gray_r5b", "rgb"), ("revert", "scale1_2_nosmooth"), ("17x9_2x1", "scale1_2_nosmooth")]
LAYOUT_SOURCES = ["revert", "q90_2x1_r1", "gray_r5b", "17x9_2x1"]
# (dither, scale) of the RGB565 cases: at 1/8 the iMCU column is 1 or 2 pixels wide, so a region starts at any column phase
MODES_565 = [(True, None), (False, None), (True, "1/8"), (False, "1/8")]
CASES_565 = [(s, d, sc) for s in LAYOUT_SOURCES for d, sc in MODES_565]


def case_id(c):
    return "-".join(str(v) for v in c).replace("/", "_")


def geometry(M, name, k):
    """(scaled width, scaled height, iMCU column width, iMCU row height) of a source at IDCT size k"""
    info = M.jpeg_info(SC.source(name))
    nc = info.num_components
    maxh = max(info.h_samp_factor[c] for c in range(nc)) if nc > 1 else 1
    maxv = max(info.v_samp_factor[c] for c in range(nc)) if nc > 1 else 1
    return -(-info.image_width * k // 8), -(-info.image_height * k // 8), k * maxh, k * maxv


def region_of(M, name, shape, k=8):
    """(x, y, w, h) of a named shape in the scaled image of a source, or None where the image has no such region"""
    W, H, mw, mh = geometry(M, name, k)
    yb = mh * min(3, (H - 1) // mh)                     # an iMCU boundary inside the image (0 for an image one iMCU row high)
    if shape == "full":
        return 0, 0, W, H
    if shape == "right_edge":
        return (0, 0, W // 2 + 1, H) if W > 1 else None
    if shape == "x_aligned":
        x = mw * min(2, (W - 1) // mw)
        return (x, 0, min(W - x, 2 * mw + 3), H) if x else None
    if shape == "x_unaligned":
        x = min(W - 1, mw + mw // 2 + 1)
        y = min(H - 1, 7)
        return (x, y, min(100, W - x), min(50, H - y)) if x % mw else None
    if shape == "partial_mcu":
        x = max(0, W - 3)
        return x, 0, W - x, H
    if shape == "w1":
        return min(W - 1, mw + 1), 0, 1, H
    if shape == "h1":
        return 0, min(H - 1, mh + 1), W, 1
    if shape == "in_mcu":
        x, y = min(W - 1, mw + 2), min(H - 1, mh + 2)
        return x, y, min(3, W - x), min(3, H - y)
    if shape in ("y_on", "y_above", "y_below"):
        y = yb + {"y_on": 0, "y_above": -1, "y_below": 1}[shape]
        return (0, y, W, min(mh + 1, H - y)) if 0 <= y < H and yb else None
    if shape == "y0":
        return 0, 0, W, min(5, H)
    if shape == "bottom":
        y = max(0, H - 5)
        return 0, y, W, H - y
    if shape == "chroma_w1":                            # luma 2 wide, chroma 1: the upsamplers are picked again (jdapistd.c:282)
        return (0, 0, 2, H) if name == "17x9_2x1" and k == 8 else None
    raise KeyError(shape)


def crop_arg(r):
    return "%dx%d+%d+%d" % (r[2], r[3], r[0], r[1])


def aligned(M, name, r, k=8):
    """the region jpeg_crop_scanline makes of r: x moved left to a multiple of the iMCU column width, the width grown by as much"""
    mw = geometry(M, name, k)[2]
    xe = r[0] // mw * mw
    return xe, r[1], r[2] + r[0] - xe, r[3]


@functools.lru_cache(maxsize=None)
def reference_file(jpeg, args):
    return DC.djpeg(jpeg, list(args))


def reference(name, r, switches=()):
    """djpeg -crop of a named source (r None: the whole image)"""
    return reference_file(SC.source(name), (() if r is None else ("-crop", crop_arg(r))) + tuple(switches))


CLIENT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "region_client")


def have_client():
    return have_tools() and os.path.exists(CLIENT) and os.path.exists(os.path.join(O.REF_DIR, "libjpeg.so.62"))


@functools.lru_cache(maxsize=None)
def client(jpeg, args, lib_dir=None):
    """(exit status, what it printed, the rows it read) of tests/native/region_client on the library in lib_dir (None: the
    reference's): jpeg_crop_scanline, jpeg_skip_scanlines, one row per jpeg_read_scanlines call, skip to the end, finish"""
    with tempfile.TemporaryDirectory() as td:
        inp, outp = os.path.join(td, "in.jpg"), os.path.join(td, "out.bin")
        with open(inp, "wb") as f:
            f.write(jpeg)
        env = dict(os.environ, LD_LIBRARY_PATH=lib_dir or O.REF_DIR)
        r = subprocess.run([CLIENT, inp, outp] + [str(a) for a in args], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        with open(outp, "rb") as f:
            return r.returncode, r.stdout.decode(errors="replace") + r.stderr.decode(errors="replace"), f.read()


def reference565(jpeg, r, dither, scale):
    """uint16 [h, w_eff] of the reference's library: JCS_RGB565 under jpeg_crop_scanline + jpeg_skip_scanlines, read row by row as
    djpeg reads (the reference's djpeg writes RGB565 as BMP only, and its BMP writer refuses -crop: "Unsupported output file format")"""
    num, denom = (int(v) for v in scale.split("/")) if scale else (1, 1)
    rc, text, rows = client(jpeg, (1, int(dither), num, denom, 1, r[0], r[2], r[1], r[3]))
    assert rc == 0 and "error" not in text, text
    return np.frombuffer(rows, "<u2").reshape(r[3], -1)


def run(M, jpeg, r, **kw):
    out = M.decode([jpeg], crop=r, **kw)[0]
    if isinstance(out, Exception):
        raise out
    return out


def regions(M, name, k):
    return [(sh, region_of(M, name, sh, k)) for sh in SHAPES if region_of(M, name, sh, k) is not None]


# ---- 1. every case against the reference ----------------------------------------------------------------------------------------------
def check_case(M, name, mode):
    kw, switches, k = MODES[mode]
    src = SC.source(name)
    seen = 0
    for shape, r in regions(M, name, k):
        ref = reference(name, r, switches)
        out = run(M, src, r, **kw)
        xe, y, we, h = aligned(M, name, r, k)
        assert out.shape[:2] == (h, we) == ref.shape[:2], "%s %s: %s, the reference %s" % (shape, r, out.shape, ref.shape)
        assert SC.same(out, ref), "%s %s" % (shape, r)
        out = run(M, src, crop_arg(r), **kw)            # the string form
        assert SC.same(out, ref), "%s %s" % (shape, crop_arg(r))
        seen += 1
    assert seen >= 5
    full = run(M, src, region_of(M, name, "full", k), **kw)
    whole = M.decode([src], **kw)[0]
    assert SC.same(full, whole) and SC.same(whole, reference(name, None, switches))


def check_layout(M, name):
    src = SC.source(name)
    for shape in ("x_unaligned", "in_mcu", "bottom", "w1"):
        r = region_of(M, name, shape)
        if r is None:
            continue
        rgb = reference(name, r, ("-rgb",))
        DC.check_layout(rgb, run(M, src, r, color="rgb", layout="bgrx"), "bgrx")
        DC.check_layout(rgb, run(M, src, r, color="rgb", layout="bgr"), "bgr")
        up = run(M, src, r, bottom_up=True)
        assert SC.same(up[::-1], reference(name, r))    # the flip is inside the region


def check_565(M, name, dither, scale):
    src = SC.source(name)
    k = 1 if scale else 8
    seen = 0
    for shape in ("x_aligned", "x_unaligned", "in_mcu", "w1", "y_below", "bottom", "right_edge"):
        r = region_of(M, name, shape, k)
        if r is None:
            continue
        ref = reference565(src, r, dither, scale)
        out = run(M, src, r, color="rgb565", dither=dither, scale=scale)
        assert SC.same(out, ref), "%s %s: %s %s, the reference %s" % (shape, r, out.shape, out.dtype, ref.shape)
        seen += 1
    assert seen >= 3


# ---- 2. the premise of the case list, from the reference alone -----------------------------------------------------------------------
def check_premise(M):
    """without fancy upsampling a region is a slice of the whole decode; with it, a crop edge strictly inside the image changes
    the columns beside it (4:2:0 and 4:2:2), which is why the cases compare with djpeg -crop and not with a slice"""
    for name, mode in CASES:
        kw, switches, k = MODES[mode]
        if "-nosmooth" not in switches:
            continue
        whole = reference(name, None, switches)
        for shape, r in regions(M, name, k):
            xe, y, we, h = aligned(M, name, r, k)
            assert SC.same(reference(name, r, switches), whole[y:y + h, xe:xe + we]), (name, mode, shape)
    for name in ("revert", "q90_2x1_r1"):
        whole = reference(name, None)
        r = region_of(M, name, "x_unaligned")
        xe, y, we, h = aligned(M, name, r)
        W = geometry(M, name, 8)[0]
        assert 0 < xe and xe + we < W
        ref = reference(name, r)
        cut = whole[y:y + h, xe:xe + we]
        assert ref.shape == cut.shape and not np.array_equal(ref, cut), name
        assert np.array_equal(ref[:, 2:-2], cut[:, 2:-2]), name       # ... and only there
    # the shape that picks the upsamplers again: chroma 1 wide under the crop, 9 wide without
    info = M.jpeg_info(SC.source("17x9_2x1"))
    r = region_of(M, "17x9_2x1", "chroma_w1")
    assert -(-r[2] * info.h_samp_factor[1] // info.h_samp_factor[0]) == 1 and -(-info.image_width // 2) > 2
    # x_unaligned moves: decode_region is checked against these numbers
    assert aligned(M, "revert", region_of(M, "revert", "x_unaligned")) != region_of(M, "revert", "x_unaligned")


# ---- 3. restart segments ------------------------------------------------------------------------------------------------------------
def restart_segments(M, jpeg):
    """[(first byte, end)] of the restart segments of a one-scan file's entropy-coded data"""
    sc = M.jpeg_info(jpeg).scans[0]
    a, b = sc.data_offset, sc.data_offset + sc.data_size
    out, start, q = [], a, a
    while q + 1 < b:
        if jpeg[q] == 0xFF and 0xD0 <= jpeg[q + 1] <= 0xD7:
            out.append((start, q))
            start = q = q + 2
        else:
            q += 1
    out.append((start, b))
    return out


def cut_segment(jpeg, seg):
    """the file with the middle half of one restart segment's bytes missing, every marker in place"""
    a, b = seg
    n = b - a
    assert n >= 8
    return jpeg[:a + n // 4] + jpeg[a + n // 4 + n // 2:]


def lower_half(M, name):
    W, H, mw, mh = geometry(M, name, 8)
    y = (H // 2 + mh) // mh * mh + 3
    return mw + 5, y, W - mw - 5 - 2, H - y - 1


def check_pruning(M):
    for name in ("q90_2x1_r1", "gray_r5b", "revert"):
        src = SC.source(name)
        r = lower_half(M, name)
        enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=1)
        out = enc.decode_host([src], crop=r)[0]
        assert SC.same(out, reference(name, r)), name
        assert enc.decode_region() == aligned(M, name, r)
        kept, total = enc.decode_segments()
        segs = restart_segments(M, src)
        assert total == len(segs), (name, total, len(segs))
        if name == "revert":
            assert kept == total == 1
        else:
            assert 0 < kept < total // 2 + 2, (name, kept, total)
        assert SC.same(enc.decode_host([src])[0], reference(name, None))
        assert enc.decode_segments() == (total, total)
        if name != "revert":
            # the first segment holds the image's first MCUs, which a region of the lower half does not read; the last one is read
            clean = enc.decode_host([cut_segment(src, segs[0])], crop=r)[0]
            assert SC.same(clean, reference(name, r)), name
            with SC.pytest_raises(M, M.EINVAL, "Corrupt"):
                enc.decode_host([cut_segment(src, segs[0])])
            # the segments of the image's last quarter hold MCUs of rows the region reads (rows decide, not columns)
            inside = max(segs[-(len(segs) // 4):], key=lambda s: s[1] - s[0])
            with SC.pytest_raises(M, M.EINVAL, "Corrupt"):
                enc.decode_host([cut_segment(src, inside)], crop=r)
            y_last = geometry(M, name, 8)[1] - 1
            with SC.pytest_raises(M, M.EINVAL, "Corrupt"):
                enc.decode_host([cut_segment(src, inside)], crop=(0, y_last // 2, 0, 0))
            assert SC.same(enc.decode_host([cut_segment(src, inside)], crop=(0, 0, 0, 20))[0], reference(name, (0, 0, geometry(M, name, 8)[0], 20)))
        enc.close()


# ---- 4. the other entropy coders ------------------------------------------------------------------------------------------------------
def check_other_entropy_coders(M):
    for src, kw in ((TD.progressive(), dict(progressive_sources=True)), (SA.arithmetic_source(), dict(arithmetic_sources=True))):
        r = (37, 21, 90, 70)
        out = M.decode([src], crop=r, **kw)[0]
        assert not isinstance(out, Exception), out
        assert SC.same(out, reference_file(src, ("-crop", crop_arg(r)))), sorted(kw)


# ---- 5. one encoder, many regions ----------------------------------------------------------------------------------------------------
def check_one_encoder(M):
    for name in ("revert", "q90_2x1_r1", "gray_r5b"):
        src = SC.source(name)
        W, H, mw, mh = geometry(M, name, 8)
        enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=1)
        steps = [((21, 9, 100, 60), None, 8), (None, None, 8), ((3, 70, 60, 41), None, 8), ((11, 5, 40, 33), "1/2", 4), (None, None, 8)]
        for r, scale, k in steps:
            sw = ("-scale", scale) if scale else ()
            out = enc.decode_host([src], crop=r, scale=scale)[0]
            assert SC.same(out, reference(name, r, sw)), (name, r, scale)
            st = enc.decode_stats()
            want = aligned(M, name, r, k) if r else (0, 0, W, H)
            assert enc.decode_region() == want and (st["width"], st["height"]) == want[2:] == out.shape[1::-1], (name, r, scale)
        enc.close()


# ---- 6. a batch with a damaged file; the device buffer --------------------------------------------------------------------------------
def check_batch(M, fetch):
    """fetch(ptr, nbytes) -> bytes of device memory"""
    files = DC.batch_files()
    files = [files[0], files[1], SC.damaged(files[0], M), files[2], files[1]]
    r = (19, 33, 150, 77)
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True), max_batch=5)
    res = enc.decode_host(files, errors="return", crop=r)
    assert [isinstance(v, M.MjhError) for v in res] == [False, False, True, False, False]
    assert res[2].code == M.EINVAL and "Corrupt" in str(res[2])
    good = [f for i, f in enumerate(files) if i != 2]
    outs = enc.decode_host(good, crop=r)
    for f, o in zip(good, outs):
        assert SC.same(o, reference_file(f, ("-crop", crop_arg(r))))
    outs = M.decode(files, crop=r, max_batch=5)
    assert isinstance(outs[2], M.MjhError) and outs[2].code == M.EINVAL and "Corrupt" in str(outs[2])
    for i in (0, 1, 3, 4):
        assert SC.same(outs[i], reference_file(files[i], ("-crop", crop_arg(r)))), i
    for kw in (dict(), dict(layout="bgrx"), dict(color="gray")):
        host = enc.decode_host(good[:2], crop=r, **kw)
        enc.submit_decode(good[:2], crop=r, **kw)
        enc.wait_decode()
        ptr, pitch, stride, st = enc.pixels_device()
        h, w, px = st["height"], st["width"], st["pixel_size"]
        assert (w, h) == aligned(M, "revert", r)[2:]
        assert pitch == (px * ((w + 3) & ~3) + 15) & ~15 and stride == pitch * h
        raw = np.frombuffer(fetch(ptr, stride * 2), np.uint8).reshape(2, h, pitch)
        for i in range(2):
            got = raw[i, :, :w * px].reshape((h, w, px) if px > 1 else (h, w))
            assert np.array_equal(got, host[i]), (sorted(kw), i)
    enc.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
def raw_opts(M, **fields):
    """a DecodeOpts with fields set WITHOUT the binding's own validation: what a C caller could pass"""
    o = M.DecodeOpts()
    M.lib().mjh_decode_opts_defaults(o)
    for k, v in fields.items():
        setattr(o, k, v)
    return o


def check_refusals(M):
    import cmyk_cases as CM
    import lossless_decode_cases as LD
    src = SC.source("revert")
    r = dict(crop_x=16, crop_y=8, crop_w=32, crop_h=16)
    enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=1)
    full = enc.decode_host([src])[0]
    for extra, word in ((dict(raw_planes=1), "raw_planes"), (dict(raw_coefs=1), "raw_coefs"), (dict(scale_num=3, scale_denom=8, all_scales=1), "all_scales")):
        with SC.pytest_raises(M, M.EUNSUPPORTED, word):
            enc.decode_host([src], opts=raw_opts(M, **dict(r, **extra)))
        assert M.lib().mjh_transcode_batch_size(enc._h) == 0
    for bad in (dict(crop_x=227, crop_w=1), dict(crop_x=200, crop_w=28), dict(crop_y=149), dict(crop_y=100, crop_h=50), dict(crop_x=227), dict(crop_w=228),
                dict(crop_x=2 ** 31 - 1, crop_w=2 ** 31 - 1)):
        with SC.pytest_raises(M, M.EINVAL, "exceeds the scaled image dimensions"):
            enc.decode_host([src], opts=raw_opts(M, **bad))
    with SC.pytest_raises(M, M.EINVAL, "exceeds the scaled image dimensions"):
        enc.decode_host([src], opts=raw_opts(M, scale_num=1, scale_denom=2, crop_x=100, crop_w=20))      # 114 wide at 1/2
    for bad in (dict(crop_x=-1, crop_w=4), dict(crop_w=-4), dict(crop_y=-1), dict(crop_h=-1)):
        with SC.pytest_raises(M, M.EINVAL, "negative"):
            enc.decode_host([src], opts=raw_opts(M, **bad))
    # to the right / bottom edge
    assert SC.same(enc.decode_host([src], opts=raw_opts(M, crop_x=200, crop_y=140))[0], reference("revert", (200, 140, 27, 9)))
    assert SC.same(enc.decode_host([src], opts=raw_opts(M))[0], full)               # the defaulted struct
    o = M.DecodeOpts()                                                              # the zeroed one: no fancy upsampling
    assert (o.crop_x, o.crop_y, o.crop_w, o.crop_h) == (0, 0, 0, 0)
    assert SC.same(enc.decode_host([src], opts=o)[0], DC.reference("revert", "nosmooth"))
    assert enc.decode_region() == (0, 0, 227, 149)
    enc.close()
    for kw, code, word in ((dict(crop=(0, 0, 8, 8), raw_planes=True), M.EUNSUPPORTED, "raw_planes"), (dict(crop=(0, 0, 8, 8), raw_coefs=True), M.EUNSUPPORTED, "raw_coefs"),
                           (dict(crop=(0, 0, 8, 8), scale="3/8", all_scales=True), M.EUNSUPPORTED, "all_scales"), (dict(crop=(0, 0, 8, 8), scale="3/8"), M.EUNSUPPORTED, "3x3"),
                           (dict(crop="8x8"), M.EINVAL, "crop"), (dict(crop=(1, 2, 3)), M.EINVAL, "crop"), (dict(crop=(-1, 0, 4, 4)), M.EINVAL, "negative")):
        with SC.pytest_raises(M, code, word):
            M.decode_opts(**kw)
    enc = M.Encoder(M.params_from_jpeg(src, revert=True, transform="flip_h"), max_batch=1)
    with SC.pytest_raises(M, M.EUNSUPPORTED, "transform"):
        enc.decode_host([src], crop=(0, 0, 8, 8))
    enc.close()
    out = M.decode([CM.source("cmyk")], crop=(0, 0, 8, 8))[0]
    assert isinstance(out, M.MjhError) and out.code == M.EUNSUPPORTED and "four-component" in str(out), out
    out = M.decode([LD.source(LD.PRECISIONS[0])], crop=(0, 0, 8, 8), lossless_sources=True)[0]
    assert isinstance(out, M.MjhError) and out.code == M.EUNSUPPORTED and "lossless" in str(out), out


# ---- 8. the TurboJPEG library with MOZJPEG_HIP_REGIONS=1 ------------------------------------------------------------------------------
ENV = "MOZJPEG_HIP_REGIONS"


def _tj_region(p, src, region, pf, sf=(1, 1), pitch_extra=None, bottom_up=False):
    """tj3SetCroppingRegion + tj3Decompress8 on both libraries into buffers of one pattern with a spare row behind: equal return
    values, equal buffers"""
    w, h, _ = p.size(src)
    assert p.same("tj3SetScalingFactor", TD.ScalingFactor(*sf)) == 0
    p.set(bottomup=bottom_up)
    assert p.same("tj3SetCroppingRegion", TD.Region(*region)) == 0, TD.err(p.S, p.hs)
    sw, sh = TD.scaled(w, *sf), TD.scaled(h, *sf)
    rw, rh = region[2] or sw - region[0], region[3] or sh - region[1]
    tight = rw * TD.PIXEL_SIZE[pf]
    pitch = 0 if pitch_extra is None else tight + pitch_extra
    a = np.full(((pitch or tight) * (rh + 1),), TD.FILL, np.uint8)
    b = a.copy()
    ra, rb = p.S.tj3Decompress8(p.hs, src, len(src), a.ctypes.data, pitch, pf), p.R.tj3Decompress8(p.hr, src, len(src), b.ctypes.data, pitch, pf)
    assert ra == rb == 0, "tj3Decompress8: %d (%s), the reference %d (%s)" % (ra, TD.err(p.S, p.hs), rb, TD.err(p.R, p.hr))
    assert np.array_equal(a, b) and not (a[:tight * rh] == TD.FILL).all(), "region %s pf %d at %d/%d: %d bytes differ" % (region, pf, sf[0], sf[1], int((a != b).sum()))
    return a


@TD.with_pair
def check_tj_regions(p):
    os.environ[ENV] = "1"
    src = TD.source("s420")                             # 227 x 149, iMCU 16 x 16
    _tj_region(p, src, (16, 16, 32, 32), TD.PF_RGB)
    _tj_region(p, src, (32, 7, 100, 50), TD.PF_BGRX, pitch_extra=5)
    _tj_region(p, src, (208, 140, 0, 0), TD.PF_RGB)                   # to the right and bottom edge: the partial iMCU
    _tj_region(p, src, (0, 33, 227, 1), TD.PF_RGB)                    # rows alone
    _tj_region(p, src, (0, 0, 227, 149), TD.PF_RGB)                   # the whole image named as a region
    _tj_region(p, src, (48, 20, 17, 31), TD.PF_RGB, bottom_up=True)
    _tj_region(p, src, (16, 10, 40, 40), TD.PF_RGB, sf=(1, 2))        # iMCU 8 wide at 1/2
    _tj_region(p, src, (6, 3, 9, 9), TD.PF_GRAY, sf=(1, 8))
    _tj_region(p, TD.source("gray"), (8, 8, 50, 50), TD.PF_GRAY)      # a one-component file: iMCU 8 wide
    # refusals, with the reference's return values and texts
    p.set(bottomup=False)
    assert p.same("tj3SetScalingFactor", TD.ScalingFactor(1, 1)) == 0
    for bad in ((13, 7, 100, 50), (16, 0, 212, 10), (0, 0, 228, 10), (0, 140, 10, 10), (240, 0, 0, 0), (-16, 0, 8, 8), (0, 0, -1, 0)):
        assert p.same("tj3SetCroppingRegion", TD.Region(*bad)) == -1, bad
        assert TD.err(p.S, p.hs) == TD.err(p.R, p.hr), (bad, TD.err(p.S, p.hs), TD.err(p.R, p.hr))
    assert "divisible by the scaled iMCU width (16)" in TD.err(p.S, p.hs) or "Invalid cropping region" in TD.err(p.S, p.hs)
    # a refused call leaves the region that was set; TJUNCROPPED clears it
    assert p.same("tj3SetCroppingRegion", TD.Region(16, 16, 32, 32)) == 0
    assert p.same("tj3SetCroppingRegion", TD.Region(13, 7, 100, 50)) == -1
    assert p.same("tj3SetCroppingRegion", TD.Region(0, 0, 0, 0)) == 0
    p.pixels(src, TD.PF_RGB)


@TD.with_pair
def check_tj_fresh_handle(p):
    """before a header was read: the reference's text"""
    os.environ[ENV] = "1"
    assert p.same("tj3SetCroppingRegion", TD.Region(16, 16, 32, 32)) == -1
    assert TD.err(p.S, p.hs) == TD.err(p.R, p.hr) and "header" in TD.err(p.S, p.hs)


@TD.with_pair
def check_tj_unset_refuses(p):
    """the variable is read per call: without it a region other than TJUNCROPPED is refused exactly as it always was"""
    src = TD.source("s420")
    os.environ.pop(ENV, None)
    p.size(src)
    assert p.S.tj3SetCroppingRegion(p.hs, TD.Region(0, 0, 0, 0)) == 0
    assert p.S.tj3SetCroppingRegion(p.hs, TD.Region(16, 16, 32, 32)) == -1
    assert "partial decompression (a cropping region other than TJUNCROPPED) is not built" in TD.err(p.S, p.hs)
    p.pixels(src, TD.PF_RGB)
    os.environ[ENV] = "1"
    _tj_region(p, src, (16, 16, 32, 32), TD.PF_RGB)
    os.environ.pop(ENV, None)
    assert p.S.tj3SetCroppingRegion(p.hs, TD.Region(32, 16, 32, 32)) == -1 and "partial" in TD.err(p.S, p.hs)


TJ_CHECKS = {"regions": check_tj_regions, "fresh_handle": check_tj_fresh_handle, "unset_refuses": check_tj_unset_refuses}


def main(shim_path):
    """every TurboJPEG check against the library at shim_path, in a process of its own; prints {"name": "ok" | traceback}"""
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
        finally:
            os.environ.pop(ENV, None)
    print("REGION_TJ_RESULTS " + json.dumps(res))


if __name__ == "__main__":
    import sys
    main(sys.argv[1])


# ---- 9. the stand-alone libjpeg.so.62 with MOZJPEG_HIP_REGIONS=1: the unchanged djpeg, and a client of the API ------------------------
import djpeg_cases as DJ  # noqa: E402

DJPEG_SWITCHES = {"crop_aligned": ["-crop", "16x16+8+8"], "crop_unaligned": ["-crop", "100x50+13+7"], "skip": ["-skip", "1,2"],
                  "skip_nosmooth": ["-skip", "16,40", "-nosmooth"], "crop_scaled": ["-crop", "40x40+16+16", "-scale", "1/2"]}
DJPEG_PAIRS = [(s, k) for s in ("revert", "gray_r5b") for k in DJPEG_SWITCHES]


def check_djpeg(R, name, switches):
    """R: a djpeg_cases.Runner whose stand-alone runs have MOZJPEG_HIP_REGIONS=1"""
    DJ.check_djpeg(R, name, DJPEG_SWITCHES[switches])


def check_djpeg_refuses_without_the_variable(R0):
    """R0: a Runner without the variable -- the refusals of today"""
    for key in ("crop", "skip"):
        switches, word = DJ.DJPEG_REFUSED[key]
        DJ.check_djpeg_refused(R0, DC.source("revert"), switches, word)


# (rgb565, dither, num, denom, fancy, x, w, y, h[, x2, w2]) of tests/native/region_client
CLIENT_CASES = {"twice": (0, 0, 1, 1, 1, 21, 150, 30, 40, 40, 60), "once_565": (1, 1, 1, 1, 1, 37, 50, 3, 20), "scaled_nosmooth": (0, 0, 1, 2, 0, 9, 30, 10, 11),
                "whole_width": (0, 0, 1, 1, 1, 0, 227, 100, 49), "gray": (0, 0, 1, 1, 1, 13, 40, 0, 9)}


def check_client(standalone_dir, env, case):
    """jpeg_crop_scanline (twice), skip, read, skip to the end, finish on both libraries: the same rows, and the same *xoffset,
    *width, output_width and return values (everything the client prints)"""
    src = SC.source("gray_r5b" if case == "gray" else "revert")
    ref = client(src, CLIENT_CASES[case])
    assert ref[0] == 0 and "error" not in ref[1] and len(ref[2]) > 0, ref[1]
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        client.cache_clear()
        out = client(src, CLIENT_CASES[case], standalone_dir)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        client.cache_clear()
    assert out[1] == ref[1], "printed on the stand-alone library:\n%s\non the reference's:\n%s" % (out[1], ref[1])
    assert out[0] == 0 and out[2] == ref[2]
