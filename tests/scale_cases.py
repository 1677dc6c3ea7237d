"""The case list and helpers of the reduced-size decoder tests (test_simt_decode_scale.py on the emulator, test_gpu_decode_scale.py
on the chip): djpeg -scale 1/2, 1/4 and 1/8, the reduced inverse DCTs of jidctred.c.

Sources are made at test time the way decode_cases.py makes them (the reference's cjpeg, and tests/jpeg_writer.py for the file
with absurd quantization steps); the expected pixels always come from the reference's djpeg at test time
(oracle/_ref/djpeg -pnm -scale M/8 + switches), and every comparison is exact equality with its PPM / PGM payload, shape
included."""
import functools

import numpy as np

import decode_cases as DC
import jpeg_writer as W
import oracle_lib as O
import transcode_cases as TC

have_tools = DC.have_tools

# name -> (the scale keyword of mozjpeg_amd.decode, djpeg's argument, the IDCT size k: output = ceil(input * k / 8))
SCALES = {"1/2": ((1, 2), "4/8", 4), "1/4": ("1/4", "2/8", 2), "1/8": ((1, 8), "1/8", 1)}
# fractions that are not M/8: djpeg is given the same fraction and resolves it (jdmaster.c:105ff)
FRACTIONS = {"1/5": 2, "3/16": 2, "7/16": 4, "1/9": 1, "1/100": 1, "9/10": 8}


def absurd_quant():
    """a 2x2,1x1,2x1 file (one component of every DCT_scaled_size at every scale) with every step of its 16-bit quantization tables
    at 65535 and dense coefficients up to +-1023: dequantized values of 2^26, products with the transforms' constants far beyond
    32 bits, samples all over the wrapped range-limit table"""
    comps = [(1, 2, 2, 0), (2, 1, 1, 1), (3, 2, 1, 1)]
    w, h = 45, 37
    rng = np.random.default_rng(77)
    coefs = []
    for ci in range(3):
        rows, cols = W.padded_blocks(w, h, comps, ci)
        a = rng.integers(-1023, 1024, (rows, cols, 64))
        a[..., 0] = rng.integers(-200, 201, (rows, cols))            # (DC differences stay within the 11 categories)
        a[rows // 2, :, 1:] = 0                                      # a row of DC-only blocks: the reference's shortcuts
        a[:, cols // 2, 8:] = 0
        coefs.append(a)
    qt = {0: (1, [65535] * 64), 1: (1, [65535] * 64)}
    scans = [dict(comps=[0, 1, 2], dc=[0, 1, 1], ac=[0, 1, 1], ri=0, shape="optimal")]
    data, _ = W.write_jpeg(w, h, comps, coefs, qt, scans, sof=1, header="jfif")
    return data


EXTRA = {
    "8x8_2x1": lambda: TC.cjpeg(O.synthetic_frame(8, 8, 4), ["-revert", "-sample", "2x1"]),
    "17x9_2x1": lambda: TC.cjpeg(O.synthetic_frame(17, 9, 5), ["-revert", "-sample", "2x1"]),
    "absurd_quant": absurd_quant,
}
# transcode_cases.SOURCES that differ in geometry: 4:2:0, 2x1 with a restart interval, 1x2, 2x2,1x1,2x1, gray with a restart interval,
# RGB, the multi-scan file; the small frames; large coefficients everywhere
GEOMETRY = ["revert", "q90_2x1_r1", "s1x2", "s_mixed", "gray_r5b", "rgb", "scans3_2x2_r2"]
SMALL = ["1x1", "8x8", "17x9", "8x8_2x1", "17x9_2x1"]
NAMES = GEOMETRY + SMALL + ["noise_q100", "absurd_quant"]

MODES = dict(DC.MODES)
CASES = [(s, "default", sc) for s in NAMES for sc in SCALES]
CASES += [(s, "nosmooth", sc) for s in ("revert", "q90_2x1_r1", "s1x2", "s_mixed", "17x9", "17x9_2x1", "absurd_quant") for sc in SCALES]
CASES += [(s, "grayscale", sc) for s in ("revert", "rgb", "s_mixed", "absurd_quant") for sc in SCALES]
CASES += [("gray_r5b", "rgb", sc) for sc in SCALES]
LAYOUT_CASES = [(s, "bgrx", sc) for s in ("revert", "17x9_2x1", "gray_r5b") for sc in SCALES]
FRACTION_CASES = [(s, f) for s in ("revert", "s_mixed", "17x9_2x1") for f in FRACTIONS]


def case_id(c):
    return "-".join(c).replace("/", "_")


@functools.lru_cache(maxsize=None)
def source(name):
    return EXTRA[name]() if name in EXTRA else TC.source(name)


@functools.lru_cache(maxsize=None)
def reference(name, mode, scale_arg):
    """djpeg -scale <scale_arg> + the mode's switches (scale_arg None: full size)"""
    args = ([] if scale_arg is None else ["-scale", scale_arg]) + MODES[mode][1]
    status, pix = DC.djpeg_status(source(name), args)
    assert status == 0 and pix is not None, "djpeg %s exits with %d on %s" % (" ".join(args), status, name)
    return pix


def scaled_shape(M, name, mode, k):
    """[ceil(H k / 8), ceil(W k / 8)(, 3)] from the file's header"""
    info = M.jpeg_info(source(name))
    hw = (-(-info.image_height * k // 8), -(-info.image_width * k // 8))
    gray = mode == "grayscale" or (info.num_components == 1 and mode != "rgb")
    return hw if gray else hw + (3,)


def run(M, name, mode, scale, **kw):
    out = M.decode([source(name)], scale=scale, **dict(MODES[mode][0], **kw))[0]
    if isinstance(out, Exception):
        raise out
    return out


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def dct_scaled_sizes(info, k):
    """DCT_scaled_size of every component at IDCT size k (jpeg_calc_output_dimensions jdmaster.c:287-302)"""
    nc = info.num_components
    maxh = max(info.h_samp_factor[c] for c in range(nc))
    maxv = max(info.v_samp_factor[c] for c in range(nc))
    out = []
    for c in range(nc):
        ss = k
        while ss < 8 and maxh * k % (info.h_samp_factor[c] * ss * 2) == 0 and maxv * k % (info.v_samp_factor[c] * ss * 2) == 0:
            ss *= 2
        out.append(ss)
    return out


def damaged(src, M):
    """`src` with 40 bytes of its entropy-coded data missing, every marker in place"""
    info = M.jpeg_info(src)
    a, n = info.scans[0].data_offset, info.scans[0].data_size
    return src[:a + n // 2] + src[a + n // 2 + 40:]


def raw_opts(M, num, denom):
    """a DecodeOpts with the two fields set WITHOUT the binding's own validation: what a C caller could pass"""
    o = M.DecodeOpts()
    M.lib().mjh_decode_opts_defaults(o)
    o.scale_num, o.scale_denom = num, denom
    return o


# ---- the checks both test files make --------------------------------------------------------------------------------------------------
def check_case(M, name, mode, sc):
    scale, arg, k = SCALES[sc]
    ref = reference(name, mode, arg)
    out = run(M, name, mode, scale)
    assert out.shape == scaled_shape(M, name, mode, k) == ref.shape, "%s, the reference %s" % (out.shape, ref.shape)
    assert same(out, ref)


def check_layout_case(M, name, layout, sc):
    scale, arg, k = SCALES[sc]
    rgb = reference(name, "rgb", arg)
    out = M.decode([source(name)], color="rgb", layout=layout, scale=scale)[0]
    DC.check_layout(rgb, out, layout)


def check_fraction(M, name, frac):
    k = FRACTIONS[frac]
    num, denom = (int(v) for v in frac.split("/"))
    assert M.scale_idct_size(num, denom) == k
    ref = reference(name, "default", frac)
    assert ref.shape == scaled_shape(M, name, "default", k), "the reference resolves %s otherwise" % frac
    assert same(run(M, name, "default", frac), ref)
    assert same(run(M, name, "default", (num, denom)), ref)


def check_every_transform_size_is_reached(M):
    """the premise of the case list: every DCT_scaled_size at every scale, mixed sizes inside one file, and the reduced widths
    that pick the plain and the fancy h2v1 function"""
    seen = set()
    for name in NAMES:
        for sc, (_, _, k) in SCALES.items():
            seen.add((k, tuple(dct_scaled_sizes(M.jpeg_info(source(name)), k))))
    for k, sizes in ((4, (4, 8, 8)), (2, (2, 4, 4)), (1, (1, 2, 2)), (4, (4, 8, 4)), (2, (2, 4, 2)), (1, (1, 2, 1)), (4, (4, 4, 4)), (1, (1,))):
        assert (k, sizes) in seen, (k, sizes, sorted(seen))
    for name, dw in (("8x8_2x1", 1), ("17x9_2x1", 3)):                # at 1/4: chroma keeps size 2 and goes through h2v1
        info = M.jpeg_info(source(name))
        assert dct_scaled_sizes(info, 2) == [2, 2, 2]
        assert -(-info.image_width * 1 * 2 // (2 * 8)) == dw


def check_one_encoder_serves_every_scale(M):
    for name in ("revert", "s_mixed", "gray_r5b"):
        src = source(name)
        fresh = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=1)
        full = fresh.decode_host([src])[0]
        fresh.close()
        assert same(full, DC.reference(name, "default"))
        enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=1)
        for scale, arg in ((None, None), ("1/4", "2/8"), ((1, 1), None), ("1/8", "1/8"), ((8, 8), None), ("1/2", "4/8")):
            out = enc.decode_host([src], scale=scale)[0]
            st = enc.decode_stats()
            assert (st["height"], st["width"]) == out.shape[:2]
            assert same(out, full if arg is None else reference(name, "default", arg)), (name, scale)
        o = M.DecodeOpts()                                            # a zeroed struct: 0/0 is 1/1 (and no fancy upsampling)
        assert (o.scale_num, o.scale_denom, o.fancy_upsampling) == (0, 0, 0)
        assert same(enc.decode_host([src], opts=o)[0], DC.reference(name, "nosmooth"))
        enc.close()


def check_mixed_batch(M):
    names = ["revert", "gray_r5b", "17x9_2x1", "s_mixed", "revert_opt", "rgb", "8x8", "q90_2x1_r1"]
    files = [source(s) for s in names]
    bad = damaged(TC.source("revert"), M)
    files.insert(3, bad)
    names.insert(3, None)
    for sc in ("1/4", "1/8"):
        scale, arg, k = SCALES[sc]
        outs = M.decode(files, max_batch=4, scale=scale)
        for s, o in zip(names, outs):
            if s is None:
                assert isinstance(o, M.MjhError) and o.code == M.EINVAL and "Corrupt" in str(o)
            else:
                assert same(o, reference(s, "default", arg)), (s, sc)


def check_refusals(M):
    src = TC.source("revert")
    M._decode_encoders.clear()
    for scale, code, word in (("3/8", M.EUNSUPPORTED, "3x3"), ((2, 1), M.EUNSUPPORTED, "16x16"), ("5/8", M.EUNSUPPORTED, "5x5"),
                              ((9, 8), M.EUNSUPPORTED, "9x9"), ((0, 3), M.EINVAL, "scale"), ((-1, 8), M.EINVAL, "scale"),
                              ((1, -8), M.EINVAL, "scale"), ((1, 0), M.EINVAL, "scale"), ("half", M.EINVAL, "scale"), ((1, 2, 3), M.EINVAL, "scale")):
        with pytest_raises(M, code, word):
            M.decode([src], scale=scale)
    assert not M._decode_encoders                                     # refused before anything was grouped
    enc = M.Encoder(M.params_from_jpeg(src, revert=True), max_batch=1)
    full = enc.decode_host([src])[0]
    for (num, denom), code, word in (((3, 8), M.EUNSUPPORTED, "3x3"), ((2, 1), M.EUNSUPPORTED, "16x16"), ((1000, 1), M.EUNSUPPORTED, "16x16"),
                                     ((0, 3), M.EINVAL, "scale"), ((3, 0), M.EINVAL, "scale"), ((-1, 8), M.EINVAL, "scale"),
                                     ((1, -8), M.EINVAL, "scale"), ((-1, -8), M.EINVAL, "scale")):
        for errors in ("raise", "return"):
            with pytest_raises(M, code, word):
                enc.decode_host([src], errors=errors, opts=raw_opts(M, num, denom))
        assert M.lib().mjh_transcode_batch_size(enc._h) == 0
    assert same(enc.decode_host([src])[0], full)                      # the encoder stays usable
    assert same(enc.decode_host([src], opts=raw_opts(M, 2 ** 31 - 1, 2 ** 31 - 1))[0], full)
    assert same(enc.decode_host([src], opts=raw_opts(M, 1, 2 ** 31 - 1))[0], reference("revert", "default", "1/8"))
    enc.close()
    enc = M.Encoder(M.params_from_jpeg(src, revert=True, transform="flip_h"), max_batch=1)
    with pytest_raises(M, M.EUNSUPPORTED, "transform"):
        enc.decode_host([src], scale="1/2")
    enc.close()


class pytest_raises:
    """`with` block that must raise an MjhError of `code` whose text holds `word`"""
    def __init__(self, M, code, word):
        self.M, self.code, self.word = M, code, word

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        assert et is not None and issubclass(et, self.M.MjhError), "no MjhError (%s)" % (et,)
        assert ev.code == self.code and self.word in str(ev), "%d %s" % (ev.code, ev)
        return True
