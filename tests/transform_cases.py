"""The case list of the lossless-transform tests of the re-compression path (test_simt_transform.py on the emulator,
test_gpu_transform.py on the chip).

Sources are transcode_cases.SOURCES; every expected byte comes from the reference's jpegtran at test time
(oracle_lib.ref_jpegtran(src, ["-copy", "none"] + transform switches + coding switches))."""
import functools

import oracle_lib as O
import transcode_cases as TC

# name of mozjpeg_amd.params_from_jpeg's `transform` keyword -> jpegtran's switch
OPS = {
    "flip_h": ["-flip", "horizontal"], "flip_v": ["-flip", "vertical"], "transpose": ["-transpose"], "transverse": ["-transverse"],
    "rot90": ["-rotate", "90"], "rot180": ["-rotate", "180"], "rot270": ["-rotate", "270"],
}

# the sources test 1 of the issue names
OP_SOURCES = ["revert", "q90_2x1_r1", "s1x2", "s_mixed", "gray_r5b", "scans3_2x2_r2", "rgb", "1x1", "8x8", "17x9"]
# (source, coding switches) on which the other coding switches are tried as well
CODING_SUBSET = [("revert", "revert_opt"), ("revert", "fastcrush_progressive"), ("q90_2x1_r1", "fastcrush_progressive"),
                 ("gray_r5b", "revert_opt"), ("scans3_2x2_r2", "revert_opt"), ("s_mixed", "fastcrush_progressive"), ("17x9", "revert_opt")]


def jpegtran_args(transform=None, trim=False, perfect=False, crop=None, grayscale=False):
    """jpegtran's switches for the keywords of mozjpeg_amd.transform_spec"""
    a = []
    if transform is not None:
        a += OPS[transform]
    if trim:
        a.append("-trim")
    if perfect:
        a.append("-perfect")
    if crop is not None:
        a += ["-crop", crop]
    if grayscale:
        a.append("-grayscale")
    return a


def _key(xf):
    return tuple(sorted(xf.items()))


@functools.lru_cache(maxsize=None)
def _reference(src_name, sw_name, key):
    return O.ref_jpegtran(TC.source(src_name), ["-copy", "none"] + jpegtran_args(**dict(key)) + TC.SWITCHES[sw_name][1])


def reference(src_name, sw_name, **xf):
    return _reference(src_name, sw_name, _key(xf))


def reference_status(src_name, sw_name, **xf):
    """(exit status, bytes or None) of the reference for a request it may refuse"""
    return TC.jpegtran_status(TC.source(src_name), ["-copy", "none"] + jpegtran_args(**xf) + TC.SWITCHES[sw_name][1])


def run(M, src, sw_name, max_batch=1, **xf):
    """the file the Encoder gives for (source bytes, coding switches, transform keywords)"""
    enc = M.Encoder(M.params_from_jpeg(src, **TC.SWITCHES[sw_name][0], **xf), max_batch=max_batch)
    try:
        return enc.transcode_host([src])[0]
    finally:
        enc.close()


def frame(M, jpeg):
    """(width, height, components, ((h, v), ...)) of a file, sequential or progressive: its SOFn segment"""
    pos = 2
    while pos + 4 <= len(jpeg):
        assert jpeg[pos] == 0xFF
        m, n = jpeg[pos + 1], (jpeg[pos + 2] << 8) | jpeg[pos + 3]
        if m in (0xC0, 0xC1, 0xC2):
            h, w, nc = (jpeg[pos + 5] << 8) | jpeg[pos + 6], (jpeg[pos + 7] << 8) | jpeg[pos + 8], jpeg[pos + 9]
            return w, h, nc, tuple((jpeg[pos + 11 + 3 * c] >> 4, jpeg[pos + 11 + 3 * c] & 15) for c in range(nc))
        pos += 2 + n
    raise AssertionError("no SOF0 / SOF1 / SOF2 segment")


# every operation x {plain, trim} x the sources above, in the `revert` coding; the other codings on the subset
OP_CASES = [(s, "revert", op, trim) for s in OP_SOURCES for op in OPS for trim in (False, True)] + \
           [(s, sw, op, trim) for s, sw in CODING_SUBSET for op in ("rot90", "flip_h", "transverse") for trim in (False, True)]

# test 2 of the issue: (source, transform, crop, the size the reference writes)
CROP_CASES = [
    ("revert", None, "100x80+17+9", (101, 89)), ("q90_2x1_r1", None, "100x80+17+9", (101, 81)), ("gray_r5b", None, "100x80+17+9", (101, 81)),
    ("revert", "rot180", "100x80+20+30", (104, 94)), ("q90_2x1_r1", "rot180", "100x80+20+30", (104, 86)),
    ("revert", None, "+16+16", (211, 133)), ("revert", None, "100x80-20-30", (111, 87)), ("revert", None, "100x80-0-0", (115, 85)),
    ("revert", None, "127x69+100+80", (131, 69)),
    # and on the way past every operation, where the crop applies in output coordinates
    ("revert", "rot90", "64x100+17+9", None), ("s_mixed", "transverse", "50x60+40+33", None), ("scans3_2x2_r2", "flip_v", "100x80+17+9", None),
    ("q90_2x1_r1", "rot270", "40x100+10+20", None), ("s1x2", "flip_h", "100x80-20-30", None), ("rgb", "transpose", "60x60+9+9", None),
]
