"""Shared by test_simt_enc_pack_groups.py (CPU suite, emulator) and test_gpu_enc_pack_groups.py (-m gpu): a workgroup of the
one-walk sequential Huffman coder (k_enc_write_pack in mjh_kernels.hip) codes MJH_ENCP_GROUPS consecutive groups of 256 scan
positions of one image: tables staged once, the window zeroed behind every group, the next group's loads under way while a group
leaves.  Every file must be the reference's and the two-walk schedule's (MJH_ENC_ONEPASS=0), whatever the setting."""
import os

import numpy as np

import mozjpeg_amd as M
import oracle_lib as O
from cases import CASES, CASES12, images, images12
from enc_onepass_cases import saturated_noise

GROUPS = [1, 2, 4, 8]


class env:
    """environment for the encoders made inside (the library reads its knobs when an encoder is made); None = unset"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def scan_positions(w, h, kw):
    """blocks of the interleaved scan, dummy blocks included (the kernel's N)"""
    if kw.get("gray"):
        return -(-w // 8) * -(-h // 8)
    s = kw.get("sample", (2, 2))
    comps = s if isinstance(s[0], tuple) else (s, (1, 1), (1, 1))
    hmax, vmax = max(c[0] for c in comps), max(c[1] for c in comps)
    return -(-w // (8 * hmax)) * -(-h // (8 * vmax)) * sum(c[0] * c[1] for c in comps)


_refs = {}


def references(key, w, h, kw, frames):
    """the reference's files and the two-walk schedule's, computed once per case and shared by every setting of the knob"""
    if key not in _refs:
        po = O.make_params(w, h, **kw)
        want = [O.encode(po, f) for f in frames]
        with env(MJH_ENC_ONEPASS="0", MJH_ENCP_GROUPS=None):
            enc = M.Encoder(M.make_params(w, h, **kw), max_batch=len(frames))
        two = enc.encode_host(np.stack(frames))
        assert not enc.enc_onepass_stats()["enabled"]
        enc.close()
        for i in range(len(frames)):
            assert two[i] == want[i], ("two-walk schedule", key, i, len(two[i]), len(want[i]))
        _refs[key] = (want, two)
    return _refs[key]


def three_way(key, w, h, kw, frames, G):
    """frames in ONE call through an encoder made with MJH_ENCP_GROUPS=G: the reference's bytes, the two-walk schedule's bytes;
    returns the files and the slow-path counters"""
    want, two = references(key, w, h, kw, frames)
    with env(MJH_ENC_ONEPASS=None, MJH_ENCP_GROUPS=G):
        enc = M.Encoder(M.make_params(w, h, **kw), max_batch=len(frames))
    got = enc.encode_host(np.stack(frames))
    st = enc.enc_onepass_stats()
    groups = enc.enc_pack_groups()
    enc.close()
    assert st["enabled"] and groups[0] == G, (st, groups)
    for i in range(len(frames)):
        assert got[i] == want[i], ("reference", key, G, i, len(got[i]), len(want[i]))
        assert got[i] == two[i], ("MJH_ENC_ONEPASS=0", key, G, i)
    return got, st


# ---- 1. group counts round G: 1, 2, G - 1, G, G + 1 and 2 G + 1 groups for G = 1, 2, 4, 8 is the set below; every image has a last
# group of fewer than 256 positions, and odd sizes put dummy blocks at the right and bottom edges, so into the first and the last
# group of a workgroup.  (name, width, height, switches, groups)
COUNT_CASES = [
    ("420_48x48", 48, 48, dict(quality=75, baseline=True), 1),                              # 54 positions
    ("420_120x100", 120, 100, dict(quality=75, baseline=True), 2),                          # 8 x 7 MCUs of 6
    ("gray_264x128", 264, 128, dict(quality=75, baseline=True, gray=True), 3),              # 528 blocks
    ("420_232x152", 232, 152, dict(quality=75, baseline=True), 4),                          # 15 x 10 MCUs
    ("444_197x117", 197, 117, dict(quality=75, baseline=True, sample=(1, 1)), 5),           # 25 x 15 MCUs of 3
    ("422_328x160", 328, 160, dict(quality=75, baseline=True, sample=(2, 1)), 7),           # 21 x 20 MCUs of 4
    ("420_312x244", 312, 244, dict(quality=75, baseline=True), 8),                          # 20 x 16 MCUs
    ("gray_370x372", 370, 372, dict(quality=75, baseline=True, gray=True), 9),              # 47 x 47 blocks
    ("420_427x407", 427, 407, dict(quality=75, baseline=True), 17),                         # 27 x 26 MCUs
]


def check_group_counts(G):
    for name, w, h, kw, groups in COUNT_CASES:
        n = scan_positions(w, h, kw)
        assert (n + 255) // 256 == groups and n % 256 != 0, (name, n)
        frame = O.synthetic_frame(w, h, 4100 + groups)
        three_way("count/" + name, w, h, kw, [frame], G)
    need = {1, 2, G - 1, G, G + 1, 2 * G + 1} - {0}
    assert need <= {c[4] for c in COUNT_CASES}, need


# ---- 2. three different images in one call: tables are per image
def check_batch_of_three(G):
    w, h = 232, 152
    rng = np.random.default_rng(77)
    frames = [O.synthetic_frame(w, h, 4201), rng.integers(0, 256, (h, w, 3), dtype=np.uint8), np.full((h, w, 3), 90, np.uint8)]
    frames[2][40:90, 60:200] = O.synthetic_frame(140, 50, 4203)
    got, _ = three_way("batch3", w, h, dict(quality=75, baseline=True), frames, G)
    assert got[0] != got[1] and got[1] != got[2] and got[0] != got[2]


# ---- 3. the slow paths inside a multi-group workgroup: a normal group, two that outgrow the window, three normal ones (one of them
# with blocks longer than their staging column)
def smooth_frame(w, h, seed):
    """the colour fields and saturated tiles of oracle_lib.synthetic_frame without its Gaussian noise: at quality 100 that noise alone
    is some 300 bits per block, more than a window holds, and every group of the frame would be left to k_enc_write_big"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    f = [np.sin(x / 97 + seed) * np.cos(y / 71), np.sin((x + y) / 53), np.cos(x / 31 - y / 43)]
    img = np.clip(np.stack([128 + a * c for a, c in zip((100, 90, 80), f)], axis=-1), 0, 255).astype(np.uint8)
    img[((x.astype(np.int64) // 64 + y.astype(np.int64) // 64) % 7) == 0] = 255
    return img


def slow_path_frame():
    w, h = 136, 240
    img = smooth_frame(w, h, 4300)
    img[48:120] = saturated_noise(w, 72, 4301)                  # MCU rows 6..14: groups 1 and 2 outgrow their window
    img[160:200, 64:80] = saturated_noise(16, 40, 4302)         # two MCU columns of MCU rows 20..24: long blocks in group 4, which fits
    return w, h, img


def check_slow_paths(G, notrellis):
    w, h, img = slow_path_frame()
    kw = dict(quality=100, sample=(1, 1), baseline=True)
    if notrellis:
        kw["notrellis"] = True
    assert scan_positions(w, h, kw) == 1530           # six groups; 51 blocks per MCU row
    # image rows 48..119 are MCU rows 6..14 = scan positions 306..764: 206 of them in group 1 (256..511), 253 in group 2 (512..767),
    # none in groups 0, 3, 4 and 5; the stripe is 6 positions of each of the MCU rows 20..24, all in group 4 (1024..1279)
    noise = range(6 * 51, 15 * 51)
    assert [sum(1 for p in noise if p // 256 == g) for g in range(6)] == [0, 206, 253, 0, 0, 0]
    stripe = [r * 51 + 3 * 8 + k for r in range(20, 25) for k in range(6)]
    assert {p // 256 for p in stripe} == {4}
    got, st = three_way("slow/%d" % notrellis, w, h, kw, [img], G)
    # the reference's bytes: the band alone is more than 500 bits per block (saturated_noise), 200 blocks of it fill a window of 64 Kbit;
    # so groups 1 and 2 are among the big ones, and the count says that no other group is
    flat = O.encode(O.make_params(w, h, **kw), smooth_frame(w, h, 4300))
    assert (len(got[0]) - len(flat)) * 8 > 500 * (len(noise) + len(stripe)), (len(got[0]), len(flat))
    assert st["big_groups"] == 2, st
    assert st["long_blocks"] > 0, st          # (only blocks of groups that fit are counted: the stripe's)


# ---- 4. components and scripts
def case_kw(cname):
    return [k for c, k, _ in CASES + CASES12 if c == cname][0]


def check_golden_images(cname, G):
    kw = case_kw(cname)
    imgs = images12() if kw.get("precision") == 12 else images()
    for iname, img in imgs.items():
        h, w = img.shape[:2]
        three_way("golden/%s/%s" % (cname, iname), w, h, kw, [img], G)


SWITCH_CASES = ["base_samp_22_21_11",        # compact records, uneven sampling
                "revert",                    # one plane per position
                "script_seq_y_cbcr",         # a sequential script of two scans: the per-scan view of the launch
                "p12_base_420"]              # 12-bit, no trellis, no restart intervals
