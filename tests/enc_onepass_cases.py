"""Shared by test_simt_enc_onepass.py (CPU suite, emulator) and test_gpu_enc_onepass.py (-m gpu): the cases of the one-walk
sequential Huffman coder (MJH_ENC_ONEPASS, k_enc_write_pack / k_enc_write_place / k_enc_write_big in mjh_kernels.hip).  A scan
without restart intervals is coded in one walk over its blocks; MJH_ENC_ONEPASS=0 and scans with restart intervals keep the
length pass and the second walk.  Both schedules must give the reference's bytes."""
import os

import numpy as np

import mozjpeg_amd as M
import oracle_lib as O
from cases import CASES, images

COMPACT_CASES = ["base", "base_q90_444", "base_gray", "base_samp_22_21_11"]     # the trellis hands compact records over
DENSE_CASES = ["revert", "base_notrellis"]                                       # one plane per position
RESTART_CASES = ["base_restart1", "base_restart5b", "base_4x2_restart1"]


class knob:
    """MJH_ENC_ONEPASS for the encoders made inside (the library reads it when an encoder is made)"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.saved = os.environ.get("MJH_ENC_ONEPASS")
        if self.value is None:
            os.environ.pop("MJH_ENC_ONEPASS", None)
        else:
            os.environ["MJH_ENC_ONEPASS"] = self.value

    def __exit__(self, *exc):
        if self.saved is None:
            os.environ.pop("MJH_ENC_ONEPASS", None)
        else:
            os.environ["MJH_ENC_ONEPASS"] = self.saved


def case_kw(cname):
    return [k for c, k, _ in CASES if c == cname][0]


def check_golden_case(cname, value, goldens):
    """every golden image of the case through an encoder made with MJH_ENC_ONEPASS=value; returns the summed counters"""
    kw = case_kw(cname)
    stats = dict(long_blocks=0, big_groups=0)
    for iname, img in images().items():
        h, w = img.shape[:2]
        with knob(value):
            enc = M.Encoder(M.make_params(w, h, **kw))
        data = enc.encode_host(img)[0]
        st = enc.enc_onepass_stats()
        enc.close()
        assert st["enabled"] == (value == "1")
        for k in stats:
            stats[k] += st[k]
        g = goldens["%s/%s" % (iname, cname)]
        assert (len(data), O.md5(data)) == (g["bytes"], g["md5"]), (iname, cname, value)
    return stats


def saturated_noise(w, h, seed):
    """every sample 0 or 255, independently per channel: 553 bits per block on average at quality 100, 4:4:4 -- more than the
    one-walk coder's window holds (256 bits per block), and luma blocks far longer than a staging column (256 bits)"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)


def check_overflow_paths(notrellis):
    # 17 x 16 MCUs of three blocks = 816 blocks: three groups of 256 that outgrow their window, and a last group of 48 blocks
    # that fits it and holds blocks longer than their staging column -- both slower paths in one image
    w, h = 136, 128
    img = saturated_noise(w, h, 20250)
    kw = dict(quality=100, sample=(1, 1), baseline=True)
    if notrellis:
        kw["notrellis"] = True
    want = O.encode(O.make_params(w, h, **kw), img)
    nblocks = 3 * (w // 8) * (h // 8)
    assert (len(want) - 700) * 8 > 2 * 256 * nblocks * 0.9        # the input is as dense as the test needs
    got = {}
    for value in ("1", "0"):
        with knob(value):
            enc = M.Encoder(M.make_params(w, h, **kw))
        got[value] = enc.encode_host(img)[0]
        st = enc.enc_onepass_stats()
        enc.close()
        assert got[value] == want, (value, len(got[value]), len(want))
        if value == "1":
            assert st["enabled"] and st["long_blocks"] > 0 and st["big_groups"] > 0, st
        else:
            assert not st["enabled"] and st["long_blocks"] == 0 and st["big_groups"] == 0, st
    # a frame with every kind of group: flat (a few bits per block), a band of noise over the whole width (groups that outgrow
    # their window), and a narrow patch of noise (long blocks inside groups that fit)
    w2, h2 = 320, 256
    mixed = np.full((h2, w2, 3), 128, np.uint8)
    mixed[32:80] = saturated_noise(w2, 48, 6)
    mixed[160:224, 120:184] = saturated_noise(64, 64, 7)
    with knob("1"):
        enc = M.Encoder(M.make_params(w2, h2, **kw))
    data = enc.encode_host(mixed)[0]
    st = enc.enc_onepass_stats()
    enc.close()
    assert data == O.encode(O.make_params(w2, h2, **kw), mixed)
    assert st["long_blocks"] > 0 and st["big_groups"] > 0, st
