"""Shared by test_simt_dc_lanes.py (CPU suite, emulator) and test_gpu_dc_lanes.py (-m gpu): the cases of the DC trellis with one
lane per chain (MJH_DC_LANES, k_trellis_dc_lane in mjh_kernels.hip).  Every comparison is byte for byte against the committed
goldens or against the oracle computed here, never against another path of the library, and every case asserts which DC kernels
ran (Encoder.dc_path()), so that none can pass without the new kernel."""
import os

import numpy as np

import mozjpeg_amd as M
import oracle_lib as O
from cases import CASES, images

# baseline 4:2:0, gray, mixed sampling, a 4x2-sampled case and a progressive one, all with the DC trellis on
GOLDEN_CASES = ["base", "base_gray", "base_samp_22_21_11", "base_4x2_restart1", "default_progressive"]
NCAND_QUALITIES = [10, 50, 60, 75]        # DC steps 8q = 1280 / 128 / 104 / 64: 3 / 5 / 7 / 9 candidates (luma; get_num_dc_trellis_candidates)
TIE_IMAGES = ["flat0", "flat127", "flat128", "flat255", "checker", "lownoise"]


class knob:
    """MJH_DC_LANES for the encoders made inside (the library reads it when an encoder is made)"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.saved = os.environ.get("MJH_DC_LANES")
        if self.value is None:
            os.environ.pop("MJH_DC_LANES", None)
        else:
            os.environ["MJH_DC_LANES"] = self.value

    def __exit__(self, *exc):
        if self.saved is None:
            os.environ.pop("MJH_DC_LANES", None)
        else:
            os.environ["MJH_DC_LANES"] = self.saved


def case_kw(cname):
    return [k for c, k, _ in CASES if c == cname][0]


def encode_one(img, value, kw):
    """one image through an encoder made with MJH_DC_LANES=value: (file, dc_path)"""
    h, w = img.shape[:2]
    with knob(value):
        enc = M.Encoder(M.make_params(w, h, **kw))
    data = enc.encode_host(img)[0]
    path = enc.dc_path()
    enc.close()
    return data, path


def check_golden_case(cname, goldens, value="1", want_path="lane"):
    kw = case_kw(cname)
    for iname, img in images().items():
        data, path = encode_one(img, value, kw)
        assert path == want_path, (iname, cname, path)
        g = goldens["%s/%s" % (iname, cname)]
        assert (len(data), O.md5(data)) == (g["bytes"], g["md5"]), (iname, cname, value)


def noise_image(w, h, seed, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, (h, w, 3)).astype(np.uint8)


def check_ncand(quality, sample):
    w, h = 136, 72
    img = noise_image(w, h, 4100 + quality)
    kw = dict(quality=quality, baseline=True, sample=sample)
    data, path = encode_one(img, "1", kw)
    assert path == "lane"
    assert data == O.encode(O.make_params(w, h, **kw), img), (quality, sample)


def tie_image(name):
    """64 x 48: exact cost ties (flat), the orientation flipping at every block (checkerboard), the raw DC crossing zero along a row"""
    w, h = 64, 48
    if name.startswith("flat"):
        return np.full((h, w, 3), int(name[4:]), np.uint8)
    if name == "checker":
        y, x = np.mgrid[0:h, 0:w]
        return np.repeat(np.where(((y // 8) + (x // 8)) % 2 == 0, 16, 240).astype(np.uint8)[:, :, None], 3, axis=2)
    assert name == "lownoise"
    return noise_image(w, h, 77, 125, 132)


def check_tie(name, gray):
    img = tie_image(name)
    h, w = img.shape[:2]
    kw = dict(quality=75, baseline=True, gray=True) if gray else dict(quality=75, baseline=True)
    data, path = encode_one(img, "1", kw)
    assert path == "lane"
    assert data == O.encode(O.make_params(w, h, **kw), img), (name, gray)


def mixed_batch():
    """5 images of 40 x 24 whose DC tables differ: 5 x 2 luma chains share a wave"""
    w, h = 40, 24
    y, x = np.mgrid[0:h, 0:w]
    grad = np.stack([(x * 6) % 256, (y * 10) % 256, ((x + y) * 4) % 256], axis=2).astype(np.uint8)
    return np.stack([np.full((h, w, 3), 30, np.uint8), noise_image(w, h, 1), np.full((h, w, 3), 200, np.uint8), noise_image(w, h, 2, 100, 160), grad])


def check_mixed_batch():
    frames = mixed_batch()
    n, h, w = frames.shape[:3]
    kw = dict(quality=75, baseline=True)
    with knob("1"):
        enc = M.Encoder(M.make_params(w, h, **kw), max_batch=n)
    got = enc.encode_host(frames)
    path = enc.dc_path()
    enc.close()
    assert path == "lane"
    po = O.make_params(w, h, **kw)
    for i in range(n):
        assert got[i] == O.encode(po, frames[i]), i


def check_threshold():
    """MJH_DC_LANES=100 counts the chains of one component, frames x iMCU rows: 8 frames of 136 x 72 have 8 x 5 = 40 (dc3), 24 frames 120 (lane)"""
    w, h = 136, 72
    kw = dict(quality=75, baseline=True)
    po = O.make_params(w, h, **kw)
    for n, want in ((8, "dc3"), (24, "lane")):
        frames = np.stack([noise_image(w, h, 500 + i) for i in range(n)])
        with knob("100"):
            enc = M.Encoder(M.make_params(w, h, **kw), max_batch=n)
        got = enc.encode_host(frames)
        path = enc.dc_path()
        enc.close()
        assert path == want, (n, path)
        for i in range(n):
            assert got[i] == O.encode(po, frames[i]), (n, i)
