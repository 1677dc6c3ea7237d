"""Shared by test_simt_dc_family.py (CPU suite, emulator) and test_gpu_dc_family.py (-m gpu): the DC trellis kernels that share
the chain setup, the window form's row walk and the back-track of mjh_kernels.hip (K6): k_trellis_dc2, k_trellis_dc3 and the
speculative pair k_trellis_dc3_fwd / _resolve.  Every case asserts which kernels ran (Encoder.dc_path()) and compares byte for
byte against the oracle computed here, never against another path of the library.

The default frame is 136 x 72 seeded noise: luma wib = 17 (one full group of 16 blocks and one more), luma hib = 9 (odd: the
last iMCU row leaves at br >= hib), chroma wib = 9 (one short group).  128 x 32 has a luma wib of exactly 16, 40 x 24 of 5."""
import os

import numpy as np

import mozjpeg_amd as M
import oracle_lib as O
from dc_lanes_cases import NCAND_QUALITIES, TIE_IMAGES, noise_image, tie_image

FRAME = (136, 72)
OTHER_SIZES = [(128, 32), (40, 24)]
BASE = dict(baseline=True)

# (id, expected path, frames, MJH_DC_SPEC, parameters)
CASES = []
for _q in NCAND_QUALITIES:          # 3 / 5 / 7 / 9 candidates (luma)
    for _n in (1, 2):
        CASES.append(("spec_q%d_n%d" % (_q, _n), "speculative", _n, None, dict(BASE, quality=_q)))
CASES += [
    ("spec_1x2_q50_n1", "speculative", 1, None, dict(BASE, quality=50, sample=(1, 2))),
    ("spec_progressive_q75_n1", "speculative", 1, None, dict(quality=75)),
    ("dc3_q75_n3", "dc3", 3, None, dict(BASE, quality=75)),
]
for _q in NCAND_QUALITIES:
    CASES.append(("dc3_nospec_q%d_n1" % _q, "dc3", 1, "0", dict(BASE, quality=_q)))
CASES += [
    ("dc3_444_n1", "dc3", 1, None, dict(BASE, quality=75, sample=(1, 1))),       # v = 1: nothing to speculate on
    ("dc3_gray_n1", "dc3", 1, None, dict(BASE, quality=75, gray=True)),
    ("dc2_q95_n1", "dc2", 1, None, dict(BASE, quality=95)),                      # 8q < 40: v = 2 with the general kernel
    ("dc2_q95_n3", "dc2", 3, None, dict(BASE, quality=95)),
    ("dc2_verw1_n1", "dc2", 1, None, dict(BASE, quality=75, dc_ver_weight=1.0)),
    ("dc2_verw025_n3", "dc2", 3, None, dict(BASE, quality=75, dc_ver_weight=0.25)),
]
CASE_IDS = [c[0] for c in CASES]
# one case of each family (dc2: both with and without the vertical term) at the other sizes
SIZE_CASES = ["spec_q75_n2", "dc3_q75_n3", "dc2_q95_n1", "dc2_verw1_n1"]


class env:
    """MJH_DC_SPEC for the encoders made inside (the library reads it when an encoder is made); MJH_DC_LANES is taken out, so
    that the default choice of the kernels is what runs"""

    def __init__(self, spec):
        self.want = {"MJH_DC_SPEC": spec, "MJH_DC_LANES": None}

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.want}
        self._set(self.want)

    def __exit__(self, *exc):
        self._set(self.saved)

    @staticmethod
    def _set(values):
        for k, v in values.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def check(frames, want_path, spec, kw):
    n, h, w = frames.shape[:3]
    with env(spec):
        enc = M.Encoder(M.make_params(w, h, **kw), max_batch=n)
    got = enc.encode_host(frames)
    path = enc.dc_path()
    enc.close()
    assert path == want_path, (path, want_path)
    po = O.make_params(w, h, **kw)
    for i in range(n):
        assert got[i] == O.encode(po, frames[i]), "frame %d differs from the oracle" % i


def check_case(cid, size=FRAME):
    _, want_path, n, spec, kw = CASES[CASE_IDS.index(cid)]
    w, h = size
    check(np.stack([noise_image(w, h, 7300 + w + i) for i in range(n)]), want_path, spec, kw)


def check_clamp():
    """a black frame at quality 100 (q0 = 1, dc2): the luma DC is -1024 quantizer steps, so the candidates -1020 .. -1028 meet the
    clamp to +-1023 (jcdctmgr.c:1058-1062) in the forward walk and in the back-track, which no other 8-bit input reaches"""
    w, h = FRAME
    check(np.zeros((1, h, w, 3), np.uint8), "dc2", None, dict(BASE, quality=100))


def check_tie(name, gray, spec):
    """the 64 x 48 images of dc_lanes_cases.py, one frame: exact ties, the orientation flipping at every block, the raw DC crossing
    zero.  Colour at the default takes the speculative pair; gray has one block row per iMCU row and keeps dc3, as MJH_DC_SPEC=0 does"""
    kw = dict(BASE, quality=75, gray=True) if gray else dict(BASE, quality=75)
    want_path = "speculative" if spec is None and not gray else "dc3"
    check(tie_image(name)[None], want_path, spec, kw)
