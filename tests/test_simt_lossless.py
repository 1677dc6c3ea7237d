"""CPU suite: the lossless (SOF3) kernels of mozjpeg_amd/csrc/mjh_lossless.hip executed by the lock-step wave64 emulator (tools/simt)
against the reference's files, pinned as MD5 + size in tests/golden/goldens_lossless.json (tests/golden/make_lossless_goldens.py runs
`oracle/_ref/cjpeg -revert -lossless` over lossless_cases.SIMT_CASES).  The refusals are host-side and checked here as well."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import mozjpeg_amd as M
import lossless_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "simt"))

with open(os.path.join(ROOT, "tests", "golden", "goldens_lossless.json")) as _f:
    GOLD = json.load(_f)


@pytest.fixture(scope="module")
def simt():
    """the ctypes layer bound to the emulator's library for this module only"""
    import build_simt
    path = build_simt.build()
    saved = (M.LIB_PATH, M._lib)
    M.LIB_PATH, M._lib = path, None
    try:
        yield path
    finally:
        M.LIB_PATH, M._lib = saved


@pytest.mark.parametrize("case", LC.SIMT_CASES, ids=LC.case_id)
def test_lossless_matches_reference(simt, case):
    kind, h, w, comps, prec, psv, pt, rst = case
    a = LC.image(kind, h, w, comps, prec)
    enc = M.Encoder(LC.params(M, a, psv, pt, prec, rst), max_batch=1)
    out = enc.encode_host(a)[0]
    g = GOLD[LC.case_id(case)]
    assert (hashlib.md5(out).hexdigest(), len(out)) == (g["md5"], g["size"])


def test_lossless_batch_of_distinct_images(simt):
    """one call, three different images: every file is the one its image gets alone"""
    cases = [c for c in LC.SIMT_CASES if c[1:5] == (29, 47, 3, 8)]
    imgs = [LC.image("smooth", 29, 47, 3, 8, seed=s) for s in range(3)]
    p = LC.params(M, imgs[0], 4, 0, 8, 1)
    enc = M.Encoder(p, max_batch=3)
    outs = enc.encode_host(np.stack(imgs))
    assert outs[0] == M.Encoder(p, max_batch=1).encode_host(imgs[0])[0]
    assert hashlib.md5(outs[0]).hexdigest() == GOLD[LC.case_id(cases[0])]["md5"]
    assert len(set(outs)) == 3


def test_lossless_category_16_is_counted(simt):
    """16-bit samples 0 next to 32768 (PSV 1): the difference -32768 is category 16 (jclhuff.c:359-365)"""
    a = LC.image("extreme", 11, 41, 1, 16)
    enc = M.Encoder(LC.params(M, a, 1, 0, 16), max_batch=1)
    enc.encode_host(a)
    counts = np.zeros(17, np.uint32)
    n = M.C.c_size_t()
    M._chk(M.lib().mjh_read_tap(enc._h, M.TAP_LL_COUNTS, 0, 0, counts.ctypes.data, counts.nbytes, M.C.byref(n)))
    assert counts[16] > 0 and counts.sum() == 11 * 41


@pytest.mark.parametrize("what", ["psv8", "psv_negative", "pt_eq_precision", "trellis", "arith", "max_profile", "restart_blocks",
                                  "ycc", "dc_table", "scans", "precision16_lossy"])
def test_lossless_refusals(simt, what):
    """what the reference refuses (or cannot write a readable file for) is an error, not a file"""
    a = LC.image("random", 8, 10, 3, 8)
    p = LC.params(M, a, 1, 0, 8)
    if what == "psv8":
        p.scan_info[0].Ss = 8
    elif what == "psv_negative":
        p.scan_info[0].Ss = -1
    elif what == "pt_eq_precision":
        p.scan_info[0].Al = 8
    elif what == "trellis":
        p.trellis_quant = 1
    elif what == "arith":
        p.arith_code = 1
    elif what == "max_profile":
        p.compress_profile = M.PROFILE_MAX_COMPRESSION
    elif what == "restart_blocks":
        p.restart_interval = 3               # cjpeg -restart 3B: not a multiple of the 10 MCUs of a row (JERR_BAD_RESTART)
    elif what == "ycc":
        p.color_transform = 0
    elif what == "dc_table":
        p.dc_tbl_no[1] = 1
    elif what == "scans":           # a lossless script of two scans (legal in the reference, one interleaved scan here)
        p.num_scans = 2
        p.scan_info[1] = p.scan_info[0]
    elif what == "precision16_lossy":
        p = M.make_params(10, 8, revert=True, precision=16)
    with pytest.raises(M.MjhError):
        M.Encoder(p, max_batch=1)


def test_lossless_has_no_planes_or_coefficient_input(simt):
    a = LC.image("random", 8, 16, 3, 8)
    enc = M.Encoder(LC.params(M, a, 1, 0, 8), max_batch=1)
    with pytest.raises(M.MjhError) as ei:
        enc.encode_planes_host([a[..., c] for c in range(3)])
    assert ei.value.code == M.EINVAL
    with pytest.raises(M.MjhError) as ei:
        enc.encode_coefficients_host([np.zeros((1, 2, 64), np.int16)] * 3)
    assert ei.value.code == M.EINVAL
