"""CPU suite: the one-walk sequential Huffman coder (MJH_ENC_ONEPASS) executed by the lock-step wave64 emulator (tools/simt).
The same cases as test_gpu_enc_onepass.py; see enc_onepass_cases.py."""
import os
import sys

import numpy as np
import pytest

import mozjpeg_amd as M
import oracle_lib as O
import enc_onepass_cases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "simt"))


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


@pytest.mark.parametrize("value", ["1", "0"])
@pytest.mark.parametrize("cname", X.COMPACT_CASES + X.DENSE_CASES)
def test_emulated_both_schedules_reproduce_the_goldens(simt, cname, value, goldens):
    X.check_golden_case(cname, value, goldens)


@pytest.mark.parametrize("cname", X.RESTART_CASES)
def test_emulated_restart_intervals_keep_the_two_walk_schedule(simt, cname, goldens):
    st = X.check_golden_case(cname, "1", goldens)
    assert st == dict(long_blocks=0, big_groups=0)


@pytest.mark.parametrize("notrellis", [False, True])
def test_emulated_long_blocks_and_big_groups_take_their_slower_paths(simt, notrellis):
    X.check_overflow_paths(notrellis)


def test_emulated_batches_of_distinct_frames_match_the_oracle(simt):
    """two consecutive calls with different inputs through one encoder (mjh_encode_host: streams are no-ops in the emulator)"""
    w, h, B = 531, 297, 5
    kw = dict(quality=75, baseline=True)
    sets = [np.stack([O.synthetic_frame(w, h, 1300 + 10 * s + i) for i in range(B)]) for s in range(2)]
    po = O.make_params(w, h, **kw)
    with X.knob("1"):
        enc = M.Encoder(M.make_params(w, h, **kw), max_batch=B)
    for s in (0, 1):
        got = enc.encode_host(sets[s])
        for i in range(B):
            assert got[i] == O.encode(po, sets[s][i]), (s, i)
    assert enc.enc_onepass_stats()["enabled"]
    enc.close()
