"""CPU suite: several groups of 256 scan positions per workgroup of the one-walk Huffman coder (MJH_ENCP_GROUPS), executed by the
lock-step wave64 emulator (tools/simt).  The same cases as test_gpu_enc_pack_groups.py; see enc_pack_groups_cases.py."""
import os
import sys

import numpy as np
import pytest

import mozjpeg_amd as M
import oracle_lib as O
import enc_pack_groups_cases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "simt"))


@pytest.fixture(scope="module")
def simt():
    """the ctypes layer bound to the emulator's library for this module only"""
    import build_simt
    path = build_simt.build()
    saved = (M.LIB_PATH, M._lib)
    M.LIB_PATH, M._lib = path, None
    X._refs.clear()
    try:
        yield path
    finally:
        M.LIB_PATH, M._lib = saved
        X._refs.clear()


@pytest.mark.parametrize("G", X.GROUPS)
def test_emulated_group_counts_round_the_setting(simt, G):
    X.check_group_counts(G)


@pytest.mark.parametrize("G", X.GROUPS)
def test_emulated_three_images_in_one_call_keep_their_own_tables(simt, G):
    X.check_batch_of_three(G)


@pytest.mark.parametrize("notrellis", [False, True])
@pytest.mark.parametrize("G", X.GROUPS)
def test_emulated_big_groups_and_long_blocks_between_normal_groups(simt, G, notrellis):
    X.check_slow_paths(G, notrellis)


@pytest.mark.parametrize("cname", X.SWITCH_CASES)
@pytest.mark.parametrize("G", X.GROUPS)
def test_emulated_components_and_scripts(simt, G, cname):
    X.check_golden_images(cname, G)


def test_emulated_consecutive_calls_of_distinct_batches(simt):
    """two calls with different inputs through one encoder at four groups per workgroup (streams are no-ops in the emulator: the
    calls with two batches in flight are test_gpu_enc_pack_groups.py's)"""
    w, h, B = 531, 297, 5
    kw = dict(quality=75, baseline=True)
    sets = [np.stack([O.synthetic_frame(w, h, 1300 + 10 * s + i) for i in range(B)]) for s in range(2)]
    po = O.make_params(w, h, **kw)
    with X.env(MJH_ENC_ONEPASS=None, MJH_ENCP_GROUPS=4):
        enc = M.Encoder(M.make_params(w, h, **kw), max_batch=B)
    for s in (0, 1, 0):
        got = enc.encode_host(sets[s])
        for i in range(B):
            assert got[i] == O.encode(po, sets[s][i]), (s, i)
    assert enc.enc_pack_groups()[0] == 4
    enc.close()
