"""GPU (-m gpu): several groups of 256 scan positions per workgroup of the one-walk Huffman coder (MJH_ENCP_GROUPS;
k_enc_write_pack).  The same cases as test_simt_enc_pack_groups.py (enc_pack_groups_cases.py), and calls with two batches in flight."""
import numpy as np
import pytest

import mozjpeg_amd as M
import oracle_lib as O
import enc_pack_groups_cases as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def fresh_references():
    X._refs.clear()          # (the emulator's module may have filled them in the same session: these are the device's)
    yield
    X._refs.clear()


@pytest.mark.parametrize("G", X.GROUPS)
def test_group_counts_round_the_setting(G):
    X.check_group_counts(G)


@pytest.mark.parametrize("G", X.GROUPS)
def test_three_images_in_one_call_keep_their_own_tables(G):
    X.check_batch_of_three(G)


@pytest.mark.parametrize("notrellis", [False, True])
@pytest.mark.parametrize("G", X.GROUPS)
def test_big_groups_and_long_blocks_between_normal_groups(G, notrellis):
    X.check_slow_paths(G, notrellis)


@pytest.mark.parametrize("cname", X.SWITCH_CASES)
@pytest.mark.parametrize("G", X.GROUPS)
def test_components_and_scripts(G, cname):
    X.check_golden_images(cname, G)


def test_consecutive_device_batch_calls_with_two_in_flight_match_the_oracle():
    import torch
    w, h, B = 531, 297, 5
    kw = dict(quality=75, baseline=True)
    sets = [np.stack([O.synthetic_frame(w, h, 1300 + 10 * s + i) for i in range(B)]) for s in range(2)]
    po = O.make_params(w, h, **kw)
    refs = [[O.encode(po, f) for f in fs] for fs in sets]
    dev = [torch.from_numpy(fs).cuda() for fs in sets]
    with X.env(MJH_ENC_ONEPASS=None, MJH_ENCP_GROUPS=4):
        enc = M.Encoder(M.make_params(w, h, **kw), max_batch=B)
    with X.env(MJH_ENCP_GROUPS=2):       # the second buffer set is made by the first call that needs it: it takes the encoder's setting, not the environment's
        order = [0, 1, 1, 0, 1]
        # back to back, no synchronisation in between: the second call is queued on the other buffer set while the first runs
        for n, s in enumerate(order):
            enc.encode_tensor(dev[s], stream="own")
            if n in (1, 4):
                assert [enc.get_jpeg(i) for i in range(B)] == refs[s], "call %d (input set %d)" % (n, s)
    assert enc.enc_pack_groups() == (4, 4)
    enc.encode_tensor(dev[0], stream="own")
    assert [enc.get_jpeg(i) for i in range(B)] == refs[0]
    enc.close()
