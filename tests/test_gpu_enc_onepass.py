"""GPU (-m gpu): the one-walk sequential Huffman coder (MJH_ENC_ONEPASS; k_enc_write_pack / k_enc_write_place /
k_enc_write_big).  The same cases as test_simt_enc_onepass.py (enc_onepass_cases.py), and two 4K frames against the reference."""
import numpy as np
import pytest

import mozjpeg_amd as M
import oracle_lib as O
import enc_onepass_cases as X

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("value", ["1", "0"])
@pytest.mark.parametrize("cname", X.COMPACT_CASES + X.DENSE_CASES)
def test_both_schedules_reproduce_the_goldens(cname, value, goldens):
    X.check_golden_case(cname, value, goldens)


@pytest.mark.parametrize("cname", X.RESTART_CASES)
def test_restart_intervals_keep_the_two_walk_schedule(cname, goldens):
    st = X.check_golden_case(cname, "1", goldens)
    assert st == dict(long_blocks=0, big_groups=0)


@pytest.mark.parametrize("notrellis", [False, True])
def test_long_blocks_and_big_groups_take_their_slower_paths(notrellis):
    X.check_overflow_paths(notrellis)


@pytest.mark.parametrize("value", ["1", "0"])
def test_consecutive_device_batch_calls_with_two_in_flight_match_the_oracle(value):
    import torch
    w, h, B = 531, 297, 5
    kw = dict(quality=75, baseline=True)
    sets = [np.stack([O.synthetic_frame(w, h, 1300 + 10 * s + i) for i in range(B)]) for s in range(2)]
    po = O.make_params(w, h, **kw)
    refs = [[O.encode(po, f) for f in fs] for fs in sets]
    dev = [torch.from_numpy(fs).cuda() for fs in sets]
    with X.knob(value):
        enc = M.Encoder(M.make_params(w, h, **kw), max_batch=B)
    # back to back, no synchronisation in between: the second call is queued on the other buffer set while the first runs
    order = [0, 1, 1, 0, 1]
    for n, s in enumerate(order):
        enc.encode_tensor(dev[s], stream="own")
        if n in (1, 4):
            assert [enc.get_jpeg(i) for i in range(B)] == refs[s], "call %d (input set %d)" % (n, s)
    assert enc.enc_onepass_stats()["enabled"] == (value == "1")       # (the second buffer set takes the first one's setting)
    enc.encode_tensor(dev[0], stream="own")
    assert [enc.get_jpeg(i) for i in range(B)] == refs[0]
    enc.close()


def test_two_4k_frames_match_the_reference():
    w, h = 3840, 2160
    kw = dict(quality=75, baseline=True)
    frames = np.stack([O.synthetic_frame(w, h, 8800 + i) for i in range(2)])
    with X.knob("1"):
        enc = M.Encoder(M.make_params(w, h, **kw), max_batch=2)
    got = enc.encode_host(frames)
    assert enc.enc_onepass_stats()["enabled"]
    enc.close()
    for i, f in enumerate(frames):
        if O.have_ref():
            want, kind = O.ref_encode(f, **kw)[0], "reference"
        else:
            want, kind = O.encode(O.make_params(w, h, **kw), f), "port"
        assert got[i] == want, "frame %d differs from the %s (%d vs %d bytes)" % (i, kind, len(got[i]), len(want))
