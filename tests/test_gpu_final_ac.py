"""GPU (-m gpu): the final AC symbol statistics counted inside the AC trellis kernels (MJH_FUSE_FINAL_AC).  The same cases as
test_simt_final_ac.py (final_ac_cases.py), and calls with two batches in flight."""
import numpy as np
import pytest

import mozjpeg_amd as M
import oracle_lib as O
import final_ac_cases as X

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(X.JOBS))
def test_counts_and_files_with_the_knob_on_and_off(name):
    X.run(M, name)


def test_knob_and_coder_groups_given_together():
    X.check_knobs_are_independent(M)


@pytest.mark.parametrize("knob", [None, 0])
def test_consecutive_device_batch_calls_with_two_in_flight(knob):
    import torch
    w, h, B = 531, 297, 5
    kw = dict(quality=75, baseline=True)
    sets = [np.stack([O.synthetic_frame(w, h, 1700 + 10 * s + i) for i in range(B)]) for s in range(2)]
    po = O.make_params(w, h, **kw)
    refs = [[O.encode(po, f) for f in fs] for fs in sets]
    dev = [torch.from_numpy(fs).cuda() for fs in sets]
    with X.env(MJH_SMALL_BATCH=1, MJH_FUSE_FINAL_AC=knob):
        enc = M.Encoder(M.make_params(w, h, **kw), max_batch=B)
    with X.env(MJH_FUSE_FINAL_AC=1 if knob == 0 else 0):      # the second buffer set takes the encoder's setting, not the environment's
        order = [0, 1, 1, 0, 1]
        # back to back, no synchronisation in between: the second call is queued on the other buffer set while the first runs
        for n, s in enumerate(order):
            enc.encode_tensor(dev[s], stream="own")
            if n in (1, 4):
                assert [enc.get_jpeg(i) for i in range(B)] == refs[s], "call %d (input set %d)" % (n, s)
    assert enc.final_ac_fused() == ((knob is None), (knob is None))
    enc.close()
