"""GPU (-m gpu): the DC trellis with one lane per chain (MJH_DC_LANES, k_trellis_dc_lane).  The same cases as
test_simt_dc_lanes.py (dc_lanes_cases.py), and two batches of 1080p frames in flight against the reference."""
import numpy as np
import pytest

import mozjpeg_amd as M
import oracle_lib as O
import dc_lanes_cases as X

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cname", X.GOLDEN_CASES)
def test_lane_kernel_reproduces_the_goldens(cname, goldens):
    X.check_golden_case(cname, goldens)


@pytest.mark.parametrize("sample", [(2, 2), (1, 1)])
@pytest.mark.parametrize("quality", X.NCAND_QUALITIES)
def test_every_candidate_count_matches_the_oracle(quality, sample):
    X.check_ncand(quality, sample)


def test_small_dc_steps_keep_the_general_kernel(goldens):
    X.check_golden_case("base_q90_444", goldens, want_path="dc2")


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("name", X.TIE_IMAGES)
def test_ties_and_sign_changes_match_the_oracle(name, gray):
    X.check_tie(name, gray)


def test_a_wave_that_spans_images_with_different_dc_tables():
    X.check_mixed_batch()


def test_threshold_selects_the_kernel_by_the_chain_count():
    X.check_threshold()


def test_two_batches_of_1080p_frames_in_flight_match_the_reference():
    import torch
    w, h, B = 1920, 1080, 4
    kw = dict(quality=75, baseline=True)
    frames = np.stack([O.synthetic_frame(w, h, 9100 + i) for i in range(B)])
    sets = [frames, np.ascontiguousarray(frames[::-1])]
    if O.have_ref():
        want, kind = [O.ref_encode(f, **kw)[0] for f in frames], "reference"
    else:
        po = O.make_params(w, h, **kw)
        want, kind = [O.encode(po, f) for f in frames], "port"
    refs = [want, want[::-1]]
    dev = [torch.from_numpy(fs).cuda() for fs in sets]
    with X.knob("1"):
        enc = M.Encoder(M.make_params(w, h, **kw), max_batch=B)
    # back to back, no synchronisation in between: the second call is queued on the other buffer set while the first runs
    enc.encode_tensor(dev[0], stream="own")
    enc.encode_tensor(dev[1], stream="own")
    got = [enc.get_jpeg(i) for i in range(B)]
    assert enc.dc_path() == "lane"
    enc.encode_tensor(dev[0], stream="own")
    got0 = [enc.get_jpeg(i) for i in range(B)]
    assert enc.dc_path() == "lane"
    enc.close()
    for i in range(B):
        assert got[i] == refs[1][i], "second call, frame %d differs from the %s" % (i, kind)
        assert got0[i] == refs[0][i], "third call, frame %d differs from the %s" % (i, kind)
