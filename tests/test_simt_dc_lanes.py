"""CPU suite: the DC trellis with one lane per chain (MJH_DC_LANES, k_trellis_dc_lane) executed by the lock-step wave64
emulator (tools/simt).  The same cases as test_gpu_dc_lanes.py; see dc_lanes_cases.py."""
import os
import sys

import pytest

import mozjpeg_amd as M
import dc_lanes_cases as X

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


@pytest.mark.parametrize("cname", X.GOLDEN_CASES)
def test_emulated_lane_kernel_reproduces_the_goldens(simt, cname, goldens):
    X.check_golden_case(cname, goldens)


@pytest.mark.parametrize("sample", [(2, 2), (1, 1)])
@pytest.mark.parametrize("quality", X.NCAND_QUALITIES)
def test_emulated_every_candidate_count_matches_the_oracle(simt, quality, sample):
    X.check_ncand(quality, sample)


def test_emulated_small_dc_steps_keep_the_general_kernel(simt, goldens):
    X.check_golden_case("base_q90_444", goldens, want_path="dc2")


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("name", X.TIE_IMAGES)
def test_emulated_ties_and_sign_changes_match_the_oracle(simt, name, gray):
    X.check_tie(name, gray)


def test_emulated_a_wave_that_spans_images_with_different_dc_tables(simt):
    X.check_mixed_batch()


def test_emulated_threshold_selects_the_kernel_by_the_chain_count(simt):
    X.check_threshold()
