"""CPU suite: k_trellis_dc2, k_trellis_dc3 and the speculative pair (k_trellis_dc3_fwd / _resolve) executed by the lock-step
wave64 emulator (tools/simt).  The same cases as test_gpu_dc_family.py; see dc_family_cases.py."""
import os
import sys

import pytest

import mozjpeg_amd as M
import dc_family_cases as X

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


@pytest.mark.parametrize("cid", X.CASE_IDS)
def test_emulated_family_takes_its_path_and_matches_the_oracle(simt, cid):
    X.check_case(cid)


@pytest.mark.parametrize("size", X.OTHER_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cid", X.SIZE_CASES)
def test_emulated_a_full_group_and_a_short_row_match_the_oracle(simt, cid, size):
    X.check_case(cid, size)


@pytest.mark.parametrize("spec", [None, "0"], ids=["default", "nospec"])
@pytest.mark.parametrize("gray", [False, True], ids=["colour", "gray"])
@pytest.mark.parametrize("name", X.TIE_IMAGES)
def test_emulated_ties_and_sign_changes_match_the_oracle(simt, name, gray, spec):
    X.check_tie(name, gray, spec)


def test_emulated_the_clamp_binds_on_a_black_frame_at_quality_100(simt):
    X.check_clamp()
