"""GPU (-m gpu): k_trellis_dc2, k_trellis_dc3 and the speculative pair (k_trellis_dc3_fwd / _resolve).  The same cases as
test_simt_dc_family.py; see dc_family_cases.py."""
import pytest

import dc_family_cases as X

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cid", X.CASE_IDS)
def test_family_takes_its_path_and_matches_the_oracle(cid):
    X.check_case(cid)


@pytest.mark.parametrize("size", X.OTHER_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cid", X.SIZE_CASES)
def test_a_full_group_and_a_short_row_match_the_oracle(cid, size):
    X.check_case(cid, size)


@pytest.mark.parametrize("spec", [None, "0"], ids=["default", "nospec"])
@pytest.mark.parametrize("gray", [False, True], ids=["colour", "gray"])
@pytest.mark.parametrize("name", X.TIE_IMAGES)
def test_ties_and_sign_changes_match_the_oracle(name, gray, spec):
    X.check_tie(name, gray, spec)


def test_the_clamp_binds_on_a_black_frame_at_quality_100():
    X.check_clamp()
