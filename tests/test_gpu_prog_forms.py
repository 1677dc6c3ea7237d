"""GPU (-m gpu): the three forms of the progressive entropy coder (records, planes, ordered walk) against the oracle.  The same
cases as test_simt_prog_forms.py; see prog_forms_cases.py."""
import pytest

import prog_forms_cases as X

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cid", X.CASE_IDS)
def test_form_matches_the_oracle(cid):
    X.check_case(cid)
