"""CPU suite: the three forms of the progressive entropy coder in mjh_prog.hip (records, planes, ordered walk) executed by the
lock-step wave64 emulator (tools/simt, SIMT_STRICT), whose device buffers end at unmapped pages.  The same cases as
test_gpu_prog_forms.py; see prog_forms_cases.py."""
import os
import sys

import pytest

import mozjpeg_amd as M
import prog_forms_cases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "simt"))


@pytest.fixture(scope="module")
def simt():
    """the ctypes layer bound to the emulator's library for this module only"""
    import build_simt
    path = build_simt.build()
    saved = (M.LIB_PATH, M._lib, os.environ.get("SIMT_STRICT"))
    M.LIB_PATH, M._lib = path, None
    os.environ["SIMT_STRICT"] = "1"
    try:
        yield path
    finally:
        M.LIB_PATH, M._lib = saved[:2]
        if saved[2] is None:
            os.environ.pop("SIMT_STRICT", None)
        else:
            os.environ["SIMT_STRICT"] = saved[2]


@pytest.mark.parametrize("cid", X.CASE_IDS)
def test_emulated_form_matches_the_oracle(simt, cid):
    X.check_case(cid)
