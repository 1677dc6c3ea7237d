"""CPU suite: the final AC symbol statistics counted inside the AC trellis kernels (MJH_FUSE_FINAL_AC; the CF instantiations of
k_trellis_ac_v3, k_trellis_ac_q and k_trellis_ac_qd in mjh_trellis.hip), executed by the lock-step wave64 emulator (tools/simt).
The same cases as test_gpu_final_ac.py; see final_ac_cases.py.  profiles/final_ac_fused_mutations.md records which of these cases
fails when a counting rule is broken."""
import os
import sys

import pytest

import mozjpeg_amd as M
import final_ac_cases as X

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


@pytest.mark.parametrize("name", list(X.JOBS))
def test_emulated_counts_and_files_with_the_knob_on_and_off(simt, name):
    X.run(M, name)


def test_emulated_knob_and_coder_groups_given_together(simt):
    X.check_knobs_are_independent(M)
