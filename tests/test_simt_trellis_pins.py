"""CPU suite: the AC trellis kernels of mjh_trellis.hip (k_trellis_ac_v3, k_trellis_ac_q, k_trellis_ac_qd and their EXT
instantiations) under DICTATED blocks, executed by the lock-step wave64 emulator (tools/simt).  The cases, the restatement of the
dynamic programme that proves which branch each block takes, and the run helpers are in tests/trellis_cases.py; every expected byte
comes from the C restatement (and from the real reference where it is built), and equality is exact.

The premise tests and the restatement-equals-oracle test need no emulator: they are the proof that the cases are what they claim,
whatever the kernels do."""
import os
import sys

import pytest

import mozjpeg_amd as M
import trellis_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "simt"))

CASES = T.cases()
SHAPES = T.shape_cases()


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


# ---- the cases are what they claim (no emulator) --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("mode", ["loop1", "loop2", "progressive", "progressive_loop2"])
def test_restatement_gives_the_oracles_blocks(name, mode):
    T.check_restatement(CASES[name], loops=2 if mode.endswith("loop2") else 1, progressive=mode.startswith("progressive"))


@pytest.mark.parametrize("name", list(CASES))
def test_dictated_blocks_show_their_events(name):
    T.check_premise(CASES[name])


def test_every_required_event_has_two_blocks_in_different_places():
    T.check_coverage()


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_have_the_keys_they_are_named_for(name):
    T.check_shape_premise(name, SHAPES[name])


def test_colour_image_has_its_dictated_blocks_in_all_three_components():
    T.check_color_premise()


@pytest.mark.parametrize("coding,seed", T.EOB_CHAIN_CASES)
def test_eob_chain_rows_have_a_tie_that_decides(coding, seed):
    T.check_eob_chain_premise(coding, seed)


# ---- the kernels --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sched", T.case_schedules(), ids=["%s-%s" % p for p in T.case_schedules()])
def test_dictated_blocks(simt, name, sched):
    T.run_case(M, CASES[name], sched)


@pytest.mark.parametrize("name,sched", T.shape_schedules(), ids=["%s-%s" % p for p in T.shape_schedules()])
def test_wave_and_tile_shapes(simt, name, sched):
    T.run_shape(M, SHAPES[name], sched)


@pytest.mark.parametrize("sched", T.FIRST_FIVE)
def test_colour_420(simt, sched):
    T.run_color(M, sched)


@pytest.mark.parametrize("sched", T.FIRST_FIVE)
def test_batch_of_three_distinct_images(simt, sched):
    T.run_batch(M, sched)


@pytest.mark.parametrize("coding", list(T.EXT_CODINGS))
@pytest.mark.parametrize("option", list(T.EXT_OPTIONS))
def test_ext_instantiations(simt, option, coding):
    T.run_ext(M, option, coding)


@pytest.mark.parametrize("coding,seed", T.EOB_CHAIN_CASES)
def test_eob_chain_ties(simt, coding, seed):
    T.run_eob_chain(M, coding, seed)
