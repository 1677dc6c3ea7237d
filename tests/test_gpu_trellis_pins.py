"""GPU (-m gpu): the AC trellis kernels of mjh_trellis.hip under dictated blocks, on the chip.  The cases of test_simt_trellis_pins.py
(tests/trellis_cases.py, whose premises that module proves on the CPU): every section-2 case under every schedule, the wave and tile
shapes under the schedules of the two first tiers, the 4:2:0 image, the batch and the EXT instantiations.  Every expected byte comes
from the C restatement and, where it is built, from the real reference; equality is exact, and schedules that share their parameters
must give one file."""
import pytest

import mozjpeg_amd as M
import trellis_cases as T

pytestmark = pytest.mark.gpu

CASES = T.cases()
SHAPES = T.shape_cases()


@pytest.mark.parametrize("name,sched", T.case_schedules(), ids=["%s-%s" % p for p in T.case_schedules()])
def test_dictated_blocks(name, sched):
    T.run_case(M, CASES[name], sched)


@pytest.mark.parametrize("name,sched", T.shape_schedules(), ids=["%s-%s" % p for p in T.shape_schedules()])
def test_wave_and_tile_shapes(name, sched):
    T.run_shape(M, SHAPES[name], sched)


@pytest.mark.parametrize("sched", T.FIRST_FIVE)
def test_colour_420(sched):
    T.run_color(M, sched)


@pytest.mark.parametrize("sched", T.FIRST_FIVE)
def test_batch_of_three_distinct_images(sched):
    T.run_batch(M, sched)


@pytest.mark.parametrize("coding", list(T.EXT_CODINGS))
@pytest.mark.parametrize("option", list(T.EXT_OPTIONS))
def test_ext_instantiations(option, coding):
    T.run_ext(M, option, coding)


@pytest.mark.parametrize("coding,seed", T.EOB_CHAIN_CASES)
def test_eob_chain_ties(coding, seed):
    T.run_eob_chain(M, coding, seed)
