"""GPU suite: lossless source files (SOF3) on the chip -- mjh_decode_lossless.hip.  The cases are those of
test_simt_lossless_decode.py (tests/lossless_decode_cases.py); every expected sample comes from the reference's djpeg at test time
and is compared for exact equality.  The files with damaged entropy-coded data run on the emulator only."""
import numpy as np
import pytest

import mozjpeg_amd as M
import lossless_cases as LC
import lossless_decode_cases as LD

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not LD.have_tools(), reason="reference cjpeg / djpeg not built (oracle/_ref)")]


@pytest.mark.parametrize("c", LD.GEOMETRY, ids=LD.case_id)
def test_geometry(c):
    LD.check_case(M, c)


@pytest.mark.parametrize("c", LD.PREDICTORS, ids=LD.case_id)
def test_every_predictor(c):
    LD.check_case(M, c)


@pytest.mark.parametrize("c", LD.RESTARTS, ids=LD.case_id)
def test_restart_intervals(c):
    LD.check_case(M, c)


@pytest.mark.parametrize("c", LD.PRECISIONS, ids=LD.case_id)
def test_precisions_and_point_transforms(c):
    LD.check_case(M, c)


@pytest.mark.parametrize("c", LD.SCRIPTS, ids=LD.case_id)
def test_scan_scripts(c):
    LD.check_case(M, c)


def test_tables_in_different_slots():
    LD.check_table_slots(M)


def test_a_segment_of_many_subsequences():
    LD.check_sync(M)


def test_five_files_in_two_batches():
    LD.check_batch(M)


def test_an_encoder_serves_calls_with_different_predictors():
    LD.check_encoder_reuse(M)


def test_a_lossless_and_a_sequential_file_in_one_call():
    LD.check_mixed_kinds(M)


@pytest.mark.parametrize("c", LD.LAYOUT_CASES, ids=LD.case_id)
def test_layouts_and_bottom_up(c):
    LD.check_layouts(M, c)


def test_scale_nosmooth_and_dct_are_ignored():
    LD.check_ignored_options(M)


class _DeviceView:
    """the encoder's pixel buffer as an object torch can wrap without a copy"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = dict(shape=(n,), strides=(1,), typestr="|u1", data=(ptr, False), version=2)


def test_device_buffer_against_get_pixels():
    import torch
    LD.check_pixels_device(M, lambda ptr, n: torch.as_tensor(_DeviceView(ptr, n), device="cuda:0").cpu().numpy().tobytes())


def test_without_the_keyword_a_lossless_file_is_refused_as_before():
    LD.check_default_refusals(M)


def test_what_stays_refused():
    LD.check_refusals(M)


def test_probe_reports_the_scans():
    LD.check_probe(M)


def test_two_full_hd_files_through_every_multi_workgroup_path():
    """the one case above toy size: two distinct 1920 x 1080 RGB files in one call, predictor 1 without restarts and predictor 6 in
    40 intervals of 27 rows"""
    imgs = [LC.image("random", 1080, 1920, 3, 8, seed=s) for s in (5, 6)]
    files = [LC.reference(imgs[0], 1, 0, 8), LC.reference(imgs[1], 6, 0, 8, 27)]
    assert all(isinstance(f, bytes) for f in files) and files[0] != files[1]
    out = M.decode(files, lossless_sources=True, max_batch=2)
    for f, o, a in zip(files, out, imgs):
        assert not isinstance(o, Exception), o
        assert LD.same(o, LD.djpeg(f)) and np.array_equal(o, a)
