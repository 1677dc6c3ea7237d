"""CPU suite: decoding lossless JPEG files (SOF3) to samples (mjh_decode_host on an encoder made from the file's own parameters) with
the kernels of mjh_decode_lossless.hip executed by the lock-step wave64 emulator (tools/simt, SIMT_STRICT), whose device buffers end
at unmapped pages.  Every expected sample comes from the reference's djpeg at test time and is compared for exact equality; the
sources are made at test time by the reference's cjpeg (tests/lossless_decode_cases.py).  The files with damaged entropy-coded data
run here only."""
import ctypes
import os
import re
import sys

import pytest

import mozjpeg_amd as M
import lossless_decode_cases as LD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "simt"))

pytestmark = pytest.mark.skipif(not LD.have_tools(), reason="reference cjpeg / djpeg not built (oracle/_ref)")


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


# ---- 0. the interface ---------------------------------------------------------------------------------------------------------------
def test_constant_and_appended_fields():
    hdr = open(os.path.join(ROOT, "include", "mozjpeg_hip.h")).read()
    assert re.search(r"#define\s+MJH_SRC_LOSSLESS\s+2u\b", hdr) and M.SRC_LOSSLESS == 2 and M.SRC_PROGRESSIVE == 1
    # mjh_jpeg_info grew at its end: the fields of before keep their places
    names = [f[0] for f in M.JpegInfo._fields_]
    assert names[-3:] == ["scans", "lossless_psv", "lossless_pt"]
    assert M.JpegInfo.lossless_psv.offset == M.JpegInfo.scans.offset + 4 * ctypes.sizeof(M.JpegScan)
    assert re.search(r"mjh_jpeg_scan scans\[MJH_MAX_FILE_SCANS\];\s*int lossless_psv, lossless_pt;[^\n]*\n\} mjh_jpeg_info;", hdr)


def test_set_sources_takes_the_bit_alone_or_with_the_progressive_one(simt):
    import lossless_cases as LC
    enc = M.Encoder(LC.params(M, LD.case_image(LD.BATCH[0]), 1, 0, 8), max_batch=1)
    try:
        L = M.lib()
        for accept in (0, 1, 2, 3):
            assert L.mjh_encoder_set_sources(enc._h, accept) == M.OK
        assert L.mjh_encoder_set_sources(enc._h, 4) == M.EINVAL
    finally:
        enc.close()
    info, n = M.JpegInfo(), ctypes.c_int()
    assert M.lib().mjh_jpeg_probe_ex(LD.source(LD.BATCH[0]), len(LD.source(LD.BATCH[0])), 4, ctypes.byref(info), None, 0, ctypes.byref(n)) == M.EINVAL


def test_probe_reports_the_scans(simt):
    LD.check_probe(M)


# ---- 1. samples == djpeg's == the image's -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", LD.GEOMETRY, ids=LD.case_id)
def test_geometry(simt, c):
    LD.check_case(M, c)


@pytest.mark.parametrize("c", LD.PREDICTORS, ids=LD.case_id)
def test_every_predictor(simt, c):
    LD.check_case(M, c)


@pytest.mark.parametrize("c", LD.RESTARTS, ids=LD.case_id)
def test_restart_intervals(simt, c):
    LD.check_case(M, c)


@pytest.mark.parametrize("c", LD.PRECISIONS, ids=LD.case_id)
def test_precisions_and_point_transforms(simt, c):
    LD.check_case(M, c)


@pytest.mark.parametrize("c", LD.SCRIPTS, ids=LD.case_id)
def test_scan_scripts(simt, c):
    LD.check_case(M, c)


def test_tables_in_different_slots(simt):
    LD.check_table_slots(M)


def test_a_segment_of_many_subsequences(simt):
    LD.check_sync(M)


# ---- 2. batches ---------------------------------------------------------------------------------------------------------------------
def test_five_files_in_two_batches(simt):
    LD.check_batch(M)


def test_an_encoder_serves_calls_with_different_predictors(simt):
    LD.check_encoder_reuse(M)


def test_a_lossless_and_a_sequential_file_in_one_call(simt):
    LD.check_mixed_kinds(M)


# ---- 3. layouts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", LD.LAYOUT_CASES, ids=LD.case_id)
def test_layouts_and_bottom_up(simt, c):
    LD.check_layouts(M, c)


def test_scale_nosmooth_and_dct_are_ignored(simt):
    LD.check_ignored_options(M)


def test_device_buffer_against_get_pixels(simt):
    LD.check_pixels_device(M, ctypes.string_at)


# ---- 4. opt-in and refusals -----------------------------------------------------------------------------------------------------------
def test_without_the_keyword_a_lossless_file_is_refused_as_before(simt):
    LD.check_default_refusals(M)


def test_what_stays_refused(simt):
    LD.check_refusals(M)


# ---- 5. untrusted input -----------------------------------------------------------------------------------------------------------------
def test_damaged_files_get_a_status_and_the_good_file_its_samples(simt):
    LD.check_damaged(M)
