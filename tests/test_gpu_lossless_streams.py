"""GPU (-m gpu): lossless files (SOF3) that the reference reads silently and no libjpeg encoder writes, on the chip --
mjh_decode_lossless.hip.  The families of test_simt_lossless_streams.py (tests/lossless_stream_cases.py; files from
tests/jpeg_writer_lossless.py at test time).  Every sample is compared with the reference's djpeg (oracle/_ref), run at test
time, which test_premise compares with the writer's; equality is exact.  Every file here is one the reference decodes cleanly;
lossless_stream_cases.CJPEG_CASES are files of its own cjpeg that the lists of tests/lossless_decode_cases.py lack."""
import pytest

import mozjpeg_amd as M
import lossless_stream_cases as LS

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not LS.have_tools(), reason="reference cjpeg / djpeg not built (oracle/_ref)")]


@pytest.mark.parametrize("name", LS.NAMES)
def test_premise(name):
    LS.check_premise(name)


@pytest.mark.parametrize("name", LS.NAMES)
def test_samples_match_djpeg(name):
    LS.check_decode(M, name)


@pytest.mark.parametrize("c", LS.CJPEG_CASES, ids=LS.LD.case_id)
def test_cjpeg_files_the_older_lists_lack(c):
    LS.LD.check_case(M, c)


@pytest.mark.parametrize("name", LS.MULTI_SCAN)
def test_probe_reports_the_scans_as_written(name):
    LS.check_scans(M, name)


@pytest.mark.parametrize("name", LS.LAYOUT_CASES)
def test_layouts_and_bottom_up(name):
    LS.check_layouts(M, name)


@pytest.mark.parametrize("name", list(LS.REFUSED))
def test_refused_by_the_reference_and_here(name):
    LS.check_refused(M, name)


def test_a_segment_of_many_subsequences_under_16_bit_codes():
    LS.check_sync_long(M)


def test_four_hand_written_files_in_one_call():
    LS.check_batch(M)
