"""GPU (-m gpu): valid progressive files (SOF2) that no libjpeg encoder writes, on the chip -- mjh_decode_prog.hip in front of the
pixel, export and entropy-coding kernels.  The families of test_simt_prog_streams.py (tests/prog_stream_cases.py; files from
tests/jpeg_writer_progressive.py at test time).  Every coefficient array is compared with the writer's, which test_premise compares with the reference's; every
pixel with the reference's djpeg and every re-coded byte with its jpegtran (oracle/_ref), run at test time; equality is exact."""
import pytest

import mozjpeg_amd as M
import prog_stream_cases as PS

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not PS.have_tools(), reason="reference cjpeg / djpeg / jpegtran / libjpeg.so.62 or tests/native/coef_dump not built")]


@pytest.fixture
def subseq(monkeypatch):
    def set_(s):
        if s is None:
            monkeypatch.delenv("MJH_DECODE_SUBSEQ", raising=False)
        else:
            monkeypatch.setenv("MJH_DECODE_SUBSEQ", str(s))
    return set_


# ---- 1. every family ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PS.NAMES)
def test_premise(name):
    PS.check_premise(M, name)


@pytest.mark.parametrize("name", PS.NAMES)
def test_coefficients_are_the_writers(name):
    PS.check_coefficients(M, name)


@pytest.mark.parametrize("name", PS.NAMES)
def test_pixels_match_djpeg(name):
    PS.check_pixels(M, name)


@pytest.mark.parametrize("sw", PS.RECOMPRESS_SWITCHES)
@pytest.mark.parametrize("name", PS.RECOMPRESS)
def test_recompressed_file_matches_jpegtran(name, sw):
    PS.check_recompress(M, name, sw)


@pytest.mark.parametrize("a,b", [("eob_none", "eob_max"), ("eob_split", "eob_max"), ("marker_noise", "marker_clean")])
def test_files_that_differ_decode_alike(a, b):
    PS.check_same_decode(M, a, b)


# ---- 2. subsequences and batching -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PS.SUBSEQ_CASES))
def test_subsequence_lengths_give_the_same_results(subseq, name):
    PS.check_subseq(M, name, subseq)


def test_sixteen_files_of_every_kind_in_one_call():
    PS.check_mixed_batch(M)
