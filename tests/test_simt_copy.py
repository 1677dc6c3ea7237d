"""CPU suite: COM / APPn markers kept in re-compression (jpegtran -copy comments / all / icc, -icc FILE) and ICC profiles on
encode (cjpeg -icc FILE), with the kernels of mozjpeg_amd/csrc -- the hand-over kernel k_pack_results_spliced among them -- executed
by the lock-step wave64 emulator (tools/simt, SIMT_STRICT).  Every expected byte comes from the reference's jpegtran / cjpeg
(oracle/_ref) at test time."""
import os
import sys

import pytest

import mozjpeg_amd as M
import copy_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "simt"))

pytestmark = pytest.mark.skipif(not CC.have_tools(), reason="reference cjpeg / jpegtran not built (oracle/_ref)")


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


@pytest.mark.parametrize("copy,sw,with_icc", CC.MODE_CASES, ids=["%s-%s%s" % (c, s, "-icc" if i else "") for c, s, i in CC.MODE_CASES])
def test_modes(simt, copy, sw, with_icc):
    CC.check_mode(M, copy, sw, with_icc)


@pytest.mark.parametrize("behind_app7", [False, True], ids=["com", "com_behind_app7"])
def test_every_shift(simt, behind_app7):
    CC.check_every_shift(M, behind_app7)


@pytest.mark.parametrize("big_endian", [False, True], ids=["II", "MM"])
def test_exif_first(simt, big_endian):
    CC.check_exif_first(M, big_endian)


def test_exif_truncated_ifd_comes_back_untouched(simt):
    CC.check_exif_truncated(M)


def test_exif_behind_jfif_is_left_alone(simt):
    CC.check_exif_behind_jfif(M)


def test_markers_behind_the_first_sos_move_to_the_front(simt):
    CC.check_markers_behind_sos(M)


def test_adobe(simt):
    CC.check_adobe(M)


def test_large_markers_take_the_slow_path_and_the_arena(simt):
    CC.check_large(M)


@pytest.mark.parametrize("progressive_sources", [False, True], ids=["sequential", "with_progressive"])
def test_batch_with_a_damaged_file(simt, progressive_sources):
    CC.check_batch(M, progressive_sources)


@pytest.mark.parametrize("name", list(CC.ENCODE_CASES))
def test_icc_profile_on_encode(simt, name):
    CC.check_encode(M, name)


def test_icc_profile_without_hand_over_kernel(simt):
    CC.check_encode_without_hand_over(M)


def test_jpeg_markers(simt):
    CC.check_jpeg_markers(M)


def test_encoder_api(simt):
    CC.check_encoder_api(M)
