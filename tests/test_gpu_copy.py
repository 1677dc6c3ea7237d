"""COM / APPn markers kept in re-compression and ICC profiles on encode, on the chip (-m gpu): the cases of test_simt_copy.py,
whole files compared with the reference's jpegtran -copy / -icc and cjpeg -icc.  Reads only the tree and oracle/_ref."""
import pytest

import mozjpeg_amd as M
import copy_cases as CC

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not CC.have_tools(), reason="reference cjpeg / jpegtran not built (oracle/_ref)")]


@pytest.mark.parametrize("copy,sw,with_icc", CC.MODE_CASES, ids=["%s-%s%s" % (c, s, "-icc" if i else "") for c, s, i in CC.MODE_CASES])
def test_modes(copy, sw, with_icc):
    CC.check_mode(M, copy, sw, with_icc)


@pytest.mark.parametrize("behind_app7", [False, True], ids=["com", "com_behind_app7"])
def test_every_shift(behind_app7):
    CC.check_every_shift(M, behind_app7)


@pytest.mark.parametrize("big_endian", [False, True], ids=["II", "MM"])
def test_exif_first(big_endian):
    CC.check_exif_first(M, big_endian)


def test_exif_truncated_ifd_comes_back_untouched():
    CC.check_exif_truncated(M)


def test_exif_behind_jfif_is_left_alone():
    CC.check_exif_behind_jfif(M)


def test_markers_behind_the_first_sos_move_to_the_front():
    CC.check_markers_behind_sos(M)


def test_adobe():
    CC.check_adobe(M)


def test_large_markers_take_the_slow_path_and_the_arena():
    CC.check_large(M)


@pytest.mark.parametrize("progressive_sources", [False, True], ids=["sequential", "with_progressive"])
def test_batch_with_a_damaged_file(progressive_sources):
    CC.check_batch(M, progressive_sources)


@pytest.mark.parametrize("name", list(CC.ENCODE_CASES))
def test_icc_profile_on_encode(name):
    CC.check_encode(M, name)


def test_icc_profile_without_hand_over_kernel():
    CC.check_encode_without_hand_over(M)


def test_jpeg_markers():
    CC.check_jpeg_markers(M)


def test_encoder_api():
    CC.check_encoder_api(M)
