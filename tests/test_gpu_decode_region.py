"""GPU (-m gpu): decoding a region of a JPEG file on the chip (mjh_decode_opts.crop_x / crop_y / crop_w / crop_h: djpeg -crop
WxH+X+Y; k_idct_region, k_idct_region_scaled, k_upcolor_region and k_upcolor_565_region of mjh_idct.hip, and the restart
segments the host leaves out).  Every expected pixel comes from the reference's djpeg -crop at test time and is compared for
exact equality, the array shape included (tests/region_cases.py)."""
import pytest

import mozjpeg_amd as M
import oracle_lib as O
import region_cases as RG
import scale_cases as SC
import transcode_cases as TC

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not RG.have_tools(), reason="reference cjpeg / jpegtran / djpeg not built (oracle/_ref)")]
needs_client = pytest.mark.skipif(not RG.have_client(), reason="reference libjpeg.so.62 or tests/native/region_client not built")


@pytest.mark.parametrize("src,mode", RG.CASES, ids=[RG.case_id(c) for c in RG.CASES])
def test_every_region_matches_djpeg_crop(src, mode):
    RG.check_case(M, src, mode)


@pytest.mark.parametrize("src", RG.LAYOUT_SOURCES)
def test_layouts_and_bottom_up(src):
    RG.check_layout(M, src)


@needs_client
@pytest.mark.parametrize("src,dither,scale", RG.CASES_565, ids=[RG.case_id(c) for c in RG.CASES_565])
def test_rgb565_regions(src, dither, scale):
    RG.check_565(M, src, dither, scale)


def test_restart_segments_outside_the_region_are_left_out():
    RG.check_pruning(M)


def test_progressive_and_arithmetic_sources():
    RG.check_other_entropy_coders(M)


def test_one_encoder_serves_regions_and_whole_images():
    RG.check_one_encoder(M)


class _DeviceView:
    """device memory as an object torch can wrap without a copy"""

    def __init__(self, ptr, shape, strides):
        self.__cuda_array_interface__ = dict(shape=shape, strides=strides, typestr="|u1", data=(ptr, False), version=2)


def _fetch(ptr, nbytes):
    import torch
    return torch.as_tensor(_DeviceView(ptr, (nbytes,), (1,)), device="cuda:0").cpu().numpy().tobytes()


def test_batch_with_a_damaged_file_and_the_device_buffer():
    RG.check_batch(M, _fetch)


def test_regions_of_a_full_size_batch():
    """4 distinct 1920x1080 4:2:0 q75 files with a restart interval of one MCU row in one call: a region wider than a wave's 64
    blocks, a narrow one, one at 1/2 scale, then the whole images on the same encoder"""
    files = [TC.cjpeg(O.synthetic_frame(1920, 1080, seed=200 + i), ["-revert", "-quality", "75", "-sample", "2x2", "-restart", "1"]) for i in range(4)]
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True), max_batch=4)
    for r, scale in (((301, 411, 1100, 300), None), ((1000, 37, 256, 256), None), ((131, 77, 500, 333), "1/2")):
        outs = enc.decode_host(files, crop=r, scale=scale)
        kept, total = enc.decode_segments()
        assert total == 4 * 68 and kept < total
        for i, (f, o) in enumerate(zip(files, outs)):
            assert SC.same(o, RG.reference_file(f, ("-crop", RG.crop_arg(r)) + (("-scale", scale) if scale else ()))), "file %d, %s at %s" % (i, r, scale)
    outs = enc.decode_host(files)
    for i, (f, o) in enumerate(zip(files, outs)):
        assert SC.same(o, RG.reference_file(f, ())), "file %d at full size" % i
    enc.close()


# ---- the TurboJPEG library, MOZJPEG_HIP_REGIONS=1 ---------------------------------------------------------------------------------------
import json  # noqa: E402
import os  # noqa: E402
import subprocess  # noqa: E402
import sys  # noqa: E402

import tj_decompress_cases as TD  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_tj = pytest.mark.skipif(not TD.have_tools(), reason="reference binaries (oracle/_ref) or the TurboJPEG-signature library are not built")


@pytest.fixture(scope="module")
def tj_results():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + sys.path))
    env.pop("MOZJPEG_HIP_TJ_DECOMPRESS", None)
    env.pop(RG.ENV, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "region_cases.py"), TD.TJSHIM], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("REGION_TJ_RESULTS ")]
    assert r.returncode == 0 and lines, "the child ended with %d: %s" % (r.returncode, r.stderr.decode()[-2000:])
    return json.loads(lines[-1].split(" ", 1)[1])


@needs_tj
@pytest.mark.parametrize("name", list(RG.TJ_CHECKS))
def test_turbojpeg_library(tj_results, name):
    assert tj_results[name] == "ok", tj_results[name]


# ---- the stand-alone libjpeg.so.62, MOZJPEG_HIP_REGIONS=1 -----------------------------------------------------------------------------
import djpeg_cases as DJ  # noqa: E402

STANDALONE = os.path.join(ROOT, "mozjpeg_amd", "standalone")
needs_djpeg = pytest.mark.skipif(not DJ.have_tools(), reason="reference djpeg / libjpeg.so.62 or tests/native/djpeg_client not built")


@needs_djpeg
@pytest.mark.parametrize("src,switches", RG.DJPEG_PAIRS, ids=["%s-%s" % p for p in RG.DJPEG_PAIRS])
def test_unchanged_djpeg_with_the_variable(src, switches):
    RG.check_djpeg(DJ.Runner(STANDALONE, env={RG.ENV: "1"}), src, switches)


@needs_djpeg
def test_unchanged_djpeg_refuses_without_the_variable():
    RG.check_djpeg_refuses_without_the_variable(DJ.Runner(STANDALONE))


@needs_client
@pytest.mark.parametrize("case", list(RG.CLIENT_CASES))
def test_libjpeg_client_on_both_libraries(case):
    RG.check_client(STANDALONE, {RG.ENV: "1"}, case)
