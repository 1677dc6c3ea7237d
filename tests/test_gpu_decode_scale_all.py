"""GPU (-m gpu): decoding at the twelve other IDCT sizes on the chip (mjh_decode_opts.all_scales: djpeg -scale 3/8, 5/8, 6/8, 7/8,
9/8 to 16/8; k_idct_sized of mjh_idct.hip, then the colour kernels on planes that may be larger than the full-size ones).  Every
expected pixel comes from the reference's djpeg -scale at test time and is compared for exact equality, the array shape included
(tests/scale_all_cases.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mozjpeg_amd as M
import oracle_lib as O
import decode_cases as DC
import djpeg_cases as DJ
import scale_all_cases as SA
import scale_cases as SC
import tj_decompress_cases as TD
import transcode_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not SA.have_tools(), reason="reference cjpeg / jpegtran / djpeg not built (oracle/_ref)")]
needs_djpeg = pytest.mark.skipif(not DJ.have_tools(), reason="reference djpeg / libjpeg.so.62 or tests/native/djpeg_client not built")
needs_tj = pytest.mark.skipif(not TD.have_tools(), reason="reference binaries (oracle/_ref) or the TurboJPEG-signature library are not built")


@pytest.mark.parametrize("src,mode,k", SA.CASES, ids=[SA.case_id(c) for c in SA.CASES])
def test_every_new_size_matches_djpeg(src, mode, k):
    SA.check_case(M, src, mode, k)


def test_every_transform_size_is_reached():
    SA.check_every_transform_size_is_reached(M)


@pytest.mark.parametrize("src,frac", SA.FRACTION_CASES, ids=[SA.case_id(c) for c in SA.FRACTION_CASES])
def test_fraction_is_resolved_as_djpeg_does(src, frac):
    SA.check_fraction(M, src, frac)


@pytest.mark.parametrize("src,k", SA.LAYOUT_CASES, ids=[SA.case_id(c) for c in SA.LAYOUT_CASES])
def test_layouts_and_colour_kernels(src, k):
    SA.check_layouts(M, src, k)


def test_four_component_files():
    SA.check_four_components(M)


def test_progressive_and_arithmetic_sources():
    SA.check_other_entropy_coders(M)


class _DeviceView:
    """device memory as an object torch can wrap without a copy"""

    def __init__(self, ptr, shape, strides):
        self.__cuda_array_interface__ = dict(shape=shape, strides=strides, typestr="|u1", data=(ptr, False), version=2)


def _fetch(ptr, nbytes):
    import torch
    return torch.as_tensor(_DeviceView(ptr, (nbytes,), (1,)), device="cuda:0").cpu().numpy().tobytes()


@pytest.mark.parametrize("src,k", SA.PLANE_CASES, ids=[SA.case_id(c) for c in SA.PLANE_CASES])
def test_raw_planes(src, k):
    SA.check_planes(M, src, k)
    SA.check_device_planes(M, src, k, _fetch)


def test_one_encoder_serves_every_scale():
    SA.check_one_encoder_serves_every_scale(M)


def test_mixed_batch_with_a_damaged_file():
    SA.check_mixed_batch(M)


def test_the_opt_in_is_the_only_door():
    SA.check_opt_in(M)


@pytest.mark.parametrize("k", [3, 13])
@pytest.mark.parametrize("kw", [dict(), dict(layout="bgrx"), dict(color="gray")], ids=["rgb", "bgrx", "gray"])
def test_device_buffer_addresses_the_scaled_image(kw, k):
    """mjh_get_pixels_device against mjh_get_pixels: pitch and stride of the scaled rows, padded by the full-size rules"""
    import torch
    files = DC.batch_files()
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True), max_batch=3)
    host = enc.decode_host(files, scale=(k, 8), all_scales=True, **kw)
    enc.submit_decode(files, scale=(k, 8), all_scales=True, **kw)
    enc.wait_decode()
    ptr, pitch, stride, st = enc.pixels_device()
    h, w, px = st["height"], st["width"], st["pixel_size"]
    info = M.jpeg_info(files[0])
    assert (h, w) == (-(-info.image_height * k // 8), -(-info.image_width * k // 8))
    assert pitch == (px * ((w + 3) & ~3) + 15) & ~15 and stride == pitch * h
    t = torch.as_tensor(_DeviceView(ptr, (3, h, w, px), (stride, pitch, px, 1)), device="cuda:0")
    got = t.cpu().numpy()
    for i in range(3):
        assert np.array_equal(got[i] if px > 1 else got[i, :, :, 0], host[i])
        if not kw:
            assert SC.same(host[i], DC.djpeg(files[i], ["-scale", SA.arg(k)]))
    enc.close()


def test_full_size_batch_at_new_scales():
    """4 distinct 1920x1080 4:2:0 q75 files in one call at 3/8, 3/4, 11/8 and 2/1, then at full size on the same encoder"""
    files = [TC.cjpeg(O.synthetic_frame(1920, 1080, seed=100 + i), ["-revert", "-quality", "75", "-sample", "2x2"]) for i in range(4)]
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True), max_batch=4)
    for scale in ("3/8", "3/4", "11/8", "2/1"):
        outs = enc.decode_host(files, scale=scale, all_scales=True)
        for i, (f, o) in enumerate(zip(files, outs)):
            assert SC.same(o, DC.djpeg(f, ["-scale", scale])), "file %d at %s" % (i, scale)
    outs = enc.decode_host(files)
    for i, (f, o) in enumerate(zip(files, outs)):
        assert SC.same(o, DC.djpeg(f)), "file %d at full size" % i
    enc.close()


# ---- the drop-in libraries --------------------------------------------------------------------------------------------------------
STANDALONE = os.path.join(ROOT, "mozjpeg_amd", "standalone")


@needs_djpeg
@pytest.mark.parametrize("src,switches", SA.DJPEG_PAIRS, ids=["%s-%s" % p for p in SA.DJPEG_PAIRS])
def test_unchanged_djpeg_with_the_variable(src, switches):
    SA.check_djpeg(DJ.Runner(STANDALONE, env={SA.ENV: "1"}), src, switches)


@needs_djpeg
def test_unchanged_djpeg_refuses_without_the_variable():
    SA.check_djpeg_refuses_without_the_variable(DJ.Runner(STANDALONE))


@pytest.fixture(scope="module")
def tj_results():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + sys.path))
    env.pop("MOZJPEG_HIP_TJ_DECOMPRESS", None)
    env.pop(SA.ENV, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "scale_all_cases.py"), TD.TJSHIM], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("SCALE_ALL_TJ_RESULTS ")]
    assert r.returncode == 0 and lines, "the child ended with %d: %s" % (r.returncode, r.stderr.decode()[-2000:])
    return json.loads(lines[-1].split(" ", 1)[1])


@needs_tj
@pytest.mark.parametrize("name", list(SA.TJ_CHECKS))
def test_turbojpeg_library(tj_results, name):
    assert tj_results[name] == "ok", tj_results[name]
