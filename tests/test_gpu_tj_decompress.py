"""GPU (-m gpu): TurboJPEG decompress instances of mozjpeg_amd/libmozjpeg_hip_turbojpeg.so (tj_shim.c) on the chip, against the
reference's oracle/_ref/libturbojpeg.so.0 loaded side by side: the same calls on both, the bytes they leave compared for exact
equality, the destination's padding included (tests/tj_decompress_cases.py).  The library runs the real device library: under
--simt the checks skip themselves (test_simt_tj_decompress.py runs them over the emulator)."""
import os

import pytest

import mozjpeg_amd as M
import tj_decompress_cases as TD

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not TD.have_tools(), reason="reference binaries (oracle/_ref) or the TurboJPEG-signature library are not built")]


@pytest.fixture(scope="module")
def libs():
    if "simt" in os.path.basename(M.LIB_PATH or ""):
        pytest.skip("the TurboJPEG-signature library is linked to the device library, not to the emulator")
    return TD.load(TD.TJSHIM), TD.load(TD.TJLIB)


@pytest.mark.parametrize("name", list(TD.CHECKS))
def test_tj_decompress(libs, name):
    TD.CHECKS[name](*libs)


def test_forwarding_switch():
    TD.check_forwarding_switch(TD.TJSHIM)
