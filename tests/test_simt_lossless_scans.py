"""CPU suite: lossless scan scripts (SOF3 files of several scans) through the C ABI and the Python binding, the kernels of
mozjpeg_amd/csrc/mjh_lossless.hip executed by the lock-step wave64 emulator (tools/simt), against
`oracle/_ref/cjpeg -revert -lossless 1 -scans FILE` byte for byte (lossless_script_cases.SIMT_CASES, the sizes of
tests/test_simt_lossless.py).  The refusals are host-side and carry the reference's reason.  The same scripts run on the chip in
tests/test_gpu_lossless_scans.py."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import mozjpeg_amd as M
import lossless_cases as LC
import lossless_script_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "simt"))
DJPEG = os.path.join(ROOT, "oracle", "_ref", "djpeg")

pytestmark = pytest.mark.skipif(not os.path.exists(LC.CJPEG), reason="reference binaries (oracle/_ref) are not built")


@pytest.fixture(scope="module")
def simt():
    """the ctypes layer bound to the emulator's library for this module only"""
    import build_simt
    path = build_simt.build()
    saved = (M.LIB_PATH, M._lib)
    M.LIB_PATH, M._lib = path, None
    try:
        yield path
    finally:
        M.LIB_PATH, M._lib = saved


@pytest.mark.parametrize("case", SC.SIMT_CASES, ids=SC.case_id)
def test_script_matches_reference(simt, case):
    kind, h, w, comps, prec, name, rst = case
    a = LC.image(kind, h, w, comps, prec)
    script = SC.script_of(name)
    ref = SC.reference(a, script, prec, rst)
    assert isinstance(ref, bytes), ref
    out = M.Encoder(SC.params(M, a, script, prec, rst), max_batch=1).encode_host(a)[0]
    assert out == ref


def test_script_file_layout(simt):
    """SOF3 once, then per scan DHT (class 0, id 0) + SOS naming table 0 for every component with Ss / Al of THAT scan; the DRI in
    front of the first SOS only (write_scan_header jcmarker.c:778-781)"""
    a = LC.image("smooth", 9, 20, 3, 8)
    out = M.Encoder(SC.params(M, a, SC.ONE_TWO, 8, 2), max_batch=1).encode_host(a)[0]
    assert out.count(b"\xff\xc3") == 1 and out.count(b"\xff\xdd\x00\x04\x00\x28") == 1
    first = out.index(b"\xff\xda\x00\x08\x01R\x00\x04\x00\x00")
    second = out.index(b"\xff\xda\x00\x0a\x02G\x00B\x00\x02\x00\x01")
    assert out.index(b"\xff\xdd") < first < second
    assert b"\xff\xc4" in out[:first]
    assert b"\xff\xc4" in out[first:second]          # the second scan's own table, between the scans


def test_script_batch_of_distinct_images_and_back_to_back(simt):
    """one call, three different images, twice: every file is the reference's for its image"""
    imgs = [LC.image("smooth", 13, 47, 3, 8, seed=s) for s in range(3)] + [LC.image("random", 13, 47, 3, 8, seed=9)]
    p = SC.params(M, imgs[0], SC.EACH_MIXED, 8, 3)
    enc = M.Encoder(p, max_batch=3)
    refs = [SC.reference(a, SC.EACH_MIXED, 8, 3) for a in imgs]
    assert enc.encode_host(np.stack(imgs[:3])) == refs[:3]
    assert enc.encode_host(np.stack(imgs[1:])) == refs[1:]
    assert enc.encode_host(np.stack(imgs[3:])) == refs[3:]     # a smaller batch on the same encoder


def test_script_decodes_to_the_input(simt):
    """independent of the byte comparison: with Pt = 0 the reference's decoder returns the samples"""
    a = LC.image("random", 10, 21, 3, 8)
    out = M.Encoder(SC.params(M, a, SC.EACH, 8), max_batch=1).encode_host(a)[0]
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "x.jpg")
        with open(f, "wb") as fh:
            fh.write(out)
        r = subprocess.run([DJPEG, "-pnm", f], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.endswith(a.tobytes()) and r.stdout.startswith(b"P6\n21 10\n255\n")


def test_last_scan_table_is_what_the_taps_read(simt):
    """the object's DC table 0 after the image is the LAST scan's (every scan re-defines table 0)"""
    a = LC.image("smooth", 10, 21, 3, 8)
    enc = M.Encoder(SC.params(M, a, SC.ONE_TWO, 8), max_batch=1)
    enc.encode_host(a)
    counts = np.zeros(17, np.uint32)
    n = M.C.c_size_t()
    M._chk(M.lib().mjh_read_tap(enc._h, M.TAP_LL_COUNTS, 0, 0, counts.ctypes.data, counts.nbytes, M.C.byref(n)))
    assert counts.sum() == 2 * 10 * 21            # the two components of the second scan


@pytest.mark.parametrize("what", sorted(SC.REFUSED))
def test_refused_scripts_keep_the_reference_reason(simt, what):
    script, code, words = SC.REFUSED[what]
    a = LC.image("random", 8, 10, 3, 8)
    ref = SC.reference(a, script, 8)
    assert not isinstance(ref, bytes) and words in ref[1], ref
    with pytest.raises(M.MjhError) as ei:
        M.Encoder(SC.params(M, a, script, 8), max_batch=1)
    assert code in str(ei.value) and words in str(ei.value)
