"""GPU suite: lossless scan scripts (SOF3 files of several scans) through the C ABI and the Python binding against
`oracle/_ref/cjpeg -revert -lossless 1 -scans FILE`, whole files byte for byte: the images of tests/lossless_cases.py (random, flat,
smooth, extreme) at 8 / 12 / 16 bits and widths 1, 37, 1300, 2100 (the last wider than 2 * LL_UNIT), batches of different images
in one call and calls back to back, and the scripts the reference refuses with its reasons."""
import os
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import mozjpeg_amd as M
import lossless_cases as LC
import lossless_script_cases as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DJPEG = os.path.join(ROOT, "oracle", "_ref", "djpeg")


def _refs(frames, script, prec, rst=None):
    with ThreadPoolExecutor(8) as ex:
        out = list(ex.map(lambda f: SC.reference(f, script, prec, rst), frames))
    for r in out:
        assert isinstance(r, bytes), r
    return out


def _ours(a, script, prec, rst=None):
    return M.Encoder(SC.params(M, a, script, prec, rst), max_batch=1).encode_host(a)[0]


@pytest.mark.parametrize("prec", [8, 12, 16])
@pytest.mark.parametrize("width", [1, 37, 1300, 2100])
def test_scripts_match_reference(prec, width):
    bad = []
    for kind in ("random", "flat", "smooth", "extreme"):
        for name, rst in (("each", None), ("one_two", 2), ("two_one", None), ("each_mixed", 1)):
            h = 5 if width > 1000 else 23
            a = LC.image(kind, h, width, 3, prec, seed=width)
            script = SC.script_of(name)
            ref = SC.reference(a, script, prec, rst)
            assert isinstance(ref, bytes), ref
            out = _ours(a, script, prec, rst)
            print("%s %s p%d w%d r%s: %d bytes, reference %d" % (kind, name, prec, width, rst, len(out), len(ref)))
            if out != ref:
                bad.append((kind, name, rst))
    assert not bad


@pytest.mark.parametrize("prec", [8, 16])
def test_gray_one_scan_script(prec):
    for width, rst in ((37, None), (2100, 3)):
        a = LC.image("smooth", 7, width, 1, prec)
        assert _ours(a, SC.GRAY_ONE, prec, rst) == _refs([a], SC.GRAY_ONE, prec, rst)[0]


@pytest.mark.parametrize("prec,name,rst", [(8, "each", None), (8, "one_two", 2), (12, "two_one", 1), (16, "each_mixed", 4)])
def test_batches_of_different_images_and_back_to_back(prec, name, rst):
    """several different images in one call, two calls back to back on the same encoder, then a smaller batch"""
    script = SC.script_of(name)
    kinds = ["random", "smooth", "extreme", "flat", "smooth"]
    fa = [LC.image(k, 31, 1300, 3, prec, seed=i) for i, k in enumerate(kinds)]
    fb = [LC.image(k, 31, 1300, 3, prec, seed=10 + i) for i, k in enumerate(reversed(kinds))]
    ra, rb = _refs(fa, script, prec, rst), _refs(fb, script, prec, rst)
    enc = M.Encoder(SC.params(M, fa[0], script, prec, rst), max_batch=len(fa))
    oa = enc.encode_host(np.stack(fa))
    ob = enc.encode_host(np.stack(fb))
    assert oa == ra and ob == rb
    assert enc.encode_host(np.stack(fb[:2])) == rb[:2]
    assert len(set(oa)) == len(oa)


def test_one_scan_script_is_the_one_scan_file():
    """a script of one scan holding all components is the file `-lossless psv,pt` gives"""
    a = LC.image("smooth", 19, 1300, 3, 8)
    assert _ours(a, [((0, 1, 2), 5, 1)], 8, 2) == LC.reference(a, 5, 1, 8, 2)


@pytest.mark.parametrize("prec", [8, 12, 16])
def test_script_decodes_to_the_input(prec):
    """independent of the byte comparison: with Pt = 0 the reference's decoder returns the samples"""
    a = LC.image("random", 10, 1100, 3, prec)
    out = _ours(a, SC.EACH, prec, 2)
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "x.jpg")
        with open(f, "wb") as fh:
            fh.write(out)
        r = subprocess.run([DJPEG, "-pnm", f], capture_output=True)
    assert r.returncode == 0, r.stderr
    want = a.astype(">u2" if prec > 8 else np.uint8).tobytes()
    assert r.stdout.endswith(want) and len(r.stdout) - len(want) < 32


@pytest.mark.parametrize("what", sorted(SC.REFUSED))
def test_refused_scripts_keep_the_reference_reason(what):
    script, code, words = SC.REFUSED[what]
    a = LC.image("random", 8, 10, 3, 8)
    ref = SC.reference(a, script, 8)
    assert not isinstance(ref, bytes) and words in ref[1], ref
    with pytest.raises(M.MjhError) as ei:
        M.Encoder(SC.params(M, a, script, 8), max_batch=1)
    assert code in str(ei.value) and words in str(ei.value)
