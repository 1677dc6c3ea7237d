"""GPU suite: lossless mode (SOF3) through the two libjpeg libraries.  The reference's unchanged `cjpeg -lossless psv,Pt` and
`cjpeg -lossless 1 -scans FILE` run with the interposing library in front of the reference's libjpeg and on the stand-alone
libjpeg.so.62 alone; expected bytes (or exit status and message) = the same binary on the reference's library
(tests/lossless_dropin_cases.py).  Whole-file byte equality everywhere."""
import hashlib
import os

import numpy as np
import pytest

import lossless_cases as LC
import lossless_dropin_cases as D

ROOT = D.ROOT
SHIM = os.path.join(ROOT, "mozjpeg_amd", "libmozjpeg_hip_jpeg62.so")
STANDALONE_DIR = os.path.join(ROOT, "mozjpeg_amd", "standalone")

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not (os.path.exists(D.CJPEG) and os.path.exists(SHIM) and os.path.exists(os.path.join(STANDALONE_DIR, "libjpeg.so.62"))),
                                 reason="reference binaries (oracle/_ref) or the drop-in libraries are not built")]


def three(args, inp, tmp, name="o"):
    return D.run_three(args, inp, tmp, SHIM, STANDALONE_DIR, name)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory, fixture_images):
    return D.write_inputs(tmp_path_factory.mktemp("ll_in"), fixture_images["testorig"])


@pytest.mark.parametrize("prec", [8, 12, 16])
def test_pinned_command_reproduces_the_references_md5(prec, tmp_path):
    res = three(D.precision_args(prec) + D.PINNED_ARGS, D.PPM, tmp_path)
    for which, rc, err, data in res:
        assert rc == 0, (which, err)
        print(which, hashlib.md5(data).hexdigest(), len(data))
        assert hashlib.md5(data).hexdigest() == D.PINNED_MD5[prec], which


@pytest.mark.parametrize("prec", [8, 12, 16])
def test_every_predictor_and_point_transform(prec, tmp_path):
    bad = []
    for psv in range(1, 8):
        for pt in (0, 1, prec - 1):
            args = ["-revert", "-lossless", "%d,%d" % (psv, pt)] + D.precision_args(prec)
            bad += D.complaints(three(args, D.PPM, tmp_path), "psv %d pt %d" % (psv, pt))
    assert not bad, bad


@pytest.mark.parametrize("restart", ["1", "3"])
def test_restart_rows(restart, tmp_path):
    assert not D.complaints(three(["-revert", "-lossless", "5", "-restart", restart], D.PPM, tmp_path))
    assert not D.complaints(three(["-revert", "-lossless", "2,1", "-precision", "16", "-restart", restart], D.PPM, tmp_path))


@pytest.mark.parametrize("kind,args", [
    ("pgm", ["-revert", "-lossless", "3"]),
    ("pgm", ["-revert", "-lossless", "7,2", "-precision", "12", "-restart", "2"]),
    ("pnm16", ["-revert", "-lossless", "1", "-precision", "16"]),
    ("pnm16", ["-revert", "-lossless", "6,3", "-precision", "16", "-restart", "1"]),
    ("pgm16", ["-revert", "-lossless", "4", "-precision", "16"]),
    ("pnm12", ["-revert", "-lossless", "2", "-precision", "12"]),
    ("bmp", ["-revert", "-lossless", "4"]),
    ("tga", ["-revert", "-lossless", "1,1", "-targa"]),
    ("1x1", ["-revert", "-lossless", "1"]),
    ("1x1", ["-revert", "-lossless", "7", "-precision", "16", "-restart", "1"]),
    ("1xN", ["-revert", "-lossless", "5", "-restart", "3"]),
    ("Nx1", ["-revert", "-lossless", "6"]),
    ("wide", ["-revert", "-lossless", "4", "-restart", "2"]),
    ("wide", ["-revert", "-lossless", "7,1", "-precision", "12"]),
])
def test_readers_and_sizes(kind, args, inputs, tmp_path):
    files, _ = inputs
    res = three(args, files[kind], tmp_path)
    assert res[0][1] == 0, res[0][2]
    assert not D.complaints(res)


@pytest.mark.parametrize("prec", [8, 16])
@pytest.mark.parametrize("restart", [None, "2"])
@pytest.mark.parametrize("name", sorted(D.SCRIPTS))
def test_lossless_scan_scripts(name, restart, prec, tmp_path):
    script, size = D.SCRIPTS[name]
    sf = D.write_script(tmp_path, name, script)
    args = ["-revert", "-lossless", "1"] + D.precision_args(prec) + (["-restart", restart] if restart else []) + ["-scans", sf]
    res = three(args, D.PPM, tmp_path)
    assert res[0][1] == 0, res[0][2]
    if prec == 8 and restart is None:
        assert len(res[0][3]) == size
    assert not D.complaints(res)


def test_one_scan_script_on_gray_input(inputs, tmp_path):
    files, _ = inputs
    sf = D.write_script(tmp_path, "gray", "0: 6-0,0,1;\n")
    res = three(["-revert", "-lossless", "1", "-scans", sf], files["pgm"], tmp_path)
    assert res[0][1] == 0 and not D.complaints(res)


def test_script_without_the_lossless_switch(tmp_path):
    """validate_script switches lossless mode on from the script alone (jcmaster.c:302-311): whatever the reference does"""
    sf = D.write_script(tmp_path, "s", D.SCRIPTS["one_two"][0])
    res = three(["-revert", "-scans", sf], D.PPM, tmp_path)
    assert not D.complaints(res)
    assert res[0][1] == 0 and b"\xff\xc3" in res[0][3][:64]


@pytest.mark.parametrize("args", [["-revert", "-lossless", "1", "-progressive"], ["-revert", "-progressive", "-lossless", "1"]])
def test_progressive_switches_lossless_off_again(args, tmp_path):
    """jpeg_simple_progression clears the lossless flag (jcparam.c:876-878): the progressive DCT file the reference writes"""
    res = three(["-dct", "int"] + args, D.PPM, tmp_path)
    assert res[0][1] == 0 and b"\xff\xc2" in res[0][3][:700] and not D.complaints(res)


def test_refusals_are_the_references(tmp_path):
    bad = []
    for what, args in D.refusal_commands(tmp_path).items():
        res = three(args, D.PPM, tmp_path)
        print(what, res[0][1], res[0][2].strip())
        assert res[0][1] != 0, what
        bad += D.complaints(res, what)
    assert not bad, bad


@pytest.mark.parametrize("prec", [8, 12, 16])
def test_decodes_to_the_input(prec, inputs, tmp_path, fixture_images):
    """independent of the byte comparison: with Pt = 0 the reference's djpeg returns the input samples"""
    files, arrays = inputs
    src, a = (D.PPM, fixture_images["testorig"]) if prec == 8 else (files["pnm%d" % prec], arrays["pnm%d" % prec])
    for which, rc, err, data in three(["-revert", "-lossless", "4", "-restart", "3"] + D.precision_args(prec), src, tmp_path)[1:]:
        assert rc == 0, (which, err)
        want = np.ascontiguousarray(a).astype(">u2" if prec > 8 else np.uint8).tobytes()
        got = D.djpeg_pixels(data, tmp_path)
        assert got.endswith(want) and len(got) - len(want) < 32, which
