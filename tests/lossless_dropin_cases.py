"""Lossless mode through the two libjpeg libraries, shared by tests/test_gpu_lossless_dropin.py (the chip) and
tests/test_simt_lossless_dropin.py (the wave64 emulator): the reference's UNCHANGED cjpeg runs three times per command line -- on
the reference's own libjpeg (the expected bytes, exit status and stderr), with the interposing library in front of it, and on the
stand-alone libjpeg.so.62 alone.  Comparison is whole-file byte equality; a refusal has the reference's exit status and message."""
import os
import subprocess

import numpy as np

import lossless_cases as LC
import lossless_script_cases as SC
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CJPEG = os.path.join(O.REF_DIR, "cjpeg")
DJPEG = os.path.join(O.REF_DIR, "djpeg")
PPM = os.path.join(ROOT, "tests", "golden", "testorig.ppm")

# The command the reference's own test suite pins ("all arguments other than -lossless and -restart should have no effect",
# CMakeLists.txt:1261-1266 and :1651-1656) and its MD5_JPEG_LOSSLESS for 16, 12 and 8 bits (CMakeLists.txt:1258, :1328, :1409)
PINNED_ARGS = ["-revert", "-lossless", "4", "-restart", "1", "-quality", "1", "-grayscale", "-optimize", "-dct", "float", "-smooth", "100",
               "-baseline", "-qslots", "1,0,0", "-sample", "1x2,3x4,2x1"]
PINNED_MD5 = {16: "fe99437df4e9976fe5e841969242b208", 12: "8473501f5bb7c826524472c858bf4fcd", 8: "fc777b82d42d835ae1282ba1ee87c209"}

# the scripts checked against the reference when the feature was specified (sizes on testorig.ppm at 8 bits, no restarts)
SCRIPTS = {"each": (SC.EACH, 59093), "one_two": (SC.ONE_TWO, 46887), "two_one": (SC.TWO_ONE, 41414)}


def precision_args(prec):
    return ["-precision", str(prec)] if prec != 8 else []


def run_three(args, inp, tmp, shim, standalone_dir, name="o"):
    """[(which, returncode, stderr, file bytes or None)] for the reference, the interposer and the stand-alone library"""
    out = []
    for which in ("reference", "interposer", "stand-alone"):
        env = dict(os.environ)
        O.set_preload(env, shim if which == "interposer" else None)
        env["LD_LIBRARY_PATH"] = standalone_dir if which == "stand-alone" else O.REF_DIR
        f = os.path.join(str(tmp), "%s_%s.jpg" % (name, which))
        if os.path.exists(f):
            os.remove(f)
        r = subprocess.run([CJPEG] + list(args) + ["-outfile", f, inp], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
        data = None
        if r.returncode == 0 and os.path.exists(f):
            with open(f, "rb") as fh:
                data = fh.read()
        out.append((which, r.returncode, r.stderr.decode(errors="replace"), data))
    return out


def complaints(res, what=""):
    """both libraries against the reference: the same file, or the same refusal"""
    (_, rc0, err0, want), bad = res[0], []
    for which, rc, err, got in res[1:]:
        if rc0 != 0:
            if rc != rc0 or err.strip() != err0.strip():
                bad.append("%s %s: exit %d %r, the reference exit %d %r" % (what, which, rc, err.strip()[-200:], rc0, err0.strip()[-200:]))
        elif rc != 0:
            bad.append("%s %s: exit %d %s" % (what, which, rc, err.strip()[-300:]))
        elif got != want:
            bad.append("%s %s: DIFFERENT (%d vs %d bytes)" % (what, which, len(got or b""), len(want or b"")))
    return bad


def write_script(tmp, name, script):
    f = os.path.join(str(tmp), name + ".scans")
    with open(f, "w") as fh:
        fh.write(script if isinstance(script, str) else SC.script_text(script))
    return f


def write_inputs(tmp, img):
    """img: [H, W, 3] uint8 (testorig).  Returns {name: path} of the other input kinds"""
    tmp = str(tmp)
    h, w = img.shape[:2]
    le = lambda v, n: int(v).to_bytes(n, "little")   # noqa: E731
    files = {}
    files["pgm"] = os.path.join(tmp, "in.pgm")
    with open(files["pgm"], "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (w, h) + img[:, :, 1].tobytes())
    a16 = LC.image("smooth", 23, 61, 3, 16)
    files["pnm16"] = os.path.join(tmp, "in16.ppm")
    LC.write_pnm(files["pnm16"], a16, 16)
    files["pgm16"] = os.path.join(tmp, "in16.pgm")
    LC.write_pnm(files["pgm16"], LC.image("random", 9, 40, 1, 16), 16)
    a12 = LC.image("smooth", 23, 61, 3, 12)
    files["pnm12"] = os.path.join(tmp, "in12.ppm")
    LC.write_pnm(files["pnm12"], a12, 12)
    row = (w * 3 + 3) & ~3
    body = b"".join(img[y, :, ::-1].tobytes() + b"\0" * (row - 3 * w) for y in range(h - 1, -1, -1))
    files["bmp"] = os.path.join(tmp, "in.bmp")
    with open(files["bmp"], "wb") as f:
        f.write(b"BM" + le(54 + len(body), 4) + le(0, 4) + le(54, 4) + le(40, 4) + le(w, 4) + le(h, 4) + le(1, 2) + le(24, 2) + le(0, 4) +
                le(len(body), 4) + le(2835, 4) * 2 + le(0, 4) * 2 + body)
    hdr = bytearray(18)
    hdr[2] = 2
    hdr[12:14] = w.to_bytes(2, "little")
    hdr[14:16] = h.to_bytes(2, "little")
    hdr[16] = 24
    files["tga"] = os.path.join(tmp, "in.tga")
    with open(files["tga"], "wb") as f:
        f.write(bytes(hdr) + img[::-1, :, ::-1].tobytes())
    for name, a in (("1x1", img[:1, :1]), ("1xN", img[:, :1]), ("Nx1", img[:1, :])):
        files[name] = os.path.join(tmp, "in_%s.ppm" % name)
        LC.write_pnm(files[name], np.ascontiguousarray(a), 8)
    files["wide"] = os.path.join(tmp, "in_wide.ppm")          # wider than 2 * LL_UNIT = 2048 pixels
    LC.write_pnm(files["wide"], LC.image("smooth", 5, 2100, 3, 8), 8)
    return files, {"pnm16": a16, "pnm12": a12}


def djpeg_pixels(jpeg_bytes, tmp):
    """the reference's decoder on a file: the PNM it writes"""
    f = os.path.join(str(tmp), "dj_in.jpg")
    with open(f, "wb") as fh:
        fh.write(jpeg_bytes)
    env = dict(os.environ)
    O.set_preload(env)
    env["LD_LIBRARY_PATH"] = O.REF_DIR
    r = subprocess.run([DJPEG, "-pnm", f], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr
    return r.stdout


# what the reference refuses: the same exit status and the same message on stderr
def refusal_commands(tmp):
    twice = write_script(tmp, "twice", "0: 1-0,0,0;\n0,1: 1-0,0,0;\n2: 1-0,0,0;\n")
    return {
        "trellis_on (no -revert)": ["-lossless", "1"],
        "arithmetic": ["-revert", "-lossless", "1", "-arithmetic"],
        "restart_5_blocks": ["-revert", "-lossless", "1", "-restart", "5B"],      # 5 does not divide into the width
        "component_twice": ["-revert", "-lossless", "1", "-scans", twice],
        "precision16_lossy": ["-revert", "-precision", "16"],
    }
