"""Lossless scan scripts (SOF3 files of several scans) shared by tests/test_simt_lossless_scans.py and tests/test_gpu_lossless_scans.py:
the scripts, the text of a cjpeg -scans file for them, the reference's answer through `oracle/_ref/cjpeg -revert -lossless 1 -scans FILE`
(built by oracle/Makefile) and the parameter sets of this library for the same script.  Images come from tests/lossless_cases.py."""
import os
import subprocess
import tempfile

import lossless_cases as LC

# a script: [(component indices, predictor Ss, point transform Al), ...]; what validate_script (jcmaster.c:302-311, :390-416) accepts
# for three components -- one scan per component, luma alone + the other two together, two together + the last alone
EACH = [((0,), 1, 0), ((1,), 1, 0), ((2,), 1, 0)]
ONE_TWO = [((0,), 4, 0), ((1, 2), 2, 1)]
TWO_ONE = [((0, 1), 7, 2), ((2,), 1, 0)]
EACH_MIXED = [((0,), 5, 0), ((1,), 6, 3), ((2,), 3, 1)]
RGB_SCRIPTS = {"each": EACH, "one_two": ONE_TWO, "two_one": TWO_ONE, "each_mixed": EACH_MIXED}
GRAY_ONE = [((0,), 6, 1)]          # a one-scan script on gray input


def script_text(script):
    """the -scans file (read_scan_script rdswitch.c: `components: Ss-Se, Ah, Al;`)"""
    return "".join("%s: %d-0,0,%d;\n" % (",".join(str(c) for c in comps), ss, al) for comps, ss, al in script)


def reference(a, script, precision, restart=None, extra=(), lossless="1"):
    """the reference's file for the script (the -lossless switch only turns the mode on: the script's own Ss / Al count), or
    (returncode, stderr) when it refuses.  script: a list as above, or the text of a -scans file."""
    with tempfile.TemporaryDirectory() as d:
        f, sf = os.path.join(d, "in.pnm"), os.path.join(d, "scans.txt")
        LC.write_pnm(f, a, precision)
        with open(sf, "w") as fh:
            fh.write(script if isinstance(script, str) else script_text(script))
        args = ["-revert"] + (["-lossless", lossless] if lossless else [])
        if precision != 8:
            args += ["-precision", str(precision)]
        if restart is not None:
            args += ["-restart", str(restart)]
        r = subprocess.run([LC.CJPEG] + args + ["-scans", sf] + list(extra) + [f], capture_output=True)
    if r.returncode != 0:
        return r.returncode, r.stderr.decode(errors="replace")
    return r.stdout


def params(M, a, script, precision, restart=None):
    h, w, c = a.shape
    return M.make_params(w, h, revert=True, lossless=(1, 0), precision=precision, grayin=c == 1, restart=restart,
                         scans=[(comps, ss, 0, 0, al) for comps, ss, al in script])


# the emulator slice: (kind, h, w, comps, precision, script name, restart)
SIMT_CASES = [
    ("random", 1, 1, 3, 8, "each", None),
    ("smooth", 29, 47, 3, 8, "each", None),
    ("smooth", 29, 47, 3, 8, "one_two", 2),
    ("random", 29, 47, 3, 8, "two_one", 1),
    ("random", 53, 1, 3, 8, "each_mixed", 3),
    ("smooth", 7, 1300, 3, 8, "one_two", 2),
    ("smooth", 21, 33, 3, 12, "each_mixed", None),
    ("extreme", 11, 41, 3, 16, "each", 2),
    ("random", 19, 25, 3, 16, "two_one", None),
    ("random", 19, 25, 1, 16, "gray_one", 5),
    ("smooth", 1, 37, 1, 8, "gray_one", None),
]


def script_of(name):
    return GRAY_ONE if name == "gray_one" else RGB_SCRIPTS[name]


def case_id(c):
    kind, h, w, comps, prec, name, rst = c
    return "%s-%dx%dx%d-p%d-%s-r%s" % (kind, w, h, comps, prec, name, rst)


# scripts the reference refuses, with the name of its error (validate_script jcmaster.c:332-347, :390-416, :432-436) and the words
# of its message (jerror.h); num_components = 3
REFUSED = {
    "twice": ([((0,), 1, 0), ((0, 1), 1, 0), ((2,), 1, 0)], "JERR_BAD_SCAN_SCRIPT", "Invalid scan script at entry 2"),
    "order": ([((1, 0), 1, 0), ((2,), 1, 0)], "JERR_BAD_SCAN_SCRIPT", "Invalid scan script at entry 1"),
    "missing": ([((0,), 1, 0), ((1,), 1, 0)], "JERR_MISSING_DATA", "Scan script does not transmit all data"),
    "psv8_in_second": ([((0,), 1, 0), ((1, 2), 8, 0)], "JERR_BAD_PROG_SCRIPT", "Invalid progressive/lossless parameters at scan script entry 2"),
    "pt_eq_precision_in_third": ([((0,), 1, 0), ((1,), 1, 0), ((2,), 1, 8)], "JERR_BAD_PROG_SCRIPT", "Invalid progressive/lossless parameters at scan script entry 3"),
}
