"""Writes tests/golden/goldens_lossless.json: MD5 + size of the reference's lossless file (`oracle/_ref/cjpeg -revert -lossless`) for
every case of lossless_cases.SIMT_CASES.  Needs the reference binaries oracle/Makefile builds; re-running it must not change an entry."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lossless_cases as LC  # noqa: E402


def main():
    out = {}
    for c in LC.SIMT_CASES:
        kind, h, w, comps, prec, psv, pt, rst = c
        f = LC.reference(LC.image(kind, h, w, comps, prec), psv, pt, prec, rst)
        assert isinstance(f, bytes), f
        out[LC.case_id(c)] = {"md5": hashlib.md5(f).hexdigest(), "size": len(f)}
    with open(os.path.join(HERE, "goldens_lossless.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(len(out), "entries")


if __name__ == "__main__":
    main()
