"""The case list and helpers of the progressive stream tests (test_simt_prog_streams.py on the emulator, test_gpu_prog_streams.py on
the chip): VALID progressive files (SOF2) that no libjpeg encoder writes, made from seeds at test time by
jpeg_writer_progressive.write_progressive: EOB runs cut short or not merged at all, a ZRL in front of an EOB, any table shape and table ids, tables
defined once for several scans, 63 correction bits in one block, DC refinement segments of 1-bits only, fourteen levels of
refinement, refinements that regroup their bands, and scan structures, restart intervals and sampling factors of every kind.

Every file is first checked against the reference with no kernel involved (check_premise): the arrays that tests/native/coef_dump
reads from it with oracle/_ref/libjpeg.so.62 are the writer's `expected`, the reference's djpeg and jpegtran -copy none exit 0 and
print nothing, the writer's statistics show the construct the case exists for, and the marker walk (jpeg_info) returns the script.
Then decode_coefficients must return `expected`, decode the pixels of djpeg, and recompress the bytes of jpegtran.  Every comparison
is exact equality.

What differs from a literal reading of the case list this file was written from:
  * zrl_before_eob: a ZRL takes sixteen positions and the decoder reads the next symbol for the same block only if a position of the
    band is left, so the extra ZRL is written where SEVENTEEN positions (in a refinement: sixteen zero-history positions and one
    more of any kind) lie behind the block's last coded coefficient, not sixteen.  The reference reads the file without a message.
  * tables_upfront: a file of three components codes with at most three DC tables; DC ids 1, 2, 3 are coded with and id 0 is defined
    and unused, AC ids 0 - 3 are all coded with.
  * refine_dense: the scripts with bands (1-5 / 6-63, and Ss == Se for 1 - 8) cannot hold 63 correction bits in one scan; their
    premise is the band's length (58 and 55), the 63 bits and the eight stuffed bytes are asserted on the two 1-63 files.
No case is left to the chip alone (GPU_ONLY is empty): eob14_all16, the one large file, takes the emulator under a second a path."""
import functools
import os
import re
import subprocess
import tempfile

import numpy as np

import oracle_lib as O
import coef_cases as CC
import decode_cases as DC
import jpeg_writer as W
import jpeg_writer_progressive as WP
import prog_source_cases as PC
import stream_cases as SC
import transcode_cases as TC

have_tools = PC.have_tools

S420, S444, S2x1 = SC.S420, ((1, 1), (1, 1), (1, 1)), ((2, 1), (1, 1), (1, 1))


# ---- scripts ------------------------------------------------------------------------------------------------------------------------
def scans_of(text, **kw):
    """the scan dictionaries of a -scans text: table id 0 for component 0, 1 for the others; kw goes into every scan"""
    out = []
    for comps, ss, se, ah, al in PC.parse_script(text):
        ids = [0 if ci == 0 else 1 for ci in comps]
        out.append(dict(comps=list(comps), Ss=ss, Se=se, Ah=ah, Al=al, dc=list(ids), ac=list(ids), **kw))
    return out


def script_of(scans):
    return [(tuple(s["comps"]), s["Ss"], s["Se"], s["Ah"], s["Al"]) for s in scans]


def is_ac(s):
    return s["Ss"] > 0


SCRIPT_A = PC.SCRIPT_A
# one interleaved DC scan in two steps, every component's AC in two steps
SCRIPT_I = "0,1,2: 0 0 0 1;\n0: 1 63 0 1;\n1: 1 63 0 1;\n2: 1 63 0 1;\n0,1,2: 0 0 1 0;\n0: 1 63 1 0;\n1: 1 63 1 0;\n2: 1 63 1 0;\n"
# the same with one DC scan per component
SCRIPT_N = ("0: 0 0 0 1;\n1: 0 0 0 1;\n2: 0 0 0 1;\n0: 1 63 0 1;\n1: 1 63 0 1;\n2: 1 63 0 1;\n"
            "0: 0 0 1 0;\n1: 0 0 1 0;\n2: 0 0 1 0;\n0: 1 63 1 0;\n1: 1 63 1 0;\n2: 1 63 1 0;\n")
# spectral selection alone: one level
SCRIPT_1 = "0,1,2: 0 0 0 0;\n0: 1 5 0 0;\n0: 6 63 0 0;\n1: 1 63 0 0;\n2: 1 63 0 0;\n"
SCRIPT_GRAY = "0: 0 0 0 1;\n0: 1 63 0 1;\n0: 0 0 1 0;\n0: 1 63 1 0;\n"
SCRIPT_SPLIT = "".join("%d: 0 0 0 1;\n%d: 1 5 0 1;\n%d: 6 63 0 1;\n" % (c, c, c) for c in range(3)) + \
               "".join("%d: 0 0 1 0;\n%d: 1 5 1 0;\n%d: 6 63 1 0;\n" % (c, c, c) for c in range(3))
SCRIPT_SINGLE = "0: 0 0 0 1;\n" + "".join("0: %d %d 0 1;\n" % (k, k) for k in range(1, 9)) + "0: 9 63 0 1;\n0: 0 0 1 0;\n" + \
                "".join("0: %d %d 1 0;\n" % (k, k) for k in range(1, 9)) + "0: 9 63 1 0;\n"
SCRIPT_DEEP = "0,1,2: 0 0 0 13;\n" + "".join("%d: 1 63 0 13;\n" % c for c in range(3)) + \
              "".join("0,1,2: 0 0 %d %d;\n" % (a + 1, a) + "".join("%d: 1 63 %d %d;\n" % (c, a + 1, a) for c in range(3)) for a in range(12, -1, -1))
SCRIPT_REGROUP = ("0,1,2: 0 0 0 0;\n0: 1 63 0 2;\n1: 1 63 0 1;\n2: 1 63 0 0;\n0: 1 5 2 1;\n0: 6 63 2 1;\n1: 1 63 1 0;\n"
                  "0: 1 2 1 0;\n0: 3 63 1 0;\n")
SCRIPT_COMPSEQ = "".join("%d: 0 0 0 1;\n%d: 1 63 0 1;\n%d: 0 0 1 0;\n%d: 1 63 1 0;\n" % (c, c, c, c) for c in range(3))
SCRIPT_AC = "0: 1 63 0 1;\n1: 1 63 0 1;\n2: 1 63 0 1;\n"
SCRIPT_AC_REF = "0: 1 63 1 0;\n1: 1 63 1 0;\n2: 1 63 1 0;\n"
SCRIPT_01_2 = "0,1: 0 0 0 1;\n2: 0 0 0 1;\n" + SCRIPT_AC + "0,1: 0 0 1 0;\n2: 0 0 1 0;\n" + SCRIPT_AC_REF
SCRIPT_0_12 = "0: 0 0 0 1;\n1,2: 0 0 0 1;\n" + SCRIPT_AC + "0: 0 0 1 0;\n1,2: 0 0 1 0;\n" + SCRIPT_AC_REF
SCRIPT_BANDS = "0,1,2: 0 0 0 0;\n" + "".join("0: %d %d 0 1;\n" % (k, k) for k in range(1, 9)) + "0: 9 63 0 1;\n1: 1 63 0 0;\n2: 1 63 0 0;\n" + \
               "".join("0: %d %d 1 0;\n" % (k, k) for k in range(1, 9)) + "0: 9 63 1 0;\n"
SCRIPT_TAIL = "0,1,2: 0 0 0 0;\n" + "".join("%d: 1 9 0 1;\n%d: 10 63 0 1;\n%d: 1 9 1 0;\n" % (c, c, c) for c in range(3))
SCRIPT_HEAD = "0,1,2: 0 0 0 0;\n" + "".join("%d: 1 2 0 0;\n%d: 3 3 0 1;\n%d: 4 63 0 0;\n" % (c, c, c) for c in range(3))
SCRIPT_EOB14 = "0: 0 0 0 1;\n0: 1 63 0 1;\n0: 0 0 1 0;\n0: 1 63 1 0;\n"
SCRIPT_STUFFED = "0: 0 0 0 0;\n0: 1 63 0 0;\n"


class Case:
    """one generated file and what the tests need to know about it"""
    def __init__(self, data, stats, expected, coefs, width, height, comps, qtables, scans, header):
        self.data, self.stats, self.expected, self.coefs = data, stats, expected, coefs
        self.width, self.height, self.comps, self.qtables, self.scans, self.header = width, height, comps, qtables, scans, header

    @property
    def script(self):
        return script_of(self.scans)

    @property
    def levels(self):
        return PC.levels_of(self.script)

    @property
    def complete(self):
        """the progression is complete in positions 0 - 9 of every component: the reference's djpeg smooths no block"""
        bits = np.full((len(self.comps), 10), -1)
        for s in self.scans:
            for ci in s["comps"]:
                bits[ci, s["Ss"]:min(s["Se"], 9) + 1] = s["Al"]
        return bool((bits == 0).all())

    def arrays(self):
        """`expected` as decode_coefficients and coef_dump give it: the real blocks, natural order, int16"""
        out = []
        for ci in range(len(self.comps)):
            rows, cols = W.real_blocks(self.width, self.height, self.comps, ci)
            e = self.expected[ci][:rows, :cols]
            nat = np.zeros(e.shape, np.int16)
            nat[..., DC.ZIGZAG] = e
            out.append(nat)
        return out


def build(seed, scans, width=45, height=37, comps=None, qtables=None, header="jfif", extras=None, coefs=None, edit=None, density=0.08):
    comps = comps or SC.ycc(*S420)
    if isinstance(scans, str):
        scans = scans_of(scans)
    if qtables is None:
        qtables = {t: SC.quant(seed * 7 + t) for t in sorted(set(c[3] for c in comps))}
    if coefs is None:
        coefs = SC.gen_coefs(seed, width, height, comps, density)
    if edit:
        edit(coefs)
    data, stats, expected = WP.write_progressive(width, height, comps, coefs, qtables, scans, header=header, extras=extras)
    return Case(data, stats, expected, coefs, width, height, comps, qtables, scans, header)


def each(scans, fn):
    """the scans with fn(index, scan) applied to each (it edits the dictionary)"""
    for k, s in enumerate(scans):
        fn(k, s)
    return scans


def ac_only(**kw):
    """an edit for each(): the keywords go into the AC scans"""
    def fn(k, s):
        if is_ac(s):
            s.update(kw)
    return fn


# ---- the families -------------------------------------------------------------------------------------------------------------------
CASES, PREMISES = {}, {}


def ac_stats(c):
    return [st for s, st in zip(c.scans, c.stats["scans"]) if is_ac(s)]


# EOB runs: the same coefficients under the three policies
def _p_eob_none(c):
    for st, mx, sp in zip(ac_stats(c), ac_stats(case("eob_max")), ac_stats(case("eob_split"))):
        assert st["eob"][0] == st["eob_blocks"] and not any(st["eob"][1:]), "an EOBn with n > 0 under the policy none"
        assert st["eob_blocks"] == mx["eob_blocks"] == sp["eob_blocks"]
    assert len({c.data, case("eob_max").data, case("eob_split").data}) == 3


def _p_eob_max(c):
    n = [sum(st["eob"]) for st in ac_stats(c)]
    sp = [sum(st["eob"]) for st in ac_stats(case("eob_split"))]
    no = [sum(st["eob"]) for st in ac_stats(case("eob_none"))]
    assert all(a <= b <= d for a, b, d in zip(n, sp, no)) and sum(n) < sum(sp) < sum(no), (n, sp, no)
    assert all(any(st["eob"][1:]) for st in ac_stats(c)), "an AC scan without a run of two blocks"


def _p_eob_split(c):
    _p_eob_max(case("eob_max"))
    runs = np.sum([st["eob"] for st in ac_stats(c)], axis=0)
    assert runs[0] and runs[1] and runs[2], "runs of 1, 2 - 3 and 4 - 7 blocks: %s" % runs


CASES["eob_none"] = lambda: build(300, each(scans_of(SCRIPT_A), ac_only(eob="none")))
CASES["eob_split"] = lambda: build(300, each(scans_of(SCRIPT_A), ac_only(eob=("split", 5))))
CASES["eob_max"] = lambda: build(300, each(scans_of(SCRIPT_A), ac_only(eob="max")))
PREMISES.update(eob_none=_p_eob_none, eob_split=_p_eob_split, eob_max=_p_eob_max)


def _p_split_restart(c):
    for s, st in zip(c.scans, c.stats["scans"]):
        assert s.get("ri", 0) == (7 if is_ac(s) else 0)
    assert sum(st["eob"][0] for st in ac_stats(c)) and sum(sum(st["eob"][1:]) for st in ac_stats(c))


CASES["eob_split_restart"] = lambda: build(301, each(scans_of(SCRIPT_A), ac_only(eob=("split", 6), ri=7)))
PREMISES["eob_split_restart"] = _p_split_restart


def _p_zrl(c):
    a, b = [st["zrl"] for st in ac_stats(c)], [st["zrl"] for st in ac_stats(case("eob_max"))]
    assert all(x >= y for x, y in zip(a, b)), (a, b)
    first = [x - y for x, y, s in zip(a, b, [s for s in c.scans if is_ac(s)]) if not s["Ah"]]
    ref = [x - y for x, y, s in zip(a, b, [s for s in c.scans if is_ac(s)]) if s["Ah"]]
    assert sum(first) > 0 and sum(ref) > 0, "extra ZRL symbols in first scans %s, in refinements %s" % (first, ref)


CASES["zrl_before_eob"] = lambda: build(300, each(scans_of(SCRIPT_A), ac_only(zrl="before_eob")))
PREMISES["zrl_before_eob"] = _p_zrl


def eob14_coefs():
    a = np.zeros((128, 129, 64), np.int64)
    rng = np.random.default_rng(302)
    for b in ((0, 0), (127, 128)):
        a[b][1:] = rng.integers(-9, 10, 63)
        a[b][0] = 37
    return [a]


def _p_eob14(c):
    assert c.coefs[0].shape[:2] == (128, 129) and c.stats["long_share"] == 1.0
    for s, st in zip(c.scans, c.stats["scans"]):
        if is_ac(s):
            assert st["eob"][14] >= 1, "no EOB14 in the scan %s" % (s,)


CASES["eob14_all16"] = lambda: build(302, scans_of(SCRIPT_EOB14, shape="all16", eob="max"), 1032, 1024, SC.gray(), coefs=eob14_coefs())
PREMISES["eob14_all16"] = _p_eob14


# table shapes and table plumbing
def _p_long(c):
    assert c.stats["long_share"] >= 0.5, "only %.2f of the code words are longer than 8 bits" % c.stats["long_share"]


for _i, _shape in enumerate(("all16", "deep", "all9", "full256")):
    CASES["shape_" + _shape] = (lambda i, shape: lambda: build(310 + i, scans_of(SCRIPT_A, shape=shape)))(_i, _shape)
    if _shape != "full256":
        PREMISES["shape_" + _shape] = _p_long


def dht_segments(data):
    """[(offset of the segment, [Tc * 16 + Th, ...])] of the file's DHT segments"""
    out = []
    for m, pos, n in segments(data):
        if m == 0xC4:
            ids, o = [], pos
            while o < pos + n:
                ids.append(data[o])
                o += 17 + sum(data[o + 1:o + 17])
            out.append((pos, ids))
    return out


def segments(data):
    """[(marker, payload offset, payload length)] of the file's marker segments in order; entropy-coded data is skipped"""
    out, pos = [], 2
    while True:
        assert data[pos] == 0xFF
        while data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        pos += 1
        if m == 0xD9:
            out.append((m, pos, 0))
            return out
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        n = int.from_bytes(data[pos:pos + 2], "big")
        out.append((m, pos + 2, n - 2))
        pos += n
        if m == 0xDA:
            while not (data[pos] == 0xFF and data[pos + 1] != 0 and not 0xD0 <= data[pos + 1] <= 0xD7):
                pos += 1


def first_sos(data):
    return next(pos for m, pos, n in segments(data) if m == 0xDA)


def _upfront_scans():
    dc, ac = {0: 3, 1: 1, 2: 2}, {(0, 1): 0, (0, 6): 3, (1, 1): 1, (2, 1): 2}

    def fn(k, s):
        s["dht"] = "upfront"
        s["dc"] = [dc[ci] for ci in s["comps"]]
        s["ac"] = [ac.get((ci, s["Ss"]), 0) for ci in s["comps"]]
        if k == 0:
            s["also"] = [("dc", 0)]
    return each(scans_of(SCRIPT_A), fn)


def _p_upfront(c):
    d = dht_segments(c.data)
    assert len(d) == 1 and d[0][0] < first_sos(c.data) and sorted(d[0][1]) == [0, 1, 2, 3, 16, 17, 18, 19]
    assert {s["dc"][0] for s in c.scans if not is_ac(s) and not s["Ah"]} == {1, 2, 3} and {s["ac"][0] for s in c.scans if is_ac(s)} == {0, 1, 2, 3}


CASES["tables_upfront"] = lambda: build(320, _upfront_scans())
PREMISES["tables_upfront"] = _p_upfront


def _group_scans():
    def fn(k, s):
        if is_ac(s) and s["comps"] == [0]:
            s["dht"] = ("group", "luma")
    return each(scans_of(SCRIPT_A), fn)


def _p_group(c):
    luma = [(s, st) for s, st in zip(c.scans, c.stats["scans"]) if is_ac(s) and s["comps"] == [0]]
    assert len(luma) == 5 and [st["dht"] for _, st in luma] == [True, False, False, False, False]
    assert any(s["Ah"] for s, _ in luma) and len({repr(st["tables"]) for _, st in luma}) == 1
    # between the first luma AC scan and the last one other scans define tables of their own (ids the group does not use)
    assert sum(st["dht"] for st in c.stats["scans"]) == len(dht_segments(c.data)) >= 8


CASES["tables_group"] = lambda: build(321, _group_scans())
PREMISES["tables_group"] = _p_group


def _many_scans():
    def fn(k, s):
        if k < 2:
            s["dht"] = ("group", "first")
        if k == 0:
            s["also"] = [("ac", 3)]
    return each(scans_of(SCRIPT_I), fn)


def _p_many(c):
    d = dht_segments(c.data)
    assert sorted(d[0][1]) == [0, 1, 16, 19] and d[0][0] < first_sos(c.data)
    assert all(3 not in s["ac"] for s in c.scans) and not c.stats["scans"][1]["dht"]


CASES["dht_many_in_one"] = lambda: build(322, _many_scans())
PREMISES["dht_many_in_one"] = _p_many


def _noise_extras(c):
    t = sorted(c.qtables)[-1]
    dqt = W._seg(0xDB, bytes([c.qtables[t][0] * 16 + t]) + bytes(c.qtables[t][1]))
    return dict(before_scan=[W.COM(b"in front of a scan \xff\xda\xff\xd9"), W.APPN(5, bytes(range(40))), dqt], fill=dict(DHT=2, SOS=1, DRI=3),
                tail=b"\x00trailing bytes\xff\xd8\xff")


def _noise_scans():
    return each(scans_of(SCRIPT_A), lambda k, s: s.update(ri=(0, 4, 0, 9)[k % 4]))


def _noisy():
    clean = case("marker_clean")
    return build(323, _noise_scans(), extras=_noise_extras(clean))


def _p_noise(c):
    clean = case("marker_clean")
    kinds = [m for m, _, _ in segments(c.data)]
    assert kinds.count(0xFE) == kinds.count(0xE5) == len(c.scans) and kinds.count(0xDB) == 2 + len(c.scans) and kinds.count(0xDD) >= 4
    assert b"\xff\xff\xff\xc4" in c.data and b"\xff\xff\xda" in c.data and b"\xff\xff\xff\xff\xdd" in c.data and not c.data.endswith(b"\xff\xd9")
    assert c.data != clean.data and all(np.array_equal(a, b) for a, b in zip(c.expected, clean.expected))


CASES["marker_clean"] = lambda: build(323, _noise_scans())
CASES["marker_noise"] = _noisy
PREMISES["marker_noise"] = _p_noise


# refinement arithmetic: hand-built blocks among generated ones
def dense_blocks(coefs):
    """the blocks (A) - (F) in every component: blocks 3 and 24 (A), 4 (F, directly behind A), 8, 12, 16 and 20 of its raster"""
    rng = np.random.default_rng(330)

    def sign(n):
        return rng.choice([-1, 1], n)
    for a in coefs:
        flat = a.reshape(-1, 64)
        flat[3, 1:] = rng.choice([3, 5, 7, 9, 31], 63) * sign(63)                  # (A) 63 correction bits, all 1
        flat[4, 1:] = 0                                                            # (F) an EOB run starts behind them
        flat[8, 1:] = np.where(np.arange(63) & 1, 3, 2) * sign(63)                 # (B) bits 0 1 0 1 ...
        flat[12, 1:63] = rng.integers(2, 40, 62) * sign(62)                        # (C) a new coefficient at 63 in front of 62 bits
        flat[12, 63] = sign(1)[0]
        flat[16, 1:] = 0                                                           # (D) three ZRL and (14, 1)
        flat[16, 63] = sign(1)[0]
        flat[20, 1:] = 0                                                           # (E) ZRL with correction bits in between
        flat[20, 1:40:2] = rng.integers(2, 8, 20) * sign(20)
        flat[20, 41] = sign(1)[0]
        flat[20, 50] = 6
        flat[24, 1:] = rng.choice([3, 5, 7], 63) * sign(63)                        # (A) once more, at another bit offset


def _p_dense(band, stuffed=None):
    def check(c):
        ref = [st for s, st in zip(c.scans, c.stats["scans"]) if is_ac(s) and s["Ah"]]
        assert max(st["max_correction"] for st in ref) == band
        if stuffed:
            assert all(st["stuffed"] >= stuffed for st in ref if st["max_correction"] == band), [st["stuffed"] for st in ref]
        assert sum(st["zrl"] for st in ref) >= 4
    return check


CASES["refine_dense"] = lambda: build(330, SCRIPT_GRAY, comps=SC.gray(), edit=dense_blocks)
CASES["refine_dense_444"] = lambda: build(331, SCRIPT_N, comps=SC.ycc(*S444), edit=dense_blocks)
CASES["refine_dense_split"] = lambda: build(332, SCRIPT_SPLIT, comps=SC.ycc(*S444), edit=dense_blocks)
CASES["refine_dense_single"] = lambda: build(333, SCRIPT_SINGLE, comps=SC.gray(), edit=dense_blocks)
PREMISES.update(refine_dense=_p_dense(63, 8), refine_dense_444=_p_dense(63, 8), refine_dense_split=_p_dense(58), refine_dense_single=_p_dense(55))


def odd_dc(coefs):
    for a in coefs:
        a[..., 0] |= 1


def _p_all_ones(c):
    import mozjpeg_amd as M
    info = M.jpeg_info(c.data, progressive_sources=True)
    n = 0
    for s in info.prog_scans:
        if s.Ss == 0 and s.Ah:
            ent = c.data[s.data_offset:s.data_offset + s.data_size]
            assert re.fullmatch(rb"(?:\xff\x00|\xff[\xd0-\xd7])+", ent), "a DC refinement segment that is not FF 00 pairs: %s" % ent[:24].hex()
            n += 1
    assert n >= 1


for _n, _args in {"420_ri0": (SCRIPT_I, 0, {}), "420_ri3": (SCRIPT_I, 3, {}),
                  "17x9_2x1_ri0": (SCRIPT_N, 0, dict(width=17, height=9, comps=SC.ycc(*S2x1))),
                  "17x9_2x1_ri3": (SCRIPT_N, 3, dict(width=17, height=9, comps=SC.ycc(*S2x1)))}.items():
    CASES["dc_refine_all_ones_" + _n] = (lambda a: lambda: build(340, each(scans_of(a[0]), lambda k, s: s.update(ri=0 if is_ac(s) else a[1])), edit=odd_dc, **a[2]))(_args)
    PREMISES["dc_refine_all_ones_" + _n] = _p_all_ones


def every_magnitude(coefs):
    """magnitudes of every bit length up to ten in every component, so that each level of refinement finds new coefficients"""
    for a in coefs:
        flat = a.reshape(-1, 64)
        for j in range(10):
            flat[1, 1 + 3 * j] = (1 << j) + (j > 1)
            flat[2, 2 + 3 * j] = -((1 << (j + 1)) - 1)


def _p_deep(c):
    assert len(c.scans) == 56 and c.levels == 14
    for s, st in zip(c.scans, c.stats["scans"]):
        if is_ac(s) and not s["Ah"]:
            assert st["zrl"] == 0 and st["codes"] == sum(st["eob"]), "an AC first scan at Al = 13 that is not EOB runs alone"
    new = [st["codes"] - sum(st["eob"]) - st["zrl"] for s, st in zip(c.scans, c.stats["scans"]) if is_ac(s) and s["Ah"] and s["comps"] == [0] and s["Al"] < 10]
    assert all(new), "a level without a newly non-zero coefficient: %s" % new


CASES["deep_al"] = lambda: build(350, SCRIPT_DEEP, edit=every_magnitude)
PREMISES["deep_al"] = _p_deep
CASES["refine_regroup"] = lambda: build(351, SCRIPT_REGROUP)

# scan structure and geometry
CASES["component_sequential"] = lambda: build(360, SCRIPT_COMPSEQ)
CASES["dc_pairs_01_2"] = lambda: build(361, SCRIPT_01_2)
CASES["dc_pairs_0_12"] = lambda: build(362, SCRIPT_0_12)
CASES["bands_single"] = lambda: build(363, SCRIPT_BANDS)


def _p_dri_once(c):
    kinds = [m for m, _, _ in segments(c.data)]
    assert kinds.count(0xDD) == 1 and kinds.index(0xDD) < kinds.index(0xDA) and all(s["ri"] == 5 for s in c.scans)


CASES["dri_once"] = lambda: build(364, scans_of(SCRIPT_A, ri=5))
PREMISES["dri_once"] = _p_dri_once
RI_MIXED = [0, 7, 1000, 4, 11, 0, 5, 2, 0, 3, 1, 7, 1000, 0, 5, 0, 1000, 1]


def _p_ri_mixed(c):
    assert c.scans[10]["Ah"] and is_ac(c.scans[10]) and c.scans[10]["ri"] == 1          # luma 1 - 5 refined: one block per segment
    assert is_ac(c.scans[11]) and c.scans[11]["Ah"] and 30 % c.scans[11]["ri"]          # luma 6 - 63 refined: 30 blocks in intervals of 7
    assert c.scans[16]["ri"] >= 12 and c.scans[13]["ri"] == 0 and c.scans[13]["Ah"]


CASES["ri_mixed"] = lambda: build(365, each(scans_of(SCRIPT_A), lambda k, s: s.update(ri=RI_MIXED[k])))
PREMISES["ri_mixed"] = _p_ri_mixed
SAMPLINGS = ("4x1_1x1_2x1", "1x1_2x2_2x2", "3x2_1x1_1x2", "1x2_2x1_2x2")
for _i, _n in enumerate(SAMPLINGS):
    CASES["samp_" + _n] = (lambda i, n: lambda: build(370 + i, SCRIPT_I, comps=SC.ycc(*SC.SAMPLINGS[n])))(_i, _n)
for _i, (_w, _h) in enumerate(((1, 1), (8, 8), (9, 17))):
    for _sn, _s in (("420", S420), ("2x1", S2x1)):
        CASES["size_%dx%d_%s" % (_w, _h, _sn)] = (lambda i, w, h, s: lambda: build(
            380 + i, each(scans_of(SCRIPT_I), ac_only(eob=("split", 7))), width=w, height=h, comps=SC.ycc(*s), density=0.15))(_i, _w, _h, _s)


def _p_qt16(c):
    assert SC.dqt_precisions(c.data) == {0: 1, 1: 1} and max(c.qtables[1][1]) > 255


CASES["qt16"] = lambda: build(390, SCRIPT_A, qtables={0: SC.quant(3900, 1, 1000, 1), 1: SC.quant(3901, 200, 3000, 1)})
PREMISES["qt16"] = _p_qt16


def _p_rgb(c):
    import mozjpeg_amd as M
    i = M.jpeg_info(c.data, progressive_sources=True)
    assert i.jpeg_color_space == M.CS_RGB and not i.saw_JFIF_marker and not i.saw_Adobe_marker


CASES["rgb_ids"] = lambda: build(391, SCRIPT_N, comps=SC.ycc(*S444, ids=(82, 71, 66), tq=(0, 0, 0)), header=None)
PREMISES["rgb_ids"] = _p_rgb


def _p_tail(c):
    got, sent = c.arrays(), Case(c.data, c.stats, c.coefs, c.coefs, c.width, c.height, c.comps, c.qtables, c.scans, c.header).arrays()
    z = DC.ZIGZAG
    assert c.complete and any((e[..., z[10:]] != a[..., z[10:]]).any() for e, a in zip(got, sent)), "nothing was lost in 10 - 63"
    assert all(np.array_equal(e[..., z[:10]], a[..., z[:10]]) for e, a in zip(got, sent))


def _p_head(c):
    assert not c.complete and any((e[..., 3] != a[..., 3]).any() for e, a in zip(c.expected, c.coefs))


CASES["unrefined_tail"] = lambda: build(392, SCRIPT_TAIL)
CASES["unrefined_head"] = lambda: build(393, SCRIPT_HEAD)
PREMISES.update(unrefined_tail=_p_tail, unrefined_head=_p_head)


# subsequences: every code 16 bits long; and blocks of exactly 128 bits that end on 0xFF, as stream_cases.stuffed_boundaries builds them
# for a sequential scan -- here an AC first scan (11 coefficients in runs of 4 and a 255 at position 63, 9-bit code words: ten of size 1,
# one of size 2; block 0 holds a size-10 value in its place and is 17 data bytes long), so byte 17 i of the scan is a stuffed zero
def stuffed_coefs(size=96, seed=395):
    rows, cols = W.padded_blocks(size, size, SC.gray(), 0)
    rng = np.random.default_rng(seed)
    a = np.zeros((rows * cols, 64), np.int64)
    a[:, 0] = rng.integers(-20, 21, rows * cols)
    pos = np.arange(5, 56, 5)
    for b in range(rows * cols):
        mag = np.ones(11, np.int64)
        mag[rng.integers(0, 11)] = 600 if b == 0 else rng.integers(2, 4)
        a[b, pos] = mag * rng.choice([-1, 1], 11)
    a[:, 63] = 255
    return [a.reshape(rows, cols, 64)]


def _p_stuffed(c):
    import mozjpeg_amd as M
    s = M.jpeg_info(c.data, progressive_sources=True).prog_scans[1]
    ent = c.data[s.data_offset:s.data_offset + s.data_size]
    nsub = -(-len(ent) // SC.STUFFED_S)
    assert nsub > 100 and all(ent[k * SC.STUFFED_S - 1] == 0xFF and ent[k * SC.STUFFED_S] == 0 for k in range(1, nsub)), "a boundary that is no stuffed zero"


CASES["subseq_all16"] = lambda: build(394, scans_of(SCRIPT_A, shape="all16"))
CASES["stuffed_boundaries_prog"] = lambda: build(395, scans_of(SCRIPT_STUFFED, shape="all9"), 96, 96, SC.gray(), coefs=stuffed_coefs())
PREMISES.update(subseq_all16=_p_long, stuffed_boundaries_prog=_p_stuffed)
SUBSEQ_CASES = {"subseq_all16": (16, None), "stuffed_boundaries_prog": (16, SC.STUFFED_S, None)}

# cases that would take the emulator more than about 10 s run on the chip only: none -- the one large case, eob14_all16 with its
# 16 512 blocks, takes it under a second per path
GPU_ONLY = []
NAMES = list(CASES)
SCALED = ("refine_dense", "deep_al")                     # scale_1_2 as well
RECOMPRESS = ("eob_split", "eob14_all16", "shape_all16", "refine_dense", "deep_al", "tables_group", "component_sequential", "samp_3x2_1x1_1x2", "unrefined_head")
RECOMPRESS_SWITCHES = ("default", "revert_opt")
PIXEL_MODES = ("default", "dct_fast")


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


# ---- the reference's programs, with what they print ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_run(tool, args, data):
    """(exit status, what it printed, the output file) of oracle/_ref/<tool> <args> on the file"""
    with tempfile.TemporaryDirectory() as td:
        inp, outp = os.path.join(td, "in.jpg"), os.path.join(td, "out")
        with open(inp, "wb") as f:
            f.write(data)
        r = subprocess.run([os.path.join(O.REF_DIR, tool)] + list(args) + ["-outfile", outp, inp], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        out = open(outp, "rb").read() if os.path.exists(outp) else None
        return r.returncode, (r.stdout + r.stderr).decode(errors="replace"), out


def ref_pixels(data, args=()):
    rc, text, out = ref_run("djpeg", ("-pnm",) + tuple(args), data)
    assert rc == 0 and text == "" and out, "the reference's djpeg: %d %s" % (rc, text)
    return DC.parse_pnm(out)


def ref_recoded(data, args=()):
    rc, text, out = ref_run("jpegtran", ("-copy", "none") + tuple(args), data)
    assert rc == 0 and text == "" and out, "the reference's jpegtran: %d %s" % (rc, text)
    return out


# ---- 1. the premise: the writer against the reference, no kernel involved --------------------------------------------------------------
def check_premise(M, name):
    c = case(name)
    ref = PC.ref_coefs(c.data)
    want = c.arrays()
    assert CC.same_arrays(want, ref), "the writer's expected arrays are not what the reference reads: components %s" % [
        k for k in range(len(ref)) if want[k].shape != ref[k].shape or not np.array_equal(want[k], ref[k])]
    ref_pixels(c.data)
    ref_recoded(c.data)
    info = M.jpeg_info(c.data, progressive_sources=True)
    assert info.sof_type == 2 and info.num_scans == 0 and (info.image_width, info.image_height) == (c.width, c.height)
    got = [(tuple(s.component_index[:s.comps_in_scan]), s.Ss, s.Se, s.Ah, s.Al) for s in info.prog_scans]
    assert got == c.script
    for s, sc, st in zip(c.scans, info.prog_scans, c.stats["scans"]):
        n = len(s["comps"])
        assert sc.restart_interval == s.get("ri", 0)
        assert [sc.dc_tbl_no[j] for j in range(n)] == list(s["dc"][:n]) and [sc.ac_tbl_no[j] for j in range(n)] == list(s["ac"][:n])
        for (cls, t), (bits, vals) in st["tables"].items():                 # the tables in force at this SOS are the ones the scan was coded with
            slot = 2 * t + (cls == "ac")
            assert list(sc.huff_bits[slot])[1:] == bits[1:] and list(sc.huff_vals[slot])[:len(vals)] == vals
    for t, (_, q) in c.qtables.items():
        assert [info.quantval[t][DC.ZIGZAG[k]] for k in range(64)] == list(q)
    if name in PREMISES:
        PREMISES[name](c)


# ---- 2. - 4. the three paths -----------------------------------------------------------------------------------------------------------
def _raise(x):
    if isinstance(x, Exception):
        raise x
    return x


def check_coefficients(M, name):
    """decode_coefficients gives `expected`; an encoder of its own reports the script's levels"""
    c = case(name)
    assert CC.same_arrays(_raise(M.decode_coefficients([c.data], progressive_sources=True)[0]), c.arrays())
    enc = M.Encoder(M.params_from_jpeg(c.data, revert=True, progressive_sources=True), max_batch=1)
    enc.set_sources(progressive=True)
    try:
        assert CC.same_arrays(enc.decode_host([c.data], coefficients=True)[0], c.arrays())
        assert enc.prog_stats()["levels"] == c.levels, "%d levels, the script has %d" % (enc.prog_stats()["levels"], c.levels)
    finally:
        enc.close()


def pixel_modes(name):
    return PIXEL_MODES + (("scale_1_2",) if name in SCALED else ())


def check_pixels(M, name):
    """the pixels of djpeg in every mode of the case; where the reference would smooth blocks, the refusal that says so"""
    c = case(name)
    for mode in pixel_modes(name):
        kw, args = PC.PIXEL_MODES[mode]
        out = M.decode([c.data], progressive_sources=True, **kw)[0]
        if not c.complete:
            for out in (out, M.decode_planes([c.data], progressive_sources=True)[0]):
                assert isinstance(out, M.MjhError) and out.code == M.EUNSUPPORTED and "block smoothing" in str(out), out
            continue
        assert SC.same(_raise(out), ref_pixels(c.data, args)), mode


def check_recompress(M, name, sw):
    c = case(name)
    kw, args = TC.SWITCHES[sw]
    assert _raise(M.recompress([c.data], progressive_sources=True, **kw)[0]) == ref_recoded(c.data, args)


def check_same_decode(M, a, b):
    """two files that differ decode to the same arrays and pixels"""
    a, b = case(a), case(b)
    assert a.data != b.data
    x, y = M.decode_coefficients([a.data, b.data], progressive_sources=True, max_batch=1)
    assert CC.same_arrays(_raise(x), _raise(y))
    x, y = M.decode([a.data, b.data], progressive_sources=True, max_batch=1)
    assert SC.same(_raise(x), _raise(y))


# ---- 5. subsequences and batching ------------------------------------------------------------------------------------------------------
def check_subseq(M, name, setenv):
    """coefficients, pixels and the re-coded file under every subsequence length of the case; at 16 bytes the scans take three rounds
    of synchronisation and more"""
    c = case(name)
    results = []
    for S in SUBSEQ_CASES[name]:
        setenv(S)
        enc = M.Encoder(M.params_from_jpeg(c.data, revert=True, optimize=True, progressive_sources=True), max_batch=1)
        enc.set_sources(progressive=True)
        try:
            co = enc.decode_host([c.data], coefficients=True)[0]
            st = enc.transcode_stats()
            pix = enc.decode_host([c.data])[0]
            rec = enc.transcode_host([c.data])[0]
        finally:
            enc.close()
        if S:
            assert st["subseq"] == S
        if S == 16:
            assert st["rounds"] >= 3, st
        assert CC.same_arrays(co, c.arrays()), S
        results.append((pix, rec))
    assert all(SC.same(p, results[0][0]) and r == results[0][1] for p, r in results)
    assert SC.same(results[0][0], ref_pixels(c.data)) and results[0][1] == ref_recoded(c.data, ["-revert", "-optimize"])


BATCH_Q = {0: SC.quant(4000), 1: SC.quant(4001)}


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """sixteen files of one signature: scripts of 1, 2, 3 and 14 levels, every table shape, the three EOB policies, restart intervals,
    and four sequential files of write_jpeg.  Returns [(bytes, expected arrays, levels)]"""
    scripts = (SCRIPT_1, SCRIPT_I, SCRIPT_A, SCRIPT_DEEP, SCRIPT_N, SCRIPT_REGROUP, SCRIPT_COMPSEQ, SCRIPT_BANDS, SCRIPT_01_2, SCRIPT_0_12, SCRIPT_SPLIT, SCRIPT_A)
    out = []
    for k in range(16):
        if k % 4 == 1:
            scans = SC.one_scan(3, W.SHAPES[k % len(W.SHAPES)], ri=k % 5)
            c = SC.build(400 + k, 45, 37, SC.ycc(*S420), scans=scans, qtables=BATCH_Q)
            exp = Case(c.data, c.stats, c.coefs, c.coefs, 45, 37, c.comps, BATCH_Q, [], "jfif").arrays()
            out.append((c.data, exp, 0))
            continue
        text = scripts[k - (k + 2) // 4]
        policy = ("max", "none", ("split", k))[k % 3]
        scans = each(scans_of(text, shape=W.SHAPES[k % len(W.SHAPES)]), lambda i, s: s.update(ri=(k + i) % 4 * (k % 3), **(dict(eob=policy) if is_ac(s) else {})))
        c = build(400 + k, scans, qtables=BATCH_Q, edit=every_magnitude if text is SCRIPT_DEEP else None)
        assert c.complete
        out.append((c.data, c.arrays(), c.levels))
    return out


def check_mixed_batch(M):
    batch = mixed_batch()
    files = [f for f, _, _ in batch]
    assert sorted(set(lv for _, _, lv in batch)) == [0, 1, 2, 3, 14] and sum(lv == 0 for _, _, lv in batch) == 4
    assert len(set(M._signature(M.jpeg_info(f, progressive_sources=True)) for f in files)) == 1
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True, optimize=True, progressive_sources=True), max_batch=16)
    enc.set_sources(progressive=True)
    try:
        co = enc.decode_host(files, coefficients=True)
        assert enc.prog_stats()["levels"] == 14
        for i, (f, exp, _) in enumerate(batch):
            assert CC.same_arrays(co[i], exp), i
        pix = enc.decode_host(files)
        for i, f in enumerate(files):
            assert SC.same(pix[i], ref_pixels(f)), i
        rec = enc.transcode_host(files)
        for i, f in enumerate(files):
            assert rec[i] == ref_recoded(f, ["-revert", "-optimize"]), i
        seq = [i for i, (_, _, lv) in enumerate(batch) if lv == 0]
        co = enc.decode_host([files[i] for i in seq], coefficients=True)
        assert enc.prog_stats()["levels"] == 0
        for k, i in enumerate(seq):
            assert CC.same_arrays(co[k], batch[i][1]), i
    finally:
        enc.close()
