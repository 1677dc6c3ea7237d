"""The case list and helpers of the stream tests (test_simt_streams.py on the emulator, test_gpu_streams.py on the chip): VALID
sequential JPEG files that no libjpeg encoder writes, made from seeds at test time by tests/jpeg_writer.py.

Every expected byte comes from the reference's jpegtran (oracle/_ref/jpegtran -copy none + switches) and every expected pixel from
its djpeg (oracle/_ref/djpeg -pnm + switches), both run at test time; equality is exact.  Every case also asserts, on its bytes or
through mozjpeg_amd.jpeg_info, that the property it exists for is present (check_premise)."""
import functools

import numpy as np

import decode_cases as DC
import jpeg_writer as W
import transcode_cases as TC
import transform_cases as XC

have_tools = DC.have_tools

CODINGS = ("revert", "revert_opt", "fastcrush_progressive")
# the transform subset: keywords of mozjpeg_amd.transform_spec; the last one is refused by the reference and by us ("not perfect")
TRANSFORMS = (dict(transform="rot90"), dict(transform="rot90", trim=True), dict(transform="flip_h", trim=True),
              dict(transform="transverse"), dict(crop="24x16+9+10"))
REFUSED_TRANSFORM = dict(transform="flip_h", perfect=True)
LONG_SHAPES = ("all16", "deep", "all9")


# ---- seeded content ---------------------------------------------------------------------------------------------------------------
def ycc(*samp, ids=(1, 2, 3), tq=(0, 1, 1)):
    return [(ids[c], samp[c][0], samp[c][1], tq[c]) for c in range(3)]


def gray(h=1, v=1):
    return [(1, h, v, 0)]


S420 = ((2, 2), (1, 1), (1, 1))


def quant(seed, lo=1, hi=64, prec=0):
    return prec, [int(v) for v in np.random.default_rng(seed).integers(lo, hi + 1, 64)]


def gen_coefs(seed, width, height, comps, density=0.08, edges=True):
    """per component [block rows][block cols][64 zig-zag], padded to whole MCUs (the padding blocks hold content as well: an interleaved
    scan codes them and their DC values take part in the prediction).  Sparse random AC data; with `edges`, every block whose
    number is 0..6 modulo 8 is one of: all-zero AC / a lone coefficient at 63 (no EOB, three ZRL) / runs of 16..47 zeros (one or
    two ZRL) / dense to 63 / the amplitudes +-1023, +-512, 511 / DC 1023 / DC -1024 (neighbours: differences of +-2047)."""
    rng = np.random.default_rng(seed)
    out = []
    for ci in range(len(comps)):
        rows, cols = W.padded_blocks(width, height, comps, ci)
        a = np.zeros((rows * cols, 64), np.int64)
        mask = rng.random((rows * cols, 63)) < density
        mag = rng.integers(1, 41, (rows * cols, 63)) * rng.choice([-1, 1], (rows * cols, 63))
        a[:, 1:] = np.where(mask, mag, 0)
        a[:, 0] = rng.integers(-300, 301, rows * cols)
        if edges:
            for b in range(rows * cols):
                kind = (b + ci) % 8
                if kind == 7:
                    continue
                if kind < 5:
                    a[b, 1:] = 0
                if kind == 1:
                    a[b, 63] = int(rng.integers(1, 30)) * (1 if b & 8 else -1)
                elif kind == 2:
                    k = 0
                    while True:
                        k += int(rng.integers(16, 48)) + 1
                        if k > 63:
                            break
                        a[b, k] = int(rng.integers(1, 200)) * (1 if rng.random() < 0.5 else -1)
                elif kind == 3:
                    a[b, 1:] = rng.integers(1, 9, 63) * rng.choice([-1, 1], 63)
                elif kind == 4:
                    pos = rng.choice(np.arange(1, 64), 5, replace=False)
                    a[b, pos] = [1023, -1023, 512, -512, 511]
                else:
                    a[b, 0] = 1023 if kind == 5 else -1024
        out.append(a.reshape(rows, cols, 64))
    return out


class Case:
    """one generated file and what the tests need to know about it"""
    def __init__(self, data, stats, coefs, width, height, comps, qtables, scans, sof, header, **kw):
        self.data, self.stats, self.coefs = data, stats, coefs
        self.width, self.height, self.comps, self.qtables, self.scans, self.sof, self.header = width, height, comps, qtables, scans, sof, header
        self.status = kw.get("status", 0)                  # the reference's exit status: 2 for the Adobe-transform-2 file alone
        self.codings = kw.get("codings", CODINGS)
        self.modes = kw.get("modes", tuple(DC.MODES))
        self.transforms = kw.get("transforms", TRANSFORMS)
        self.edges = kw.get("edges", True)
        self.long_codes = kw.get("long_codes", False)


def one_scan(nc, shape="optimal", ri=0, dc=None, ac=None):
    ids = [0, 1, 1][:nc]
    return [dict(comps=list(range(nc)), dc=list(dc or ids), ac=list(ac or ids), ri=ri, shape=shape)]


def build(seed, width, height, comps, scans=None, qtables=None, sof=0, header="jfif", density=0.08, edges=True, extras=None, coefs=None, **kw):
    if scans is None:
        scans = one_scan(len(comps))
    if qtables is None:
        qtables = {t: quant(seed * 7 + t) for t in sorted(set(c[3] for c in comps))}
    if coefs is None:
        coefs = gen_coefs(seed, width, height, comps, density, edges)
    data, stats = W.write_jpeg(width, height, comps, coefs, qtables, scans, sof=sof, header=header, extras=extras)
    shapes = [s.get("shape", "optimal") for s in scans]
    kw.setdefault("long_codes", all(isinstance(s, str) and s in LONG_SHAPES for s in shapes))
    return Case(data, stats, coefs, width, height, comps, qtables, scans, sof, header, edges=edges, **kw)


# ---- the families -------------------------------------------------------------------------------------------------------------------
CASES = {}


def case_(name):
    def reg(f):
        CASES[name] = f
        return f
    return reg


META = {}      # name -> what the case runs through, known without building it


def _simple(name, seed, comps, w=45, h=37, **kw):
    META[name] = dict(codings=kw.get("codings", CODINGS), transforms=kw.get("transforms", TRANSFORMS))
    CASES[name] = lambda: build(seed, w, h, comps, **kw)


# table shapes on 4:2:0; one pair shared by the three components (canon[] collapses every block position onto 0)
for _i, _shape in enumerate(W.SHAPES):
    _simple("shape_" + _shape, 100 + _i, ycc(*S420), w=61, h=43, scans=one_scan(3, _shape))
_simple("shape_shared_pair", 110, ycc(*S420), w=61, h=43, scans=one_scan(3, "optimal", dc=[0, 0, 0], ac=[0, 0, 0]))
_simple("shape_shared_pair_all16", 111, ycc(*S420), w=61, h=43, scans=one_scan(3, "all16", dc=[1, 1, 1], ac=[1, 1, 1]))
# table ids 2 and 3 (SOF1), swapped between luma and chroma, DC and AC of a component on different ids
_simple("ids_2_3", 120, ycc(*S420), sof=1, scans=one_scan(3, dc=[2, 3, 3], ac=[2, 3, 3]))
_simple("ids_3_2", 121, ycc(*S420), sof=1, scans=one_scan(3, "deep", dc=[3, 2, 2], ac=[3, 2, 2]))
_simple("ids_dc_ac_differ", 122, ycc(*S420), sof=1, scans=one_scan(3, dc=[2, 3, 0], ac=[3, 2, 1]))
_simple("ids_1_0", 123, ycc(*S420), scans=one_scan(3, dc=[1, 0, 0], ac=[0, 1, 1]))
# scan layouts: the same table id redefined in front of every scan (in another shape), restart intervals that differ, 0 behind
# non-zero, one interval beyond the scan's MCU count
_simple("scans_0_12", 130, ycc(*S420), scans=[dict(comps=[0], dc=[0], ac=[0], ri=3, shape="optimal"),
                                              dict(comps=[1, 2], dc=[0, 0], ac=[0, 0], ri=0, shape="all9")])
_simple("scans_2_0_1", 131, ycc(*S420), scans=[dict(comps=[2], dc=[0], ac=[0], ri=1000, shape="deep"),
                                               dict(comps=[0], dc=[0], ac=[0], ri=2, shape="optimal"),
                                               dict(comps=[1], dc=[0], ac=[0], ri=0, shape="all16")])
_simple("scans_1_02", 132, ycc(*S420), scans=[dict(comps=[1], dc=[1], ac=[1], ri=5, shape="all16"),
                                              dict(comps=[0, 2], dc=[1, 0], ac=[1, 0], ri=2, shape="optimal")])
# quantization: 16-bit precision with values above 255 / of 255 and below / one entry of 32768 and more (decode only)
_simple("q16_above_255", 140, ycc(*S420), sof=1, qtables={0: quant(1400, 1, 1000, 1), 1: quant(1401, 200, 3000, 1)})
_simple("q16_up_to_255", 141, ycc(*S420), qtables={0: quant(1410, 1, 255, 1), 1: quant(1411, 1, 99, 0)})
_simple("q16_entry_40000", 142, ycc(*S420), sof=1, qtables={0: (1, [40000 if k == 5 else v for k, v in enumerate(quant(1420, 1, 300)[1])]), 1: quant(1421, 1, 64)},
        codings=(), transforms=())
# colour-space detection (default_decompress_parms)
_simple("cs_none_1_2_3", 150, ycc((1, 1), (1, 1), (1, 1)), header=None)
_simple("cs_none_R_G_B", 151, ycc((1, 1), (1, 1), (1, 1), ids=(82, 71, 66), tq=(0, 0, 0)), header=None)
_simple("cs_none_0_7_200", 152, ycc(*S420, ids=(0, 7, 200)), header=None)
_simple("cs_adobe_0", 153, ycc((1, 1), (1, 1), (1, 1), tq=(0, 0, 0)), header=("adobe", 0))
_simple("cs_adobe_1", 154, ycc(*S420), header=("adobe", 1))
_simple("cs_adobe_2", 155, ycc(*S420), header=("adobe", 2), status=2)
# sampling factors
SAMPLINGS = {
    "4x1_1x1_2x1": ((4, 1), (1, 1), (2, 1)), "3x1_1x1_1x1": ((3, 1), (1, 1), (1, 1)), "1x1_2x2_2x2": ((1, 1), (2, 2), (2, 2)),
    "4x2_1x1_1x1": ((4, 2), (1, 1), (1, 1)), "1x2_2x1_2x2": ((1, 2), (2, 1), (2, 2)), "2x2_2x1_1x2": ((2, 2), (2, 1), (1, 2)),
    "3x2_1x1_1x2": ((3, 2), (1, 1), (1, 2)),
}
for _i, (_n, _s) in enumerate(SAMPLINGS.items()):
    _simple("samp_" + _n, 160 + _i, ycc(*_s))
_simple("samp_gray_1x1", 170, gray(1, 1))
_simple("samp_gray_2x2", 171, gray(2, 2))      # jpegtran forces 1x1 into the frame header it writes (jtransform_adjust_parameters)
_simple("samp_gray_3x4", 172, gray(3, 4))
GRAY_FORCED = ("samp_gray_2x2", "samp_gray_3x4")

FRACTIONAL = "fractional_2x1_3x1_1x1"          # not in CASES: a pinned refusal (check_fractional_refusal)


@functools.lru_cache(maxsize=None)
def fractional_case():
    return build(180, 45, 37, ycc((2, 1), (3, 1), (1, 1)))


# marker noise in a two-scan file: TEM, COM, APP5, fill bytes in front of DHT / SOS / EOI, bytes behind EOI
NOISE_SCANS = [dict(comps=[0], dc=[0], ac=[0], ri=4, shape="optimal"), dict(comps=[1, 2], dc=[1, 1], ac=[1, 1], ri=0, shape="deep")]
NOISE_EXTRAS = dict(after_soi=[W.TEM, W.COM(b"a comment \xff\xd9 with marker bytes"), W.APPN(5, bytes(range(40)))],
                    before_scan=[W.COM(b"in front of a scan"), W.TEM], fill=dict(DHT=2, SOS=1, EOI=3, DRI=1), tail=b"\x00trailing bytes\xff\xd8\xff")
_simple("noise_clean", 190, ycc(*S420), scans=NOISE_SCANS)
_simple("noise_markers", 190, ycc(*S420), scans=NOISE_SCANS, extras=NOISE_EXTRAS)


# out-of-range amplitudes: legal Huffman syntax, beyond what an 8-bit encoder produces
def _oor(seed, ac=None, dc=None):
    def make():
        comps = ycc(*S420)
        coefs = gen_coefs(seed, 45, 37, comps, edges=False)
        q = oor_qtables(dc is not None)
        if ac is not None:
            coefs[0][1, 2, 9] = ac
            coefs[2][0, 1, 63] = ac
        if dc is not None:
            coefs[0][..., 0] = 0
            coefs[0][1, 1, 0] = dc
            coefs[0][2, 3, 0] = -dc
        return build(seed, 45, 37, comps, coefs=coefs, qtables=q, codings=(), transforms=(), edges=False)
    return make


def oor_qtables(unit):
    return {0: (0, [1] * 64), 1: (0, [1] * 64)} if unit else {0: quant(1400), 1: quant(1401)}


OUT_OF_RANGE = {"oor_ac_1024": _oor(200, ac=1024), "oor_ac_m20000": _oor(201, ac=-20000), "oor_ac_32767": _oor(202, ac=32767),
                "oor_dc_6000": _oor(203, dc=6000)}


@functools.lru_cache(maxsize=None)
def oor_case(name):
    return OUT_OF_RANGE[name]()


@functools.lru_cache(maxsize=None)
def oor_neighbour(k, unit):
    """a file of the out-of-range files' signature with ordinary amplitudes, in another table shape"""
    return build(210 + k, 45, 37, ycc(*S420), qtables=oor_qtables(unit), scans=one_scan(3, ("optimal", "deep")[k & 1]))


# slow synchronisation: near-fixed-length code words (blocks of 127 / 129 bits): no lane ever lands on a code boundary by chance
def slow_sync(size, seed=220):
    comps = gray()
    rows, cols = W.padded_blocks(size, size, comps, 0)
    rng = np.random.default_rng(seed)
    a = np.zeros((rows * cols, 64), np.int64)
    a[:, 1:] = rng.choice([-1, 1], (rows * cols, 63))
    # DC categories 0 and 1: differences of 0 (three times out of four) and +-1
    step = rng.choice([0, 0, 0, 1], rows * cols) * np.where(np.arange(rows * cols) & 1, 1, -1)
    a[:, 0] = np.cumsum(step)
    return build(seed, size, size, comps, coefs=[a.reshape(rows, cols, 64)], edges=False, transforms=())


CASES["slow_sync_96"] = lambda: slow_sync(96)

# every subsequence boundary ON a stuffed zero: gray blocks of exactly 128 bits whose last byte is 0xFF (the value bits of a 255 at
# position 63), 9-bit code words throughout, so with MJH_DECODE_SUBSEQ = 17 byte i * 17 is the 0x00 behind a block's last byte and
# block i starts right behind it.  A lane that starts behind the zero guesses its state exactly; one that starts ON it never does.
STUFFED_S = 17


def stuffed_boundaries(size=96, seed=225):
    comps = gray()
    rows, cols = W.padded_blocks(size, size, comps, 0)
    rng = np.random.default_rng(seed)
    a = np.zeros((rows * cols, 64), np.int64)
    a[:, 0] = 200                                          # block 0: an 8-bit DC difference (17 data bytes), then differences of 0
    pos = np.arange(6, 61, 6)                              # ten coefficients, runs of 5: eight of size 1 and two of size 2
    for b in range(rows * cols):
        mag = np.ones(10, np.int64)
        mag[rng.choice(10, 2, replace=False)] = rng.integers(2, 4, 2)
        a[b, pos] = mag * rng.choice([-1, 1], 10)
    a[:, 63] = 255
    return build(seed, size, size, comps, coefs=[a.reshape(rows, cols, 64)], scans=one_scan(1, "all9"), edges=False, transforms=())


def check_stuffed_boundaries(M, c, setenv):
    i = M.jpeg_info(c.data)
    ent = c.data[i.scans[0].data_offset:i.scans[0].data_offset + i.scans[0].data_size]
    nsub = -(-len(ent) // STUFFED_S)
    assert nsub > 100 and all(ent[k * STUFFED_S - 1] == 0xFF and ent[k * STUFFED_S] == 0 for k in range(1, nsub)), "a boundary that is no stuffed zero"
    st = check_subseq(M, c, STUFFED_S, setenv)
    # every guess was right: the first group of synchronisation rounds (three launches) finds nothing to change
    assert st["subseq"] == STUFFED_S and st["rounds"] <= 3, "%d rounds for %d subsequences" % (st["rounds"], nsub)
    return st, nsub


def lone_eob_case(seed=240):
    """gray, every code 16 bits long, four AC symbols: every block ends on position 63 but one, whose EOB is the table's rarest
    symbol and therefore the last 16-bit code"""
    comps = gray()
    rows, cols = W.padded_blocks(45, 37, comps, 0)
    rng = np.random.default_rng(seed)
    a = np.zeros((rows * cols, 64), np.int64)
    a[:, 0] = rng.integers(-50, 51, rows * cols)
    a[:, [3, 9, 63]] = rng.choice([-1, 1], (rows * cols, 3))
    a[7, 63] = 0
    return build(seed, 45, 37, comps, coefs=[a.reshape(rows, cols, 64)], scans=one_scan(1, "all16"), edges=False, transforms=())


def undefine_rarest_code(c, cls=1, tid=0):
    """the file of a one-scan case with the last (rarest) symbol of one Huffman table removed from its DHT segment: the stream now holds
    a code word of the table's longest length that no entry exists for.  Returns (bytes, the symbol)."""
    data = c.data
    pos = data.index(b"\xff\xc4")
    n = int.from_bytes(data[pos + 2:pos + 4], "big")
    seg, o, out, sym = data[pos + 4:pos + 2 + n], 0, bytearray(), None
    while o < len(seg):
        head, bits = seg[o], list(seg[o + 1:o + 17])
        vals = seg[o + 17:o + 17 + sum(bits)]
        o += 17 + len(vals)
        if head == cls * 16 + tid:
            bits[max(k for k in range(16) if bits[k])] -= 1
            sym, vals = vals[-1], vals[:-1]
        out += bytes([head]) + bytes(bits) + bytes(vals)
    assert sym is not None
    return data[:pos] + b"\xff\xc4" + (len(out) + 2).to_bytes(2, "big") + bytes(out) + data[pos + 2 + n:], sym

META["slow_sync_96"] = dict(codings=CODINGS, transforms=())
# long codes over many subsequences
_simple("long_all16_200x120", 230, ycc(*S420), w=200, h=120, scans=one_scan(3, "all16"), density=0.05, transforms=())
_simple("long_deep_200x120", 231, ycc(*S420), w=200, h=120, scans=one_scan(3, "deep"), density=0.05, transforms=())
_simple("long_two_scans_200x120", 232, ycc(*S420), w=200, h=120, density=0.05, transforms=(),
        scans=[dict(comps=[0], dc=[0], ac=[0], ri=13, shape="all16"), dict(comps=[1, 2], dc=[0, 0], ac=[0, 0], ri=0, shape="deep")])
SUBSEQ_CASES = ("long_all16_200x120", "long_deep_200x120", "long_two_scans_200x120")

NAMES = list(CASES)
TRANSCODE_PAIRS = [(n, sw) for n in NAMES for sw in META[n]["codings"]]
TRANSFORM_NAMES = [n for n in NAMES if META[n]["transforms"]]

# small sizes x five samplings, decode only
SMALL_SIZES = [(1, 1), (2, 3), (3, 2), (4, 4), (5, 1), (6, 17), (7, 7), (8, 9), (9, 8), (15, 16), (16, 15), (17, 33), (31, 5), (32, 32), (33, 1)]
SMALL_SAMPLINGS = {"420": S420, "422": ((2, 1), (1, 1), (1, 1)), "440": ((1, 2), (1, 1), (1, 1)), "411": ((4, 1), (1, 1), (1, 1)), "444": ((1, 1), (1, 1), (1, 1))}
SMALL = [(w, h, s) for (w, h) in SMALL_SIZES for s in SMALL_SAMPLINGS]
SMALL_LAYOUTS = ("bgr", "xrgb")


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def small_case(w, h, samp):
    return build(1000 + 37 * w + h, w, h, ycc(*SMALL_SAMPLINGS[samp]), density=0.15, scans=one_scan(3, ("optimal", "deep", "all9")[(w + h) % 3]))


# ---- premises -----------------------------------------------------------------------------------------------------------------------
def dqt_precisions(data):
    """{table number: Pq} of the DQT segments in front of the first SOS"""
    out, pos = {}, 2
    while data[pos + 1] != 0xDA:
        if data[pos + 1] == 0xFF or data[pos + 1] == 0x01:
            pos += 1 if data[pos + 1] == 0xFF else 2
            continue
        n = (data[pos + 2] << 8) | data[pos + 3]
        if data[pos + 1] == 0xDB:
            q = pos + 4
            while q < pos + 2 + n:
                out[data[q] & 15] = data[q] >> 4
                q += 1 + (128 if data[q] >> 4 else 64)
        pos += 2 + n
    return out


def check_premise(M, c):
    """the description really is in the bytes: frame, table ids, restart intervals, DQT precision, code lengths, the block edges"""
    i = M.jpeg_info(c.data)
    assert (i.image_width, i.image_height, i.num_components, i.sof_type) == (c.width, c.height, len(c.comps), c.sof)
    for k, (cid, h, v, tq) in enumerate(c.comps):
        assert (i.component_id[k], i.h_samp_factor[k], i.v_samp_factor[k], i.quant_tbl_no[k]) == (cid, h, v, tq)
    assert i.num_scans == len(c.scans)
    for k, s in enumerate(c.scans):
        sc = i.scans[k]
        n = len(s["comps"])
        assert [sc.component_index[j] for j in range(n)] == list(s["comps"]) and sc.comps_in_scan == n
        assert [sc.dc_tbl_no[j] for j in range(n)] == list(s["dc"]) and [sc.ac_tbl_no[j] for j in range(n)] == list(s["ac"])
        assert sc.restart_interval == s.get("ri", 0)
        for (cls, t), (bits, vals) in c.stats["scans"][k].items():           # the tables in force at this scan are this scan's own
            slot = 2 * t + (cls == "ac")
            assert list(sc.huff_bits[slot])[1:] == bits[1:] and list(sc.huff_vals[slot])[:len(vals)] == vals
    assert dqt_precisions(c.data) == {t: p for t, (p, _) in c.qtables.items()}
    for t, (_, q) in c.qtables.items():
        assert [i.quantval[t][DC.ZIGZAG[k]] for k in range(64)] == list(q)
    assert bool(i.saw_JFIF_marker) == (c.header == "jfif") and bool(i.saw_Adobe_marker) == (isinstance(c.header, tuple))
    if c.long_codes:
        assert c.stats["long_share"] >= 0.5, "only %.2f of the code words are longer than 8 bits" % c.stats["long_share"]
    if c.edges:
        a = np.concatenate([x.reshape(-1, 64) for x in c.coefs])
        nz = a[:, 1:] != 0
        assert (a[:, 63] != 0).any(), "no block without EOB"
        assert ((a[:, 63] != 0) & (nz.sum(axis=1) == 1)).any(), "no ZRL triple (a lone coefficient at 63)"
        assert (~nz.any(axis=1)).any() and (nz.all(axis=1)).any(), "no all-zero / no dense block"
        assert (a[:, 1:] == 1023).any() and (a[:, 1:] == -1023).any() and (np.abs(np.diff(a[:, 0])) == 2047).any()


def expected_colour_space(M, c):
    """default_decompress_parms (jdapimin.c): one component gray; JFIF YCbCr; Adobe by its transform; else by the component ids"""
    if len(c.comps) == 1:
        return M.CS_GRAYSCALE
    if c.header == "jfif":
        return M.CS_YCBCR
    if isinstance(c.header, tuple):
        return M.CS_RGB if c.header[1] == 0 else M.CS_YCBCR
    return M.CS_RGB if [x[0] for x in c.comps] == [82, 71, 66] else M.CS_YCBCR


# ---- the checks both test files run ---------------------------------------------------------------------------------------------------
def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def transcode(M, data, sw, max_batch=1, **xf):
    enc = M.Encoder(M.params_from_jpeg(data, **TC.SWITCHES[sw][0], **xf), max_batch=max_batch)
    try:
        return enc.transcode_host([data])[0]
    finally:
        enc.close()


def check_transcode(M, c, sw):
    status, ref = TC.jpegtran_status(c.data, ["-copy", "none"] + TC.SWITCHES[sw][1])
    assert status == c.status and ref is not None, "the reference's jpegtran exits with %d" % status
    out = transcode(M, c.data, sw)
    assert out == ref, "%d bytes, the reference %d; first difference at %d" % (
        len(out), len(ref), next((k for k in range(min(len(out), len(ref))) if out[k] != ref[k]), -1))


def check_decode(M, c, layouts=()):
    enc = M.Encoder(M.params_from_jpeg(c.data, revert=True), max_batch=1)
    try:
        for mode in c.modes:
            kw, args = DC.MODES[mode]
            status, ref = DC.djpeg_status(c.data, args)
            assert status == c.status and ref is not None, "the reference's djpeg exits with %d (%s)" % (status, mode)
            out = enc.decode_host([c.data], **kw)[0]
            assert same(out, ref), "%s: %s, the reference %s" % (mode, out.shape, ref.shape)
            if mode == "rgb":
                for layout in layouts:
                    DC.check_layout(ref, enc.decode_host([c.data], color="rgb", layout=layout)[0], layout)
    finally:
        enc.close()


def check_transforms(M, c):
    import pytest
    for xf in c.transforms:
        status, ref = TC.jpegtran_status(c.data, ["-copy", "none"] + XC.jpegtran_args(**xf) + TC.SWITCHES["revert"][1])
        assert status == c.status and ref is not None, "the reference's jpegtran exits with %d on %s" % (status, xf)
        assert transcode(M, c.data, "revert", **xf) == ref, str(xf)
    if c.transforms:
        status, _ = TC.jpegtran_status(c.data, ["-copy", "none"] + XC.jpegtran_args(**REFUSED_TRANSFORM) + TC.SWITCHES["revert"][1])
        assert status == 1, "the reference accepts -perfect here (%d)" % status
        with pytest.raises(M.MjhError) as ei:
            transcode(M, c.data, "revert", **REFUSED_TRANSFORM)
        assert ei.value.code == M.EINVAL and "perfect" in str(ei.value)


def check_coefficients(M, c):
    """the coefficients the device decodes (TAP_COEF_Q) are the arrays the file was written from; the reference's programs accept it"""
    assert DC.djpeg_status(c.data)[0] == c.status
    assert TC.jpegtran_status(c.data, ["-copy", "none"])[0] == c.status
    enc = M.Encoder(M.params_from_jpeg(c.data, revert=True), max_batch=1)
    try:
        enc.decode_host([c.data])
        for ci in range(len(c.comps)):
            rows, cols = W.real_blocks(c.width, c.height, c.comps, ci)
            got = enc.read_tap(M.TAP_COEF_Q, 0, ci)                      # [64 zig-zag][blocks]
            want = c.coefs[ci][:rows, :cols].reshape(-1, 64)
            assert np.array_equal(got.T, want), "component %d" % ci
    finally:
        enc.close()


def check_fractional_refusal(M):
    """(2,1)(3,1)(1,1): the reference's djpeg stops (JERR_FRACT_SAMPLE_NOTIMPL, exit 1), and no encoder can be made for the frame
    (MJH_EUNSUPPORTED), so decode() and recompress() put that error into the file's slot and leave the other files alone.  The
    reference's jpegtran ACCEPTS the file (no resampling is involved in re-coding coefficients): this is a limit of this project's
    re-compression path that the reference does not have, pinned here under its name."""
    import pytest
    c, good = fractional_case(), case("samp_4x1_1x1_2x1")
    assert DC.djpeg_status(c.data)[0] == 1
    assert TC.jpegtran_status(c.data, ["-copy", "none", "-revert"])[0] == 0
    with pytest.raises(M.MjhError) as ei:
        M.Encoder(M.params_from_jpeg(c.data, revert=True), max_batch=1)
    assert ei.value.code == M.EUNSUPPORTED and "fractional" in str(ei.value)
    r = M.decode([c.data, good.data])
    assert isinstance(r[0], M.MjhError) and r[0].code == M.EUNSUPPORTED and "fractional" in str(r[0])
    assert same(r[1], DC.djpeg(good.data))
    r = M.recompress([good.data, c.data], revert=True)
    assert isinstance(r[1], M.MjhError) and r[1].code == M.EUNSUPPORTED and "fractional" in str(r[1])
    assert r[0] == TC.jpegtran_status(good.data, ["-copy", "none", "-revert"])[1]


def check_out_of_range(M, name):
    """decode == djpeg (exit 0) in every mode; re-compression refuses as the reference's jpegtran does (JERR_BAD_DCT_COEF, exit 1);
    in a batch the good files on either side are unaffected"""
    import pytest
    c = oor_case(name)
    check_premise(M, c)
    check_decode(M, c)
    status, _ = TC.jpegtran_status(c.data, ["-copy", "none", "-revert"])
    assert status == 1, "the reference's jpegtran exits with %d" % status
    left, right = oor_neighbour(0, name == "oor_dc_6000"), oor_neighbour(1, name == "oor_dc_6000")
    files = [left.data, c.data, right.data]
    enc = M.Encoder(M.params_from_jpeg(c.data, revert=True), max_batch=3)
    try:
        with pytest.raises(M.MjhError) as ei:
            enc.transcode_host([c.data])
        assert ei.value.code == M.EINVAL and "JERR_BAD_DCT_COEF" in str(ei.value) and "Corrupt" not in str(ei.value)
        res = enc.transcode_host(files, errors="return")
        assert res[0] is None and res[2] is None and isinstance(res[1], M.MjhError)
        assert res[1].code == M.EINVAL and "JERR_BAD_DCT_COEF" in str(res[1]) and "Corrupt" not in str(res[1])
        assert [enc.transcode_status(k)[0] for k in range(3)] == [M.OK, M.EINVAL, M.OK]
        outs = enc.decode_host(files)
        for f, o in zip(files, outs):
            assert same(o, DC.djpeg(f))
    finally:
        enc.close()
    out = M.recompress(files, revert=True)
    assert isinstance(out[1], M.MjhError) and "JERR_BAD_DCT_COEF" in str(out[1])
    for k in (0, 2):
        assert out[k] == TC.jpegtran_status(files[k], ["-copy", "none", "-revert"])[1]


def check_subseq(M, c, S, setenv):
    """decode and revert_opt under a subsequence length; returns the decoder's statistics of the transcode call"""
    setenv(S)
    enc = M.Encoder(M.params_from_jpeg(c.data, revert=True, optimize=True), max_batch=1)
    try:
        out = enc.transcode_host([c.data])[0]
        st = enc.transcode_stats()
        pix = enc.decode_host([c.data])[0]
    finally:
        enc.close()
    assert out == TC.jpegtran_status(c.data, ["-copy", "none", "-revert", "-optimize"])[1]
    assert same(pix, DC.djpeg(c.data))
    return st


def check_slow_sync(M, c, S, setenv):
    """the premise: synchronisation takes (nearly) one round per subsequence, i.e. no lane finds a code boundary by chance"""
    i = M.jpeg_info(c.data)
    st = check_subseq(M, c, S, setenv)
    nsub = -(-i.scans[0].data_size // st["subseq"])
    assert st["rounds"] >= nsub - 2, "%d rounds for %d subsequences" % (st["rounds"], nsub)
    return st, nsub


# ---- sizes the emulator cannot afford (test_gpu_streams.py) ----------------------------------------------------------------------------
BIG_QTABLES = {0: quant(5000, 1, 40), 1: quant(5001, 1, 60)}
BIG_SCANS = {
    "all16": lambda: one_scan(3, "all16"),
    "all16_shared_pair": lambda: one_scan(3, "all16", dc=[0, 0, 0], ac=[0, 0, 0]),
    # one MCU row of luma blocks per interval in the first scan (240 blocks across), none in the second
    "all16_two_scans": lambda: [dict(comps=[0], dc=[0], ac=[0], ri=240, shape="all16"), dict(comps=[1, 2], dc=[0, 0], ac=[0, 0], ri=0, shape="all16")],
}


@functools.lru_cache(maxsize=None)
def big_case(kind, seed=500, w=1920, h=1080):
    """1920 x 1080, 4:2:0; kind: a key of BIG_SCANS or a table shape"""
    scans = BIG_SCANS[kind]() if kind in BIG_SCANS else one_scan(3, kind)
    return build(seed, w, h, ycc(*S420), scans=scans, qtables=BIG_QTABLES, density=0.05, transforms=())


BIG_BATCH_SHAPES = ("all16", "optimal", "deep", "all9", "full256", ("all16", "optimal"), ("deep", "all9"), ("optimal", "full256"))


def big_batch():
    """eight 1080p files of one signature, each in another table shape and with other content"""
    return [big_case(s, 510 + k) for k, s in enumerate(BIG_BATCH_SHAPES)]


@functools.lru_cache(maxsize=None)
def small_batch(n=64):
    """n small files of one signature: table shapes, table ids, scan layouts and restart intervals all differ"""
    out = []
    for k in range(n):
        shape = W.SHAPES[k % len(W.SHAPES)]
        if k % 4 == 3:
            scans = [dict(comps=[0], dc=[k % 3], ac=[(k + 1) % 4], ri=k % 7, shape=shape),
                     dict(comps=[1, 2], dc=[0, k % 4], ac=[k % 2, 3], ri=(k // 4) % 3, shape=W.SHAPES[(k + 2) % len(W.SHAPES)])]
        else:
            scans = one_scan(3, shape, ri=k % 5, dc=[k % 4, (k + 1) % 4, (k + 2) % 4], ac=[(k + 3) % 4, k % 4, k % 4])
        out.append(build(600 + k, 45, 37, ycc(*S420), scans=scans, sof=1, qtables={0: quant(6000), 1: quant(6001)}))
    return out


def check_batch(M, cases, max_batch=None):
    """one decode call and one revert_opt call over the files: every result is its own file's reference"""
    files = [c.data for c in cases]
    n = len(files)
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True, optimize=True), max_batch=max_batch or n)
    try:
        outs = enc.transcode_host(files)
        pix = enc.decode_host(files)
    finally:
        enc.close()
    for k, c in enumerate(cases):
        assert outs[k] == TC.jpegtran_status(c.data, ["-copy", "none", "-revert", "-optimize"])[1], "file %d" % k
        assert same(pix[k], DC.djpeg(c.data)), "file %d" % k
