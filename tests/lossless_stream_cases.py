"""The case list and checks of the lossless stream tests (test_simt_lossless_streams.py on the emulator, test_gpu_lossless_streams.py
on the chip): lossless files (SOF3) that the reference's djpeg reads without a message and that no libjpeg encoder writes, made from
seeds at test time by jpeg_writer_lossless.write_lossless.  The reference's cjpeg names DC table 0 for every component of a scan,
writes frequency-optimal tables and one DRI in front of the first scan, and never lets a reconstructed value need more than P
bits; the files here have a table slot per component, tables of every shape and placement, a restart interval per scan, fill bytes
in front of markers, component ids of every kind, and running values that use all 16 bits at every precision.

Every file is first checked against the reference with no kernel involved (check_premise): oracle/_ref/djpeg -pnm exits 0, prints
nothing and returns exactly the writer's `expected` (shape, dtype and values), and the writer's statistics show the construct the
case exists for.  Then decode(lossless_sources=True) must return djpeg's samples, jpeg_info must report every scan as the writer
wrote it, and two cases go through the pixel layouts.  Every comparison is exact equality; nothing expected comes from the code
under test.

The `modular` family: files whose running values exceed 2^(P - Pt).  T.81 defines the arithmetic modulo 2^16 and the reference
decodes them silently, truncating to the sample type on output; they are not images any encoder was given.  They are here
because they put all 16 bits through every predictor at the precisions whose ordinary files never do."""
import functools

import numpy as np

import jpeg_writer as W
import jpeg_writer_lossless as WL
import lossless_decode_cases as LD

have_tools = LD.have_tools

H0, W0 = 13, 21


class Case:
    """one generated file and what the tests need to know about it"""
    def __init__(self, precision, planes, scans, modular=False, **kw):
        if not modular:                                     # an image of P bits: its running values are the samples >> Pt
            planes = list(planes)
            for s in scans:
                for c in s["comps"]:
                    planes[c] = planes[c] >> s["pt"]
                    assert int(planes[c].max()) << s["pt"] < (1 << precision)
        self.precision, self.planes, self.scans, self.kw = precision, planes, scans, kw
        self.data, self.expected, self.stats = WL.write_lossless(precision, planes, scans, **kw)
        self.height, self.width = planes[0].shape

    def tables(self):
        """every (bits, huffval) of the file, in scan and slot order"""
        return [(tuple(b), tuple(v)) for st in self.stats["scans"] for _, (b, v) in sorted(st["tables"].items())]


# ---- planes -------------------------------------------------------------------------------------------------------------------------
def noise(seed, n, top, h=H0, w=W0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, top, (h, w)) for _ in range(n)]


def varied(seed, h=H0, w=W0):
    """three 8-bit planes whose differences are distributed differently: uniform noise, noise crowded towards 0, noise with flat runs"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w))
    b = rng.integers(0, 256, (h, w)) ** 2 // 255
    c = np.where(rng.integers(0, 2, (h, w)) == 1, 100, rng.integers(0, 256, (h, w)))
    return [a, b, c]


def wide(seed, n, precision, psv, pt=0, rows=0, h=H0, w=W0):
    """planes uniform over 0 .. 2^(16 - pt) - 1, with differences placed by hand in every plane: 32768 (category 16) on the first
    sample and on one in the interior, and one of every category 9 .. 15 (a plane of 273 uniform samples may miss the rarer ones)"""
    out = noise(seed, n, 1 << (16 - pt), h, w)
    for x in out:
        # in raster order: a prediction is made of earlier samples only
        for y, c, d in [(0, 0, 32768)] + [(k - 8, 5, (1 << (k - 1)) + k) for k in range(9, 16)] + [(h - 2, w // 2, 32768)]:
            x[y, c] = (WL.predictions(x, precision, pt, psv, rows)[y, c] + d) & 0xFFFF
    return out


def scan(comps, psv, tables, pt=0, rows=0, **kw):
    return dict(comps=list(comps), psv=psv, pt=pt, rows=rows, tables=list(tables), **kw)


# ---- the families -------------------------------------------------------------------------------------------------------------------
CASES, PREMISES, REFUSED = {}, {}, {}


def _distinct_tables(c):
    t = c.tables()
    assert len(t) >= 2 and len(set(t)) == len(t), "tables that do not differ in content"


def _categories(c):
    return np.sum([h for st in c.stats["scans"] for h in st["categories"].values()], axis=0)


# tables: a slot per component of an interleaved scan, every shape
def _p_slots(c):
    _distinct_tables(c)
    assert sorted(c.stats["scans"][0]["tables"]) == [1, 2, 3] and c.scans[0]["tables"] == [1, 3, 2]


def _p_all16(c):
    _p_slots(c)
    assert c.stats["scans"][0]["long_share"] == 1.0 and all(sum(b[1:16]) == 0 for b, _ in c.tables())


def _p_all9(c):
    _p_slots(c)
    assert c.stats["scans"][0]["long_share"] == 1.0 and all(b[9] == len(v) for b, v in c.tables())


def _p_deep(c):
    _p_slots(c)
    # (the seven rarest symbols take the codes of 1 .. 7 bits; of the nine categories of 8-bit noise the two most frequent stay long)
    assert all(b[16] > 0 and b[1] == 1 for b, _ in c.tables()) and c.stats["scans"][0]["long_share"] > 0.4


def _p_deep17(c):
    _p_deep(c)
    assert all(sorted(v) == list(range(17)) for _, v in c.tables())
    used = _categories(c)
    assert used[9:].sum() == 0, "an 8-bit image uses the categories up to 8: the other eight are defined and unused"
    assert c.stats["scans"][0]["long_share"] > 0.9, "the short codes went to the unused categories"


CASES["t_slots_132"] = lambda: Case(8, varied(1), [scan((0, 1, 2), 4, (1, 3, 2))])
for _shape in ("all16", "all9", "deep", "deep17"):
    CASES["t_" + _shape] = (lambda s: lambda: Case(8, varied(2), [scan((0, 1, 2), 7, (1, 3, 2), shape=s)]))(_shape)
PREMISES.update(t_slots_132=_p_slots, t_all16=_p_all16, t_all9=_p_all9, t_deep=_p_deep, t_deep17=_p_deep17)


def _p_one_symbol(c):
    (st,) = c.stats["scans"]
    bits, vals = st["tables"][0]
    assert bits[1:] == [1] + [0] * 15 and vals == [0], "one symbol with a 1-bit code"
    assert (c.height, c.width) == (120, 5) and st["data_bytes"] == 75 and st["ff_bytes"] == 0
    assert 64 * 8 // c.width > 100, "the first subsequence of 64 bytes holds more than 100 rows"


CASES["t_one_symbol"] = lambda: Case(8, [np.full((120, 5), 128)], [scan((0,), 1, (0,))])
PREMISES["t_one_symbol"] = _p_one_symbol


def _p_upfront(c):
    assert c.stats["dht"] == [(0, [0, 1, 2])], "one DHT segment, in front of the first SOS, with the three tables"
    assert c.data.count(b"\xff\xc4") == 1 and c.data.index(b"\xff\xc4") < c.data.index(b"\xff\xda")
    _distinct_tables(c)


CASES["t_upfront_one_dht"] = lambda: Case(8, varied(3), [scan((0,), 2, (0,), dht="upfront_merged"), scan((1,), 5, (1,), dht="upfront_merged", shape="all9"),
                                                         scan((2,), 1, (2,), dht="upfront_merged", shape="deep17")])
PREMISES["t_upfront_one_dht"] = _p_upfront


def _p_redefined(c):
    assert [d for d in c.stats["dht"]] == [(0, [0]), (1, [0]), (2, [0])]
    _distinct_tables(c)


CASES["t_slot_redefined"] = lambda: Case(8, varied(4), [scan((0,), 6, (0,)), scan((1,), 6, (0,)), scan((2,), 3, (0,), shape="all16")])
PREMISES["t_slot_redefined"] = _p_redefined


def _p_shared(c):
    assert c.stats["dht"] == [(0, [1]), (2, [0])], "the second scan defines nothing"
    a, b = c.stats["scans"][0], c.stats["scans"][1]
    assert a["tables"][1] is b["tables"][1] and (a["categories"][1] != b["categories"][1]).any()


CASES["t_shared_table"] = lambda: Case(8, varied(5), [scan((0,), 4, (1,)), scan((1,), 7, (1,), tables_from=0), scan((2,), 2, (0,))])
PREMISES["t_shared_table"] = _p_shared


def _p_th3(c):
    assert sorted(c.stats["scans"][0]["tables"]) == [3] and c.stats["dht"] == [(0, [3])]


CASES["t_th3"] = lambda: Case(8, noise(6, 1, 256), [scan((0,), 5, (3,))])
PREMISES["t_th3"] = _p_th3


# restarts
def _p_per_scan(c):
    assert c.stats["dri"] == [3 * W0, 0, 5 * W0], "a DRI in front of every scan, the second of 0"
    assert [len(st["rst"]) for st in c.stats["scans"]] == [4, 0, 2]
    assert [s["psv"] for s in c.scans] == [1, 6, 2] and [tuple(s["comps"]) for s in c.scans] == [(2,), (0,), (1,)]


CASES["r_interval_per_scan"] = lambda: Case(8, varied(10), [scan((2,), 1, (0,), rows=3), scan((0,), 6, (1,), pt=1), scan((1,), 2, (0,), rows=5)])
PREMISES["r_interval_per_scan"] = _p_per_scan


def _p_beyond(c):
    assert c.stats["dri"] == [40 * W0] and c.stats["scans"][0]["rst"] == [] and c.height == 13


CASES["r_beyond_image"] = lambda: Case(8, varied(11), [scan((0, 1, 2), 3, (0, 0, 0), rows=40)])
PREMISES["r_beyond_image"] = _p_beyond


def _p_fill(n):
    def check(c):
        rst = c.stats["scans"][0]["rst"]
        assert rst == [0xD0 + k for k in range(6)]
        for m in rst:
            assert c.data.count(b"\xff" * (n + 1) + bytes([m])) == 1 and c.data.count(b"\xff" * (n + 2) + bytes([m])) == 0
    return check


for _n in (1, 2, 3):
    CASES["r_fill_%d" % _n] = (lambda n: lambda: Case(8, varied(12), [scan((0, 1, 2), 5, (0, 0, 0), rows=2, fill={"RST": n})]))(_n)
    PREMISES["r_fill_%d" % _n] = _p_fill(_n)


def _p_wrap(c):
    assert c.stats["scans"][0]["rst"] == [0xD0 + (k & 7) for k in range(12)], "thirteen intervals: RST0 .. RST7, RST0 .. RST3"


CASES["r_wrap"] = lambda: Case(8, noise(13, 1, 256), [scan((0,), 7, (0,), rows=1)])
PREMISES["r_wrap"] = _p_wrap


def _p_w1(c):
    st = c.stats["scans"][0]
    assert c.width == 1 and len(st["rst"]) == c.height - 1 and st["dri"] == 1, "segments of one MCU"


CASES["r_w1"] = lambda: Case(8, varied(14, 13, 1), [scan((0, 1, 2), 4, (0, 1, 0), rows=1)])
PREMISES["r_w1"] = _p_w1


def _p_strip(rows, psv):
    def check(c):
        st = c.stats["scans"][0]
        assert c.height == 130 and c.scans[0]["psv"] == psv and st["dri"] == rows * c.width and len(st["rst"]) == -(-130 // rows) - 1
    return check


# 63 rows below the interval's first fill the wavefront's strip exactly, 64 and 65 hand over to a strip of 1 and 2 rows
for _rows, _psv in ((63, 6), (64, 7), (65, 4)):
    CASES["r_strip_%d" % _rows] = (lambda r, p: lambda: Case(8, noise(15 + r, 1, 256, 130, 9), [scan((0,), p, (0,), rows=r)]))(_rows, _psv)
    PREMISES["r_strip_%d" % _rows] = _p_strip(_rows, _psv)
# predictor 1: the chain down column 0 is carried from the 64th row of an interval to the 65th
CASES["r_col0_65"] = lambda: Case(8, noise(16, 1, 256, 130, 9), [scan((0,), 1, (0,), rows=65)])
PREMISES["r_col0_65"] = _p_strip(65, 1)


# modular: running values that use all 16 bits in 8-bit and 12-bit files
def _p_modular(c):
    used = _categories(c)
    assert used[16] >= 2 * len(c.planes), "the difference 32768, placed by hand twice a plane"
    assert (used[9:16] >= len(c.planes)).all(), "categories 9 .. 15"
    top = max(int(p.max()) for p in c.planes) << c.scans[0]["pt"]
    assert top >= 0xF000 and (c.precision == 16 or top > (1 << c.precision)), "values that use all 16 bits, beyond the precision"


MODULAR = []
for _p in (8, 12):
    for _psv in range(1, 8):
        for _n in (1, 3):
            _name = "m%d_psv%d_%s" % (_p, _psv, "gray" if _n == 1 else "rgb")
            CASES[_name] = (lambda p, v, n: lambda: Case(p, wide(100 * p + 10 * v + n, n, p, v), [scan(range(n), v, (0, 1, 2)[:n])], modular=True))(_p, _psv, _n)
            MODULAR.append(_name)
CASES["m8_pt3_rgb"] = lambda: Case(8, wide(30, 3, 8, 5, pt=3), [scan((0, 1, 2), 5, (0, 1, 2), pt=3)], modular=True)
CASES["m12_pt3_gray"] = lambda: Case(12, wide(31, 1, 12, 7, pt=3), [scan((0,), 7, (0,), pt=3)], modular=True)
CASES["m8_rows_rgb"] = lambda: Case(8, wide(32, 3, 8, 6, rows=4), [scan((0, 1, 2), 6, (0, 1, 2), rows=4)], modular=True)
CASES["m12_rows_gray"] = lambda: Case(12, wide(33, 1, 12, 4, rows=4), [scan((0,), 4, (0,), rows=4)], modular=True)
CASES["m12_pt3_rows_rgb"] = lambda: Case(12, wide(34, 3, 12, 6, pt=3, rows=5), [scan((0, 1, 2), 6, (2, 0, 1), pt=3, rows=5)], modular=True)
MODULAR += ["m8_pt3_rgb", "m12_pt3_gray", "m8_rows_rgb", "m12_rows_gray", "m12_pt3_rows_rgb"]
# the same values where they are ordinary: a 16-bit RGB file (it also serves the pixel layouts)
CASES["m16_psv7_rgb"] = lambda: Case(16, wide(35, 3, 16, 7), [scan((0, 1, 2), 7, (2, 0, 1), shape="deep17")], modular=True)
MODULAR.append("m16_psv7_rgb")
for _name in MODULAR:
    PREMISES[_name] = _p_modular


# ones: every difference +32767, which a one-symbol table codes as a 0-bit and fifteen 1-bits
def _p_ones(c):
    (st,) = c.stats["scans"]
    bits, vals = st["tables"][0]
    assert bits[1:] == [1] + [0] * 15 and vals == [15] and st["categories"][0][15] == c.height * c.width
    assert st["ff_bytes"] >= 0.30 * st["data_bytes"], "%d of %d" % (st["ff_bytes"], st["data_bytes"])
    assert st["data_bytes"] > 20 * 64 and not st["rst"]


CASES["ones"] = lambda: Case(16, [(32768 + 32767 * (1 + np.add.outer(np.arange(13), np.arange(64)))) & 0xFFFF], [scan((0,), 1, (0,))])
PREMISES["ones"] = _p_ones


# sync_long: 16-bit noise under a table whose codes are all 16 bits long, one segment
def _p_sync_long(c):
    (st,) = c.stats["scans"]
    assert st["long_share"] == 1.0 and not st["rst"] and st["data_bytes"] > 400 * 64 and (c.height, c.width) == (31, 300)


CASES["sync_long"] = lambda: Case(16, noise(40, 1, 65536, 31, 300), [scan((0,), 1, (0,), shape="all16")])
PREMISES["sync_long"] = _p_sync_long


# frames
def _p_ids(ids):
    def check(c):
        at = c.data.index(b"\xff\xc3")
        assert [c.data[at + 10 + 3 * k] for k in range(3)] == list(ids)
        assert b"JFIF" not in c.data and b"Adobe" not in c.data
    return check


for _tag, _ids in (("0_200_7", (0, 200, 7)), ("1_2_3", (1, 2, 3)), ("RGB", (82, 71, 66))):
    CASES["f_ids_" + _tag] = (lambda ids: lambda: Case(8, varied(50), [scan((0, 1, 2), 1, (0, 1, 0))], ids=ids))(_ids)
    PREMISES["f_ids_" + _tag] = _p_ids(_ids)
def _p_marker(marker, word):
    def check(c):
        assert c.data[2:4] == marker and c.data[6:6 + len(word)] == word
    return check


CASES["f_adobe0"] = lambda: Case(8, varied(51), [scan((0, 1, 2), 1, (0, 1, 0))], header=("adobe", 0))
PREMISES["f_adobe0"] = _p_marker(b"\xff\xee", b"Adobe\0")
CASES["f_gray_jfif"] = lambda: Case(8, noise(52, 1, 256), [scan((0,), 1, (0,))], header="jfif")
PREMISES["f_gray_jfif"] = _p_marker(b"\xff\xe0", b"JFIF\0")
def _p_order(order):
    def check(c):
        assert [tuple(s["comps"]) for s in c.scans] == order and sorted({k for k, _ in c.stats["dht"]}) == list(range(len(order)))
    return check


CASES["f_order_2_0_1"] = lambda: Case(8, varied(53), [scan((2,), 7, (0,)), scan((0,), 1, (1,), pt=2), scan((1,), 3, (2,), rows=6)])
PREMISES["f_order_2_0_1"] = _p_order([(2,), (0,), (1,)])
CASES["f_order_12_0"] = lambda: Case(8, varied(54), [scan((1, 2), 5, (1, 0), rows=4), scan((0,), 2, (0,), pt=1)])
PREMISES["f_order_12_0"] = _p_order([(1, 2), (0,)])


def _p_com(c):
    com, app = W.COM(b"between scans"), W.APPN(7, b"seven\0" + bytes(range(40)))
    a, b = c.data.index(com), c.data.index(app)
    sos = [i for i in range(len(c.data) - 1) if c.data[i:i + 2] == b"\xff\xda"]
    assert len(sos) >= 3 and sos[0] < a < sos[1] < b < sos[2]


CASES["f_com_appn"] = lambda: Case(8, varied(55), [scan((0,), 4, (0,)), scan((1,), 4, (0,), before=[W.COM(b"between scans")]),
                                                   scan((2,), 1, (0,), before=[W.APPN(7, b"seven\0" + bytes(range(40)))])])
PREMISES["f_com_appn"] = _p_com


def _p_fill_all(c):
    for marker, n in ((0xC4, 2), (0xDD, 1), (0xDA, 3), (0xD9, 2)):
        assert c.data.count(b"\xff" * (n + 1) + bytes([marker])) >= 1 and c.data.count(b"\xff" * (n + 2) + bytes([marker])) == 0, hex(marker)
    assert c.stats["dri"] == [4 * W0, 2 * W0] and [len(st["rst"]) for st in c.stats["scans"]] == [3, 6]


# fill bytes 0xFF in front of every kind of marker (B.1.1.2)
CASES["f_fill_everywhere"] = lambda: Case(8, varied(57), [scan((0, 1), 3, (0, 1), rows=4), scan((2,), 6, (1,), rows=2)],
                                          fill={"RST": 1, "SOS": 3, "DHT": 2, "DRI": 1, "EOI": 2})
PREMISES["f_fill_everywhere"] = _p_fill_all

# refused by the reference and here: a three-component lossless file that its markers call YCbCr
REFUSED["f_rgb_jfif"] = lambda: Case(8, varied(56), [scan((0, 1, 2), 1, (0, 1, 0))], header="jfif")
REFUSED["f_rgb_adobe1"] = lambda: Case(8, varied(56), [scan((0, 1, 2), 1, (0, 1, 0))], header=("adobe", 1))

# files of the reference's own encoder that the lists of lossless_decode_cases.py lack, checked as its cases are (check_case): full-range
# 16-bit noise under every predictor, gray and RGB; a flat image under a point transform; rows of one sample with a restart each
CJPEG_CASES = [("random", 19, 25, n, 16, psv, 0, None) for psv in range(1, 8) for n in (1, 3)] + \
              [("flat", 17, 23, 3, 8, 6, 1, None), ("random", 53, 1, 1, 8, 1, 0, 1)]

NAMES = list(CASES)
MULTI_SCAN = ["t_upfront_one_dht", "t_slot_redefined", "t_shared_table", "r_interval_per_scan", "f_order_2_0_1", "f_order_12_0", "f_com_appn", "f_fill_everywhere"]
LAYOUT_CASES = ["t_slots_132", "m16_psv7_rgb"]
# four files of one geometry (13 x 21 RGB, 8 bits) that differ in tables, intervals per scan, predictors and point transforms
BATCH = ["r_interval_per_scan", "t_all16", "r_fill_3", "m8_pt3_rgb"]


@functools.lru_cache(maxsize=None)
def case(name):
    return (CASES.get(name) or REFUSED[name])()


@functools.lru_cache(maxsize=None)
def reference(name):
    """djpeg's samples of the case's file, computed once and shared"""
    status, pix, err = LD.djpeg_run(case(name).data)
    assert status == 0 and err == "" and pix is not None, "djpeg: exit status %d, %r" % (status, err)
    pix.setflags(write=False)
    return pix


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def check_premise(name):
    """no kernel: the reference reads the file silently and returns the writer's samples; the file holds its construct"""
    c = case(name)
    ref = reference(name)
    assert LD.same(ref, c.expected), "%s: djpeg %s %s, the writer %s %s, first difference at %s" % (
        name, ref.shape, ref.dtype, c.expected.shape, c.expected.dtype, np.argwhere(ref != c.expected)[:1].tolist() if ref.shape == c.expected.shape else "-")
    PREMISES[name](c)


def check_lists():
    assert sorted(MULTI_SCAN) == sorted(n for n in NAMES if len(case(n).scans) > 1)
    assert set(PREMISES) == set(NAMES) and not set(REFUSED) & set(NAMES)


def check_decode(M, name):
    out = LD.decode1(M, case(name).data)
    ref = reference(name)
    assert LD.same(out, ref), "%s: %s %s, the reference %s %s, first difference at %s" % (
        name, out.shape, out.dtype, ref.shape, ref.dtype, np.argwhere(out != ref)[:1].tolist() if out.shape == ref.shape else "-")


def check_scans(M, name):
    """jpeg_info reports every scan as the writer wrote it"""
    c = case(name)
    info = M.jpeg_info(c.data, lossless_sources=True)
    assert (info.sof_type, info.data_precision, info.image_width, info.image_height, info.num_components) == (3, c.precision, c.width, c.height, len(c.planes))
    got = [(tuple(s.component_index[:s.comps_in_scan]), s.Ss, s.Se, s.Ah, s.Al, tuple(s.dc_tbl_no[:s.comps_in_scan]), s.restart_interval, s.restart_markers)
           for s in info.lossless_scans]
    want = [(tuple(s["comps"]), s["psv"], 0, 0, s["pt"], tuple(s["tables"]), s["rows"] * c.width, len(st["rst"])) for s, st in zip(c.scans, c.stats["scans"])]
    assert got == want


def check_layouts(M, name):
    """the reference's RGB rearranged; the fourth sample is the sample maximum"""
    c = case(name)
    rgb = reference(name)
    assert rgb.ndim == 3
    px, off = M.PIXEL_LAYOUTS["bgrx"]
    out = LD.decode1(M, c.data, layout="bgrx")
    assert out.shape == rgb.shape[:2] + (px,) and out.dtype == rgb.dtype
    for k in range(3):
        assert np.array_equal(out[:, :, off[k]], rgb[:, :, k])
    assert (out[:, :, 6 - sum(off)] == (1 << c.precision) - 1).all()
    assert LD.same(LD.decode1(M, c.data, bottom_up=True), rgb[::-1])
    assert LD.same(LD.decode1(M, c.data, layout="bgrx", bottom_up=True)[:, :, :3], rgb[::-1, :, ::-1])


def check_refused(M, name):
    """refused on both sides, each in its own words"""
    c = case(name)
    status, _, err = LD.djpeg_run(c.data)
    assert status != 0 and "Unsupported color conversion request" in err, (status, err)
    LD._refused(M, M.decode([c.data], lossless_sources=True)[0], M.EUNSUPPORTED, "colour conversion is not built")


def check_sync_long(M):
    """one entropy-coded segment of many subsequences under 16-bit codes: more than one round of synchronisation"""
    c = case("sync_long")
    info = M.jpeg_info(c.data, lossless_sources=True)
    assert len(info.lossless_scans) == 1 and info.lossless_scans[0].restart_markers == 0
    enc = M.Encoder(M.params_from_jpeg(info, revert=True), max_batch=1)
    try:
        enc.set_sources(progressive=False, lossless=True)
        out = enc.decode_host([c.data])[0]
        st = enc.transcode_stats()
        # (st["subseq"] is the length of a subsequence in bytes)
        assert 0 < st["subseq"] and 400 * st["subseq"] < info.lossless_scans[0].data_size and st["rounds"] > 1, st
        assert LD.same(out, reference("sync_long"))
    finally:
        enc.close()


def check_batch(M):
    """four hand-written files in one call of one encoder"""
    files = [case(n).data for n in BATCH]
    assert len(set(files)) == 4 and len({(case(n).height, case(n).width, case(n).precision, len(case(n).planes)) for n in BATCH}) == 1
    assert len({tuple((s["psv"], s["pt"], s["rows"], tuple(s["tables"])) for s in case(n).scans) for n in BATCH}) == 4
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True, lossless_sources=True), max_batch=4)
    try:
        enc.set_sources(progressive=False, lossless=True)
        out = enc.decode_host(files)
        for n, o in zip(BATCH, out):
            assert LD.same(o, reference(n)), n
    finally:
        enc.close()
    for n, o in zip(BATCH, M.decode(files, lossless_sources=True)):
        assert not isinstance(o, Exception), (n, o)
        assert LD.same(o, reference(n)), n
