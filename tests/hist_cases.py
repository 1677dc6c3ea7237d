"""The case list and helpers of the histogram tests (test_simt_hist.py on the emulator, test_gpu_hist.py on the chip): inputs whose
SYMBOL HISTOGRAMS are dictated, so that the branches of the optimal-table kernel (gen_table_body of mjh_kernels.hip: the length
limit of Figure K.3, the tie rule, the removal of the pseudo-symbol, the huffval order) and the forced flush of buffered correction
bits of the progressive coder (BE > 937, jcphuff.c:998; twice in mjh_prog.hip) are known to run.

  family A  sequential files from tests/jpeg_writer.py whose (run, size) histogram per output table is the dictated one, re-compressed
  family B  one-row 16-bit lossless images whose category histogram is the dictated one (17 categories + the pseudo-symbol = 18 leaves)
  family C  files whose every AC coefficient is 4..39: a refinement scan buffers 63 correction bits a block

Every expected byte comes from the reference's jpegtran / cjpeg (oracle/_ref) at test time; equality is exact.  Every case proves
its premise from the reference and from two restatements written here from jchuff.c / jcphuff.c (gen_optimal_table, ac_scan_walk),
never from the code under test; the restated table builder is itself checked against the DHT segments the reference writes.

What differs from a literal reading of the case list this file was written from:
  * gray 40x200 under a restart interval: one block row holds 5 blocks = 315 correction bits, so `-restart 1` can never buffer 938.
    That shape runs `-restart 4` (20 blocks an interval: the forced flush falls behind the 15th, five blocks follow); the two
    other shapes run `-restart 1`.
  * family C under the default switches: a file whose every AC coefficient is 4..39 never gets a refinement scan from the reference's
    scan search.  The search takes Al = 1 only if that is strictly smaller than Al = 0, and for such content the first scan at Al = 1
    saves exactly the bit a coefficient the refinement scan adds again, which leaves the second scan's header as a loss.  The `dense`
    and `mixed` files still run the default switches (bytes == jpegtran's; the premise asserts that the reference's file has no
    refinement scan, or is the source given back).  The forced flush in a file of the default switches is pinned by a third variant,
    `tail`: the first quarter of every component's blocks is dense, the other blocks hold 4..39 at positions 1..31 and +-1 at 32..63.
    The +-1 make Al = 1 pay (a table of their own), the dense quarter buffers 63 bits a block in the scan that refines to Al = 0.
  * the 4:2:0 files of family A have sizes that are multiples of 16, so that the blocks an interleaved scan codes are the blocks a
    non-interleaved one codes and one histogram holds for every coding."""
import functools
import os
import subprocess
import tempfile

import numpy as np

import jpeg_writer as W
import lossless_cases as LC
import stream_cases as SC
import transcode_cases as TC

have_tools = SC.have_tools

EOB, ZRL = 0x00, 0xF0
UNIT_Q = {0: (0, [1] * 64), 1: (0, [1] * 64)}

# name -> (keywords of mozjpeg_amd.params_from_jpeg / recompress, jpegtran's arguments)
CODINGS = {
    "revert_opt": TC.SWITCHES["revert_opt"],
    "revert_progressive": (dict(revert=True, progressive=True), ["-revert", "-progressive"]),
    "fastcrush_progressive": TC.SWITCHES["fastcrush_progressive"],
    "default": TC.SWITCHES["default"],
    "revert_progressive_restart1": (dict(revert=True, progressive=True, restart=1), ["-revert", "-progressive", "-restart", "1"]),
    "revert_progressive_restart4": (dict(revert=True, progressive=True, restart=4), ["-revert", "-progressive", "-restart", "4"]),
}
A_CODINGS = ("revert_opt", "revert_progressive", "fastcrush_progressive", "default")
PROGRESSIVE = ("revert_progressive", "fastcrush_progressive", "default")


# ---- restatement 1: jpeg_gen_optimal_table (jchuff.c) --------------------------------------------------------------------------------
def gen_optimal_table(freq):
    """(longest code length before limiting, moves of the K.3 loop, bits[0..16] with the pseudo-symbol removed, huffval) of the counts
    freq[0..255].  Section K.2 as jchuff.c writes it: pseudo-symbol 256 with a count of 1, the two smallest counts with ties towards
    the LARGER symbol, code sizes along the others[] chains, Figure K.3, the pseudo-symbol leaves the longest length still in use,
    huffval by (code size BEFORE limiting, symbol)."""
    freq = [int(v) for v in freq] + [0] * (256 - len(freq)) + [1]
    codesize, others = [0] * 257, [-1] * 257
    live = [i for i in range(257) if freq[i]]
    while True:
        c1, v = -1, 1000000000
        for i in live:
            if freq[i] <= v:
                v, c1 = freq[i], i
        c2, v = -1, 1000000000
        for i in live:
            if freq[i] <= v and i != c1:
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        live.remove(c2)
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    longest = max(codesize)
    assert longest <= 32, "JERR_HUFF_CLEN_OVERFLOW"
    bits = [0] * 33
    for i in range(257):
        if codesize[i]:
            bits[codesize[i]] += 1
    moves, i = 0, 32
    while i > 16:
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
            moves += 1
        i -= 1
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    huffval = [s for l in range(1, 33) for s in range(256) if codesize[s] == l]
    return longest, moves, bits[:17], huffval


# ---- restatement 2: the symbols and the forced flushes of one AC scan (jcphuff.c) ----------------------------------------------------
def ac_scan_walk(blocks, Ss, Se, Ah, Al, ri=0):
    """encode_mcu_AC_first / encode_mcu_AC_refine + emit_eobrun over the blocks of one non-interleaved scan in coding order.
    Returns dict(hist = symbol counts [256], be = flushes forced by BE > 937, run = flushes forced by EOBRUN == 0x7FFF,
    be_last = those of `be` behind the last block of a restart interval or of the scan)."""
    hist = [0] * 256
    n = len(blocks)
    st = dict(eobrun=0, be=0)
    forced = dict(be=0, run=0, be_last=0)

    def emit_eobrun():
        if st["eobrun"] > 0:
            hist[(st["eobrun"].bit_length() - 1) << 4] += 1
            st["eobrun"] = st["be"] = 0

    for b in range(n):
        if ri and b and b % ri == 0:                       # emit_restart
            emit_eobrun()
            st["eobrun"] = st["be"] = 0
        t = [abs(int(v)) >> Al for v in blocks[b]]
        r = br = 0
        if Ah == 0:
            for k in range(Ss, Se + 1):
                if t[k] == 0:
                    r += 1
                    continue
                emit_eobrun()
                while r > 15:
                    hist[ZRL] += 1
                    r -= 16
                hist[(r << 4) + t[k].bit_length()] += 1
                r = 0
        else:
            eob = max([k for k in range(Ss, Se + 1) if t[k] == 1], default=0)
            for k in range(Ss, Se + 1):
                if t[k] == 0:
                    r += 1
                    continue
                while r > 15 and k <= eob:
                    emit_eobrun()
                    hist[ZRL] += 1
                    r -= 16
                    br = 0
                if t[k] > 1:
                    br += 1
                    continue
                emit_eobrun()
                hist[(r << 4) + 1] += 1
                r = br = 0
        if r > 0 or br > 0:
            st["eobrun"] += 1
            st["be"] += br
            if st["eobrun"] == 0x7FFF:
                forced["run"] += 1
                emit_eobrun()
            elif st["be"] > 1000 - 64 + 1:
                forced["be"] += 1
                if b == n - 1 or (ri and (b + 1) % ri == 0):
                    forced["be_last"] += 1
                emit_eobrun()
    emit_eobrun()
    return dict(hist=hist, **forced)


# ---- the reference's files, read by their markers --------------------------------------------------------------------------------------
def scan_headers(data):
    """every scan of a file in order: dict(comps = component ids, tables = [(Td, Ta)], Ss, Se, Ah, Al, ri = the interval in force,
    dht = {(class, id): (bits[17], huffval)} in force)"""
    out, dht, ri, pos = [], {}, 0, 2
    while pos < len(data):
        assert data[pos] == 0xFF, "no marker at %d" % pos
        m = data[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        if m == 0xD9:
            break
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            pos += 2
            continue
        n = (data[pos + 2] << 8) | data[pos + 3]
        seg = data[pos + 4:pos + 2 + n]
        pos += 2 + n
        if m == 0xC4:
            o = 0
            while o < len(seg):
                bits = [0] + list(seg[o + 1:o + 17])
                dht[(seg[o] >> 4, seg[o] & 15)] = (bits, list(seg[o + 17:o + 17 + sum(bits)]))
                o += 17 + sum(bits)
        elif m == 0xDD:
            ri = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            ns = seg[0]
            out.append(dict(comps=[seg[1 + 2 * j] for j in range(ns)], tables=[(seg[2 + 2 * j] >> 4, seg[2 + 2 * j] & 15) for j in range(ns)],
                            Ss=seg[1 + 2 * ns], Se=seg[2 + 2 * ns], Ah=seg[3 + 2 * ns] >> 4, Al=seg[3 + 2 * ns] & 15, ri=ri, dht=dict(dht)))
            while not (data[pos] == 0xFF and data[pos + 1] != 0 and not 0xD0 <= data[pos + 1] <= 0xD7):      # entropy-coded data
                pos += 1
    return out


@functools.lru_cache(maxsize=None)
def ref_jpegtran(data, sw):
    """the reference's file for a coding; asserts exit status 0"""
    status, ref = TC.jpegtran_status(data, ["-copy", "none"] + CODINGS[sw][1])
    assert status == 0 and ref is not None, "the reference's jpegtran exits with %d" % status
    return ref


def run_quiet(tool, args, data, suffix):
    """the program exits 0 and prints nothing"""
    with tempfile.TemporaryDirectory() as td:
        inp = os.path.join(td, "in" + suffix)
        with open(inp, "wb") as f:
            f.write(data)
        r = subprocess.run([os.path.join(os.path.dirname(TC.JPEGTRAN), tool)] + list(args) + ["-outfile", os.path.join(td, "out"), inp],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0 and r.stdout + r.stderr == b"", "%s: exit %d, %r" % (tool, r.returncode, r.stdout + r.stderr)


def first_difference(out, ref):
    return "%d bytes, the reference %d; first difference at %d" % (
        len(out), len(ref), next((k for k in range(min(len(out), len(ref))) if out[k] != ref[k]), -1))


# ---- family A: blocks from a dictated (run, size) histogram ----------------------------------------------------------------------------
def ac_histogram(blocks):
    """the AC symbols of a sequential scan over these blocks ([n][64] zig-zag), counted the plain way"""
    hist = np.zeros(256, np.int64)
    for row in np.asarray(blocks).reshape(-1, 64):
        r = 0
        for k in range(1, 64):
            v = abs(int(row[k]))
            if v == 0:
                r += 1
                continue
            hist[ZRL] += r >> 4
            hist[((r & 15) << 4) + v.bit_length()] += 1
            r = 0
        if r:
            hist[EOB] += 1
    return hist


def _items(hist, rng):
    """one [zero run, size] per coefficient; every ZRL lengthens the run of some coefficient by 16"""
    items = [[s >> 4, s & 15] for s in sorted(hist) if s not in (EOB, ZRL) for _ in range(hist[s])]
    z = hist.get(ZRL, 0)
    while z:
        before = z
        for i in rng.permutation(len(items)):
            if z and items[i][0] + 16 <= 62:
                items[i][0] += 16
                z -= 1
        assert z < before, "a ZRL with no coefficient behind it"
    return items


class PackError(AssertionError):
    pass


def block_range(hist):
    """(fewest, most) blocks that can hold the histogram: hist[EOB] blocks end before position 63, every other block ON it"""
    p = sum((r + 1) for r, _ in _items(hist, np.random.default_rng(0)))
    e = hist.get(EOB, 0)
    return e + -(-max(0, p - 62 * e) // 63), e + p // 63


def pack(hist, nblocks, seed, small_first=False):
    """[nblocks][64] coefficients (DC small and random) whose AC histogram is `hist`.  small_first: the coefficients of size 1 of a
    block in front of the others, so that a refinement scan at Al = 0 codes them with the runs they have here (a coefficient coded
    earlier does not end a run there: its zeros would be added to the next one's)"""
    rng = np.random.default_rng(seed)
    by_len = {}
    for it in _items(hist, rng):
        by_len.setdefault(it[0] + 1, []).append(it)
    e = hist.get(EOB, 0)
    assert 0 <= e <= nblocks, "%d blocks for %d EOB" % (nblocks, e)

    def fill(rem, longest, out):
        for l in range(min(rem, longest), 0, -1):
            if by_len.get(l):
                out.append(by_len[l].pop())
                if rem == l or fill(rem - l, l, out):
                    return True
                by_len[l].append(out.pop())
        return False

    bins = []
    for _ in range(nblocks - e):                           # the blocks that end on position 63
        out = []
        if not fill(63, 63, out):
            raise PackError("the histogram does not fill %d blocks" % (nblocks - e))
        bins.append(out)
    short, room = [[] for _ in range(e)], [62] * e
    for l in sorted(by_len, reverse=True):
        for it in by_len[l]:
            k = next((k for k in range(e) if room[k] >= l), None)
            if k is None:
                raise PackError("the histogram does not fit %d blocks" % nblocks)
            short[k].append(it)
            room[k] -= l
    bins += short
    a = np.zeros((nblocks, 64), np.int64)
    a[:, 0] = rng.integers(-20, 21, nblocks)
    for b, i in enumerate(rng.permutation(nblocks)):
        pos = 0
        order = rng.permutation(len(bins[i]))
        if small_first:
            order = sorted(order, key=lambda j: bins[i][j][1] != 1)
        for j in order:
            run, size = bins[i][j]
            pos += run + 1
            a[b, pos] = int(rng.integers(1 << (size - 1), 1 << size)) * (1 if rng.random() < 0.5 else -1)
    return a


AC_SYMBOLS = [EOB, ZRL] + [(r << 4) + s for r in range(16) for s in range(1, 11)]
FIB = [1, 2]
while len(FIB) < 24:
    FIB.append(FIB[-1] + FIB[-2])


def chain_hist(nsym, nblocks):
    """a Fibonacci chain of nsym symbols that fills nblocks blocks to position 63: 1, 2, 3, 5, ... for run 5..0 with size 2 (the last
    nsym - 16 of them), then for run 15..1 with size 1; run 0 / size 1 takes every position that is left and must be the largest count"""
    syms = [(r << 4) + 2 for r in range(5, -1, -1)][22 - nsym:] + [(r << 4) + 1 for r in range(15, 0, -1)]
    assert len(syms) == nsym - 1
    hist = {s: FIB[k] for k, s in enumerate(syms)}
    hist[0x01] = 63 * nblocks - sum(c * ((s >> 4) + 1) for s, c in hist.items())
    assert hist[0x01] >= FIB[nsym - 1], "%d blocks are too few" % nblocks
    return hist


def uniform_hist(count):
    return {s: count for s in AC_SYMBOLS}


def ties_hist(seed, nsym):
    rng = np.random.default_rng(seed)
    syms = [EOB] + [AC_SYMBOLS[i] for i in 1 + rng.choice(len(AC_SYMBOLS) - 1, nsym - 1, replace=False)]
    return {s: int(c) for s, c in zip(syms, rng.integers(1, 3, nsym))}


def pow2_hist(seed, nsym):
    """counts 1, 2, 4, ... over nsym symbols in an order drawn from the seed: EOB (256 at the most: one per block that ends early),
    a run-0 symbol with the largest count (it fills the blocks that end on position 63 to the last position) and nsym - 2 others"""
    rng = np.random.default_rng(seed)
    unit = int(rng.integers(1, 11))
    rest = [s for s in AC_SYMBOLS[2:] if s != unit]
    syms = [rest[i] for i in rng.choice(len(rest), nsym - 2, replace=False)]
    e = int(rng.integers(0, min(nsym - 1, 9)))
    hist = {s: 1 << int(k) for s, k in zip(syms, rng.permutation([k for k in range(nsym - 1) if k != e]))}
    hist[EOB], hist[unit] = 1 << e, 1 << (nsym - 1)
    if nsym == 2 and seed & 1:                             # (two symbols: either order)
        hist[EOB], hist[unit] = 2, 1
    return hist


def single_hist(sym, nblocks):
    assert 63 % ((sym >> 4) + 1) == 0
    return {sym: nblocks * 63 // ((sym >> 4) + 1)}


def two_hist(nblocks):
    return {0x01: 21 * nblocks, 0x11: 21 * nblocks}          # 21 + 2 * 21 positions a block


def small_hist(nblocks):
    """chroma of the 4:2:0 chain files: any small histogram"""
    return {0x01: 20 * nblocks, 0x32: 5 * nblocks, EOB: nblocks}


class ACase:
    """one family A file: .c (a stream_cases.Case), .hists = {output AC table: the dictated histogram}, .comp_table = table per component"""
    def __init__(self, name, c, hists, shape):
        self.name, self.c, self.hists, self.shape = name, c, hists, shape
        self.comp_table = [0, 1, 1][:len(c.comps)]


def _grid(nblocks):
    """(block rows, block columns) of nblocks blocks, as square as the number allows"""
    rows = max(r for r in range(1, int(nblocks ** 0.5) + 1) if nblocks % r == 0)
    return rows, nblocks // rows


def _file(name, seed, layout, blocks, hists, shape):
    """blocks: per component [n][64] in raster order"""
    if layout == "gray":
        comps = SC.gray()
        rows, cols = blocks[0][1]
        coefs = [blocks[0][0].reshape(rows, cols, 64)]
        w, h = 8 * cols, 8 * rows
    else:
        comps = SC.ycc(*SC.S420)
        my, mx = blocks[1][1]
        coefs = [blocks[0][0].reshape(2 * my, 2 * mx, 64), blocks[1][0].reshape(my, mx, 64), blocks[2][0].reshape(my, mx, 64)]
        w, h = 16 * mx, 16 * my
    c = SC.build(seed, w, h, comps, coefs=coefs, qtables={t: UNIT_Q[t] for t in set(x[3] for x in comps)}, scans=SC.one_scan(len(comps), shape),
                 edges=False, transforms=())
    return ACase(name, c, hists, shape)


def make_a(name, layout, seed, shape, luma, chroma=None, nblocks=None, small_first=False):
    """luma / chroma: callables (try number) -> histogram, or (number of blocks) -> histogram where nblocks fixes the grid.
    gray: `luma` alone.  4:2:0: luma over 4 m blocks, chroma over the 2 m blocks of Cb and Cr together (one output table)."""
    if layout == "gray":
        if nblocks is not None:
            hist, n = luma(nblocks), nblocks
            return _file(name, seed, layout, [(pack(hist, n, seed, small_first), _grid(n))], {0: hist}, shape)
        for t in range(20):
            hist = luma(t)
            n = block_range(hist)[0]
            try:
                return _file(name, seed, layout, [(pack(hist, n, seed), _grid(n))], {0: hist}, shape)
            except PackError:
                continue
        raise AssertionError("no grid holds a histogram of %s" % name)
    if nblocks is not None:
        m = nblocks
        hl, hc = luma(4 * m), chroma(2 * m)
    else:
        found = None
        for t in range(400):
            hl, hc = luma(t // 20), chroma(t % 20)
            (l0, l1), (c0, c1) = block_range(hl), block_range(hc)
            ms = [m for m in range(1, 800) if l0 <= 4 * m <= l1 and c0 <= 2 * m <= c1]
            if ms:
                try:
                    m = ms[0]
                    found = pack(hl, 4 * m, seed), pack(hc, 2 * m, seed + 1)
                    break
                except PackError:
                    continue
        assert found, "no 4:2:0 grid holds the histograms of %s" % name
        yblocks, both = found
        return _file(name, seed, layout, [(yblocks, None), (both[:m], _grid(m)), (both[m:], None)], {0: hl, 1: hc}, shape)
    both = pack(hc, 2 * m, seed + 1)                       # Cb takes the first m blocks and Cr the rest: the sum is dictated
    return _file(name, seed, layout, [(pack(hl, 4 * m, seed, small_first), None), (both[:m], _grid(m)), (both[m:], None)], {0: hl, 1: hc}, shape)


CHAIN_MIN_GRAY = 289        # 136 x 136
A_MAKERS = {}


def _a(name, **kw):
    for layout in ("gray", "420"):
        args = dict(kw)
        if layout == "420":
            args.update(args.pop("kw420", {}))
        else:
            args.pop("kw420", None)
            args.pop("chroma", None)
        A_MAKERS["%s-%s" % (name, layout)] = functools.partial(make_a, "%s-%s" % (name, layout), layout, **args)


# 4:2:0 chain files: the chain on the luma table (4 m blocks), chroma small
_a("chain_22", seed=7000, shape="all9", luma=lambda n: chain_hist(22, n), chroma=small_hist, nblocks=56 * 56, small_first=True,
   kw420=dict(nblocks=28 * 28))
_a("chain_min", seed=7010, shape="optimal", luma=lambda n: chain_hist(17, n), chroma=small_hist, nblocks=CHAIN_MIN_GRAY, small_first=True,
   kw420=dict(nblocks=72))
_a("uniform_162", seed=7020, shape="all9", luma=lambda t: uniform_hist(4), chroma=lambda t: uniform_hist(2))
_a("ties_12", seed=7030, shape="optimal", luma=lambda t: ties_hist(7030 + t, 12), chroma=lambda t: ties_hist(7060 + t, 12),
   kw420=dict(luma=lambda t: ties_hist(7030 + t, 24)))
for _n in range(2, 14):
    _a("pow2_%d" % _n, seed=7100 + 10 * _n, shape=("all9", "optimal")[_n & 1], luma=lambda t, n=_n: pow2_hist(7100 + 10 * n + t, n),
       chroma=lambda t, n=_n: pow2_hist(7400 + 20 * n + t, n), kw420=dict(luma=lambda t, n=_n: pow2_hist(7100 + 20 * n + t, max(n + 1, 4))))
_a("single", seed=7300, shape="all9", luma=lambda n: single_hist(0x62, n), chroma=lambda n: single_hist(0x23, n), nblocks=6, kw420=dict(nblocks=2))
_a("two", seed=7310, shape="optimal", luma=two_hist, chroma=two_hist, nblocks=6, kw420=dict(nblocks=2))
A_NAMES = list(A_MAKERS)
A_PAIRS = [(n, sw) for n in A_NAMES for sw in A_CODINGS]


@functools.lru_cache(maxsize=None)
def a_case(name):
    return A_MAKERS[name]()


def _pow2_for(nblocks):
    """a powers-of-two histogram that nblocks blocks hold"""
    for n in range(13, 1, -1):
        for t in range(200):
            h = pow2_hist(7800 + t, n)
            lo, hi = block_range(h)
            if lo <= nblocks <= hi:
                return h
    raise AssertionError("no powers-of-two histogram for %d blocks" % nblocks)


@functools.lru_cache(maxsize=None)
def batch_cases():
    """four gray files of chain_min's size: chain_min, uniform_162, single and pow2 content"""
    n = CHAIN_MIN_GRAY
    count = next(k for k in range(1, 100) if block_range(uniform_hist(k))[0] <= n <= block_range(uniform_hist(k))[1])
    return [a_case("chain_min-gray"),
            make_a("batch_uniform", "gray", 7500, "all9", lambda k: uniform_hist(count), nblocks=n),
            make_a("batch_single", "gray", 7501, "optimal", lambda k: single_hist(0x62, k), nblocks=n),
            make_a("batch_pow2", "gray", 7502, "all9", _pow2_for, nblocks=n)]


BATCH_CODINGS = ("revert_opt", "revert_progressive")


def component_blocks(c, ci):
    """the blocks of a non-interleaved scan of component ci in coding order"""
    rows, cols = W.real_blocks(c.width, c.height, c.comps, ci)
    return c.coefs[ci][:rows, :cols].reshape(-1, 64)


def counted(ac):
    """{output AC table: histogram counted from the arrays the file was written from} (every block of an interleaved scan)"""
    out = {}
    for ci, t in enumerate(ac.comp_table):
        out[t] = out.get(t, 0) + ac_histogram(ac.c.coefs[ci])
    return out


def dictated(hist):
    a = np.zeros(256, np.int64)
    for s, c in hist.items():
        a[s] = c
    return a


def ac_tables(ref):
    """[(scan header, bits, huffval)] of every progressive AC scan of the file"""
    return [(s,) + s["dht"][(1, s["tables"][0][1])] for s in scan_headers(ref) if s["Ss"] > 0]


def check_restatement_on_scan(ac, s, bits, vals):
    """the restated table of the symbols the restated walk counts in this progressive AC scan is the table the reference wrote in
    front of it; returns gen_optimal_table's answer"""
    ids = [x[0] for x in ac.c.comps]
    hist = ac_scan_walk(component_blocks(ac.c, ids.index(s["comps"][0])), s["Ss"], s["Se"], s["Ah"], s["Al"], s["ri"])["hist"]
    got = gen_optimal_table(hist)
    assert (got[2], got[3]) == (bits, vals), "the restated table of scan %s differs from the reference's DHT" % (
        (s["comps"], s["Ss"], s["Se"], s["Ah"], s["Al"]),)
    return got


def check_a_premise(M, name):
    ac = a_case(name)
    c = ac.c
    # 1. the histogram of the file is the dictated one
    have = counted(ac)
    for t, hist in ac.hists.items():
        assert np.array_equal(have[t], dictated(hist)), "table %d: the file's histogram is not the dictated one" % t
    run_quiet("jpegtran", ["-copy", "none"], c.data, ".jpg")
    run_quiet("djpeg", ["-pnm"], c.data, ".jpg")
    # 2. the sequential coding: the restated tables are the reference's, and the property the case is named for
    ref = ref_jpegtran(c.data, "revert_opt")
    scans = scan_headers(ref)
    assert len(scans) == 1 and scans[0]["Se"] == 63
    res = {}
    for t, hist in ac.hists.items():
        res[t] = gen_optimal_table(dictated(hist))
        assert (res[t][2], res[t][3]) == scans[0]["dht"][(1, t)], "table %d: the restated table differs from the reference's DHT" % t
    longest, moves, bits, vals = res[0]
    kind = name.split("-")[0]
    if kind == "chain_22":
        assert longest >= 20 and moves >= 5, "longest %d, %d moves" % (longest, moves)
    elif kind == "chain_min":
        assert (longest, moves) == (17, 1), "longest %d, %d moves" % (longest, moves)
    elif kind == "uniform_162":
        assert all(len(scans[0]["dht"][(1, t)][1]) == 162 for t in ac.hists) and len(set(ac.hists[0].values())) == 1
    elif kind == "ties_12":
        assert all(set(h.values()) <= {1, 2} and len(h) >= 12 for h in ac.hists.values())
    elif kind.startswith("pow2"):
        n = int(kind.split("_")[1])
        last = max(ac.hists)
        assert sorted(ac.hists[last].values()) == [1 << k for k in range(n)]
    elif kind == "single":
        assert all(scans[0]["dht"][(1, t)][0] == [0, 1] + [0] * 15 for t in ac.hists)
    elif kind == "two":
        assert all(len(set(h.values())) == 1 and len(h) == 2 for h in ac.hists.values())
    # 3. the progressive codings: the restated walk and table builder give the reference's DHT for every AC scan
    for sw in PROGRESSIVE:
        ref = ref_jpegtran(c.data, sw)
        limited = 0
        for s, bits, vals in ac_tables(ref):
            got = check_restatement_on_scan(ac, s, bits, vals)
            if bits[16] >= 2 and got[1] >= 1:
                limited += 1
        if kind == "chain_22":
            assert limited >= 1, "%s: no AC table of the reference's file went through the length limit" % sw
    return res


def transcode(M, data, sw, max_batch=1):
    kw = CODINGS[sw][0]
    if sw == "default":                                    # through recompress(): the smaller of source and result, as jpegtran
        out = M.recompress([data], max_batch=max_batch, **kw)[0]
        if isinstance(out, Exception):
            raise out
        return out
    enc = M.Encoder(M.params_from_jpeg(data, **kw), max_batch=max_batch)
    try:
        return enc.transcode_host([data])[0]
    finally:
        enc.close()


def check_transcode(M, c, sw):
    ref = ref_jpegtran(c.data, sw)
    out = transcode(M, c.data, sw)
    assert out == ref, first_difference(out, ref)


def check_batch(M, sw):
    cases = batch_cases()
    files = [x.c.data for x in cases]
    tables = [scan_headers(ref_jpegtran(f, "revert_opt"))[0]["dht"][(1, 0)] for f in files]
    assert len(set(str(t) for t in tables)) == 4, "the four files do not have four tables"
    enc = M.Encoder(M.params_from_jpeg(files[0], **CODINGS[sw][0]), max_batch=4)
    try:
        outs = enc.transcode_host(files)
    finally:
        enc.close()
    for k, f in enumerate(files):
        ref = ref_jpegtran(f, sw)
        assert outs[k] == ref, "file %d (%s): %s" % (k, cases[k].name, first_difference(outs[k], ref))


# ---- family B: one-row 16-bit lossless images from a dictated category histogram ------------------------------------------------------
FIB17 = FIB[:17]
assert sum(FIB17) == 6763 and FIB17[-1] == 2584
PERM17 = [int(v) for v in np.random.default_rng(17).permutation(17)]
B_COUNTS = {
    "fib_up": FIB17,
    "fib_down": FIB17[::-1],
    "fib_perm": [FIB17[PERM17[k]] for k in range(17)],
    "uniform17": [3] * 17,
    "lone16": [0] * 16 + [5],
}
B_CASES = {n: (n,) for n in B_COUNTS}
B_CASES["rgb_fib"] = ("fib_up", "fib_down", "fib_perm")
B_NAMES = list(B_CASES)


def category_row(counts, seed):
    """16-bit samples of one row whose differences from the left neighbour (the first one from 32768), modulo 65536, hold counts[c]
    values of category c, in an order drawn from the seed; category 16 is the difference 32768"""
    rng = np.random.default_rng(seed)
    cats = rng.permutation(np.repeat(np.arange(17), counts))
    mag = np.array([0 if c == 0 else 32768 if c == 16 else int(rng.integers(1 << (c - 1), 1 << c)) for c in cats], np.int64)
    diff = np.where((cats < 16) & (rng.random(len(cats)) < 0.5), -mag, mag)
    return ((32768 + np.cumsum(diff)) & 0xFFFF).astype(np.uint16)


def category_counts(row):
    """the categories of a row's differences (PSV 1, Pt 0, 16 bits), counted the plain way"""
    out, prev = [0] * 17, 32768
    for v in row:
        d = (int(v) - prev) & 0xFFFF
        if d & 0x8000 and d != 0x8000:
            d = 0x10000 - d
        out[d.bit_length()] += 1
        prev = int(v)
    return out


@functools.lru_cache(maxsize=None)
def b_case(name):
    """(image [1][W][components], dictated counts per component)"""
    parts = B_CASES[name]
    rows = [category_row(B_COUNTS[p], 8000 + 10 * B_NAMES.index(name) + k) for k, p in enumerate(parts)]
    return np.stack(rows, axis=-1)[None].copy(), [B_COUNTS[p] for p in parts]


@functools.lru_cache(maxsize=None)
def b_reference(name):
    a, _ = b_case(name)
    ref = LC.reference(a, 1, 0, 16)
    assert isinstance(ref, bytes), "the reference's cjpeg refuses: %r" % (ref,)
    return ref


def check_b_premise(M, name):
    a, counts = b_case(name)
    for k, want in enumerate(counts):
        assert category_counts(a[0, :, k]) == list(want), "component %d: the row's histogram is not the dictated one" % k
    with tempfile.TemporaryDirectory() as td:
        f = os.path.join(td, "in.pnm")
        LC.write_pnm(f, a, 16)
        with open(f, "rb") as fh:
            run_quiet("cjpeg", LC.cjpeg_args(1, 0, 16), fh.read(), ".pnm")
    scans = scan_headers(b_reference(name))
    assert len(scans) == 1 and all(t[0] == 0 for t in scans[0]["tables"]), "one scan, one table for every component"
    bits, vals = scans[0]["dht"][(0, 0)]
    total = [sum(c[k] for c in counts) for k in range(17)]
    longest, moves, rbits, rvals = gen_optimal_table(total)
    assert (rbits, rvals) == (bits, vals), "the restated table differs from the reference's DHT"
    if name.startswith("fib"):
        assert bits[1:] == [1] * 14 + [0, 3] and moves >= 1, "bits %s, %d moves" % (bits[1:], moves)
    elif name == "rgb_fib":
        assert len(vals) == 17 and a.shape[2] == 3
    elif name == "uniform17":
        assert len(vals) == 17
    elif name == "lone16":
        assert bits[1:] == [1] + [0] * 15 and vals == [16]
    return longest, moves, bits


def check_b_encode(M, name):
    a, _ = b_case(name)
    ref = b_reference(name)
    enc = M.Encoder(LC.params(M, a, 1, 0, 16), max_batch=1)
    try:
        out = enc.encode_host(a)[0]
    finally:
        enc.close()
    assert out == ref, first_difference(out, ref)


# ---- family C: 63 correction bits a block ------------------------------------------------------------------------------------------------
C_SHAPES = {"gray_128x64": (128, 64, "gray"), "gray_40x200": (40, 200, "gray"), "420_257x33": (257, 33, "420")}
C_VARIANTS = ("dense", "mixed", "tail")
C_NAMES = ["%s-%s" % (s, v) for s in C_SHAPES for v in C_VARIANTS]


def c_codings(name):
    shape, variant = name.split("-")
    if variant == "tail":
        return ("revert_progressive", "fastcrush_progressive", "default")
    return ("revert_progressive", "fastcrush_progressive", "default", "revert_progressive_restart4" if shape == "gray_40x200" else "revert_progressive_restart1")


C_PAIRS = [(n, sw) for n in C_NAMES for sw in c_codings(n)]


@functools.lru_cache(maxsize=None)
def c_case(name):
    shape, variant = name.split("-")
    w, h, layout = C_SHAPES[shape]
    comps = SC.gray() if layout == "gray" else SC.ycc(*SC.S420)
    seed = 9000 + 10 * list(C_SHAPES).index(shape) + C_VARIANTS.index(variant)
    rng = np.random.default_rng(seed)
    coefs = []
    for ci in range(len(comps)):
        rows, cols = W.padded_blocks(w, h, comps, ci)
        n = rows * cols
        a = rng.integers(4, 40, (n, 64)) * rng.choice([-1, 1], (n, 64))
        a[:, 0] = rng.integers(-100, 101, n)
        if variant == "mixed":
            for b in rng.choice(n, max(1, round(0.06 * n)), replace=False):     # one coefficient that a later scan codes as newly non-zero
                a[b, int(rng.integers(1, 64))] = int(rng.integers(1, 4)) * (1 if rng.random() < 0.5 else -1)
            for b in rng.choice(n, max(1, round(0.04 * n)), replace=False):     # a block cut short with zeros
                a[b, int(rng.integers(1, 64)):] = 0
        if variant == "tail":
            a[n // 4:, 32:] = rng.choice([-1, 1], (n - n // 4, 32))
        coefs.append(a.reshape(rows, cols, 64))
    return SC.build(seed, w, h, comps, coefs=coefs, qtables={t: UNIT_Q[t] for t in set(x[3] for x in comps)}, edges=False, transforms=())


def check_c_premise(M, name):
    c = c_case(name)
    shape, variant = name.split("-")
    a = np.concatenate([x.reshape(-1, 64) for x in c.coefs])[:, 1:]
    mag = np.abs(a)
    if variant == "dense":
        assert mag.min() >= 4 and mag.max() <= 39
    elif variant == "tail":
        for x in c.coefs:
            m = np.abs(x.reshape(-1, 64))
            q = len(m) // 4
            assert m[:q, 1:].min() >= 4 and m[q:, 1:32].min() >= 4 and (m[q:, 32:] == 1).all() and m.max() <= 100
    else:
        small = ((mag >= 1) & (mag <= 3)).sum(axis=1)
        cut = (mag == 0).any(axis=1)
        assert small.max() == 1 and 0.02 < small.mean() <= 0.07 and 0.03 <= cut.mean() <= 0.05 and mag.max() <= 39
        assert all((row[np.argmax(row == 0):] == 0).all() for row in mag[cut]), "zeros that are not the end of a block"
    run_quiet("jpegtran", ["-copy", "none"], c.data, ".jpg")
    run_quiet("djpeg", ["-pnm"], c.data, ".jpg")
    ids = [x[0] for x in c.comps]
    found = {}
    for sw in c_codings(name):
        be = 0
        ref = ref_jpegtran(c.data, sw)
        if sw == "default" and variant != "tail":          # (see the module's docstring)
            assert ref == c.data or not any(s["Ah"] for s in scan_headers(ref)), "the scan search chose a refinement scan: assert its flushes here"
            continue
        for s in scan_headers(ref):
            if s["Ss"] == 0 or s["Ah"] == 0:
                continue
            assert (s["ri"] > 0) == ("restart" in sw)
            r = ac_scan_walk(component_blocks(c, ids.index(s["comps"][0])), s["Ss"], s["Se"], s["Ah"], s["Al"], s["ri"])
            assert r["run"] == 0, "%s: a flush forced by EOBRUN == 0x7FFF" % sw
            be += r["be"] - r["be_last"] > 0              # (one behind an interval's last block writes what the restart would write)
        assert be >= 1, "%s: no AC refinement scan of the reference's file has a flush forced by BE > 937 inside an interval" % sw
        found[sw] = be
    return found
