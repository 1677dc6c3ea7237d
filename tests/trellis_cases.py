"""The case list and helpers of the AC trellis pins (test_simt_trellis_pins.py on the emulator, test_gpu_trellis_pins.py on the chip):
gray images, 8 rows high, built from DICTATED 8x8 blocks whose raw coefficients make a named branch of the dynamic programme of
mjh_trellis.hip run -- the tie rule, candidates without a Huffman code, forbidden runs, the pruning of the predecessor scan, the
tier edges, the end-of-block choice -- next to filler blocks, and wave / tile shapes of dictated key patterns.

Every expected byte comes from the C restatement (oracle_lib.encode) and, where it is built and the case is expressible in its
switches, from the real reference; equality is exact.  Every dictated block proves its premise from `restate_block`, a restatement of
the AC part of quantize_trellis (jcdctmgr.c:1120-1222, with norm / lambda / lambda_tbl of :1011-1037) in numpy.float32 scalars, one
operation per rounding, that RECORDS the events of the programme; the code lengths it prices with are restated too (histogram of the
coefficients in front of the pass -> hist_cases.gen_optimal_table), never read from the product.  The restatement itself is checked:
for every dictated block it must give the oracle's coef_q tap.

Blocks come from spec tuples (spec_block): pixel blocks whose FDCT gives the wanted multiples of the quantizer step (as basis_block of
test_gpu_fdct_fused_stats.py), drawn with a seed where the event cannot be hit by construction; `search` over the gen_* functions is what the
committed seeds (FOUND_SEEDS) were found with; no test runs it.  What the taps say was actually obtained is what the premises judge."""
import functools
import math
import os

import numpy as np

import oracle_lib as O
import hist_cases as HC

F = np.float32
ZZ = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
               28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
               54, 47, 55, 62, 63])     # natural index of zig-zag position k
BIG = F(1e38)


# ---- restatement: code lengths of a trellis pass ------------------------------------------------------------------------------------
def code_lengths(hist):
    """size[256] of the optimal table of these counts (jpeg_gen_optimal_table + jpeg_make_c_derived_tbl: lengths in huffval order)"""
    _, _, bits, huffval = HC.gen_optimal_table(hist)
    size, p = [0] * 256, 0
    for l in range(1, 17):
        for _ in range(bits[l]):
            size[huffval[p]] = l
            p += 1
    return size


def pass_lengths(blocks_zz, progressive=False):
    """code lengths of the AC table a 1..63 trellis pass prices with: the optimal table of the component's coefficients as they stand
    in front of the pass ([n][64] zig-zag).  Sequential: the plain (run, size) histogram (jchuff.c htest_one_block).  Progressive: every
    symbol 16 i + j, j < 12, starts at a count of 1 (jcphuff.c:257-264) and the blocks are walked as an AC-first scan with its
    end-of-band runs."""
    if progressive:
        hist = [0] * 256
        for i in range(16):
            for j in range(12):
                hist[16 * i + j] = 1
        walk = HC.ac_scan_walk([list(map(int, b)) for b in blocks_zz], 1, 63, 0, 0)["hist"]
        hist = [a + b for a, b in zip(hist, walk)]
    else:
        hist = HC.ac_histogram(blocks_zz)
    return code_lengths(hist)


# ---- restatement: the AC dynamic programme of one block, with its events ------------------------------------------------------------
def block_lambda(src, lambda1, lambda2):
    """norm and lambda of one block (jcdctmgr.c:1027-1037): src in natural order"""
    norm = F(0.0)
    for i in range(1, 64):
        norm = norm + F(int(src[i]) * int(src[i]))
    norm = F(float(norm) / 63.0)
    l1, l2 = float(F(lambda1)), float(F(lambda2))
    if l2 > 0.0:
        return F(math.pow(2.0, l1) * 1.0 / (math.pow(2.0, l2) + float(norm)))
    return F(math.pow(2.0, l1 - 12.0) * 1.0)


def _cost(rate, dist, azd_prev, azd_j, acost_j):
    cost = F(rate) + dist
    rhs = azd_prev - azd_j
    rhs = rhs + acost_j
    return cost + rhs


def restate_block(src, coef_in, qt, size, lambda1, lambda2, Ss=1, Se=63):
    """src: the block's raw coefficients, coef_in: its quantized coefficients in front of the pass (what a position none of whose
    candidates has a code keeps), qt: the quantization table -- all three in natural order; size: code lengths of the pass's AC table.
    Returns (the block behind the pass, natural order, positions outside Ss..Se as in coef_in; events)."""
    src = [int(v) for v in src]
    coef = [int(v) for v in coef_in]
    before = list(coef)
    lt = [F(1.0 / float(int(q) * int(q))) for q in qt]
    lam = block_lambda(src, lambda1, lambda2)
    azd, acost, run_start = [F(0.0)] * 64, [F(0.0)] * 64, [0] * 64
    ev = dict(nrec=0, maxq=0, clamped=False, tie_pred=[], tie_cand=[], no_code=[], dead_position=[], zrl_forbidden=[], far_pred=[],
              no_code_cheaper=[], zrl_forbidden_cheaper=[],
              start_pred=[], near_pred_all=True, last_at_se=False, band_zeroed=False, eob_tie=False, eob_no_code=size[0] == 0)
    skipped = {}        # position -> live positions between it and its chosen predecessor
    for i in range(Ss, Se + 1):
        z = int(ZZ[i])
        sign = -1 if src[z] < 0 else 0
        x = abs(src[z])
        q = 8 * int(qt[z])
        t = F(x * x) * lam
        t = t * lt[z]
        azd[i] = t + azd[i - 1]
        qval = (x + q // 2) // q
        if qval == 0:
            coef[z] = 0
            acost[i] = BIG
            continue
        ev["nrec"] += 1
        if qval >= 1024:
            qval = 1023
            ev["clamped"] = True
        ev["maxq"] = max(ev["maxq"], qval)
        ncd = qval.bit_length()
        cand, cdist = [], []
        for k in range(ncd):
            c = (2 << k) - 1 if k < ncd - 1 else qval
            delta = c * q - x
            t = F(delta * delta) * lam
            cand.append(c)
            cdist.append(t * lt[z])
        acost[i] = BIG
        ghost = []          # (event, cost) of what the rules about missing codes keep out
        tried = []          # (predecessor, candidate, cost) in the reference's order
        bestj = bestk = -1
        for j in range(Ss - 1, i):
            if j != Ss - 1 and coef[int(ZZ[j])] == 0:
                continue
            zero_run = i - 1 - j
            if (zero_run >> 4) and size[0xF0] == 0:
                ev["zrl_forbidden"].append(i)
                # what the predecessor would cost if the missing ZRL were free: does forbidding it change the choice?
                for k in range(ncd):
                    if size[16 * (zero_run & 15) + k + 1]:
                        ghost.append(("zrl_forbidden_cheaper", _cost(size[16 * (zero_run & 15) + k + 1] + k + 1, cdist[k], azd[i - 1], azd[j], acost[j])))
                continue
            run_bits = (zero_run >> 4) * size[0xF0]
            zero_run &= 15
            for k in range(ncd):
                coef_bits = size[16 * zero_run + k + 1]
                if coef_bits == 0:
                    ev["no_code"].append(i)
                    # what the candidate would cost if a missing code were a code of length 0
                    ghost.append(("no_code_cheaper", _cost(k + 1 + run_bits, cdist[k], azd[i - 1], azd[j], acost[j])))
                    continue
                rate = coef_bits + (k + 1) + run_bits
                cost = F(rate) + cdist[k]
                rhs = azd[i - 1] - azd[j]
                rhs = rhs + acost[j]
                cost = cost + rhs
                tried.append((j, k, cost))
                if cost < acost[i]:
                    coef[z] = (cand[k] ^ sign) - sign
                    acost[i] = cost
                    run_start[i] = j
                    bestj, bestk = j, k
        for name, cost in ghost:
            if cost < acost[i]:
                ev[name].append(i)
        if bestj < 0:
            ev["dead_position"].append(i)
            continue
        for j, k, cost in tried:
            if cost == acost[i] and (j, k) != (bestj, bestk):
                ev["tie_pred" if j != bestj else "tie_cand"].append(i)
        between = [p for p in range(bestj + 1, i) if coef[int(ZZ[p])] != 0 and acost[p] < BIG]
        skipped[i] = len(between)
        if between:
            ev["near_pred_all"] = False
    # the end-of-block choice (:1187-1207)
    last = Ss - 1
    best_cost = azd[Se] + F(size[0])
    best_skip = azd[Se]
    ends = [(Ss - 1, best_cost)]
    for i in range(Ss, Se + 1):
        if coef[int(ZZ[i])] != 0:
            cost = acost[i] + azd[Se]
            cost = cost - azd[i]
            wo_eob = cost
            if i < Se:
                cost = cost + F(size[0])
            ends.append((i, cost))
            if cost < best_cost:
                best_cost, last, best_skip = cost, i, wo_eob
    # what trellis_eob_opt carries from the block into its row's chain (:1187-1209)
    ev["cost_all_zeros"], ev["best_cost_skip"], ev["has_eob"] = azd[Se], best_skip, int(last < Se) + int(last == Ss - 1)
    ev["eob_tie"] = any(c == best_cost and i != last for i, c in ends)
    ev["last_at_se"] = last == Se
    ev["front"] = [i for i in range(Ss, Se + 1) if before[int(ZZ[i])] != 0]
    ev["band_zeroed"] = last == Ss - 1 and len(ev["front"]) > 0
    # back-track (:1211-1222)
    path = []
    i = Se
    while i >= Ss:
        while i > last:
            coef[int(ZZ[i])] = 0
            i -= 1
        if i < Ss:
            break
        path.append(i)
        last = run_start[i]
        i -= 1
    # what only counts where the decision reaches the file: ties and skipped predecessors of the positions on the chosen path
    ev["no_code_cheaper"] = sorted(set(ev["no_code_cheaper"]) & set(path))
    ev["zrl_forbidden_cheaper"] = sorted(set(ev["zrl_forbidden_cheaper"]) & set(path))
    ev["tie_pred"] = sorted(set(ev["tie_pred"]) & set(path))
    ev["tie_cand"] = sorted(set(ev["tie_cand"]) & set(path))
    ev["far_pred"] = sorted(p for p in path if skipped[p] >= 8 and run_start[p] != Ss - 1)
    ev["start_pred"] = sorted(p for p in path if skipped[p] >= 8 and run_start[p] == Ss - 1)
    for k in ("no_code", "dead_position", "zrl_forbidden"):
        ev[k] = sorted(set(ev[k]))
    ev["path"] = sorted(path)
    ev["gaps"] = [b - a - 1 for a, b in zip([Ss - 1] + sorted(path), sorted(path))]
    ev["ndiff"] = sum(1 for i in range(Ss, Se + 1) if coef[int(ZZ[i])] != before[int(ZZ[i])])
    return coef, ev


def restate_eob_chain(info, size, Ss=1, Se=63):
    """trellis_eob_opt over one block row (jcdctmgr.c:1224-1297): info = (cost_all_zeros, best_cost_skip, has_eob) of every block in
    order.  Returns (blocks whose band is zeroed, blocks at which a LATER run start equals the best cost and loses; -1 = in the choice
    of the last run).  A block whose last coefficient sits at Se never enters the recursion; its run start is not restated (callers
    assert that the row has none)."""
    n = len(info)
    azbc, abc, req, start, ties = [F(0.0)] * (n + 1), [F(0.0)] * (n + 1), [0] * (n + 1), [0] * n, []
    for bi, (caz, skip, has) in enumerate(info):
        azbc[bi + 1] = azbc[bi] + caz
        req[bi + 1] = has
        best = BIG
        if has != 2:
            for i in range(bi + 1):
                if req[i] == 2:
                    continue
                cost = skip + azbc[bi]
                cost = cost - azbc[i]
                cost = cost + abc[i]
                nb = (bi - i + req[i]).bit_length()
                cost = cost + F(size[16 * nb] + nb)
                if cost < best:
                    start[bi], best, abc[bi + 1] = i, cost, cost
                    tied = False
                elif cost == best:
                    tied = True
            if tied:
                ties.append(bi)
    best, last_block, tied = BIG, n, False
    for i in range(n + 1):
        if req[i] == 2:
            continue
        cost = F(0.0) + azbc[n]
        cost = cost - azbc[i]
        nb = (n - i + req[i]).bit_length()
        cost = cost + F(size[16 * nb] + nb)
        if cost < best:
            best, last_block, tied = cost, i, False
        elif cost == best:
            tied = True
    if tied:
        ties.append(-1)
    zeroed, chosen = [], []
    last_block -= 1
    bi = n - 1
    while bi >= 0:
        while bi > last_block:
            zeroed.append(bi)
            bi -= 1
        if bi < 0:
            break
        chosen.append(bi)
        last_block = start[bi] - 1
        bi -= 1
    return sorted(zeroed), [t for t in ties if t == -1 or t in chosen]


def tokens(ev):
    """the events of one block as {token: where it happens} (the `where` tells two blocks that show the same event apart)"""
    t = {"nrec=%d" % ev["nrec"]: tuple(ev["path"]), "maxq=%d" % ev["maxq"]: tuple(ev["path"])}
    for k in ("tie_pred", "tie_cand", "no_code", "dead_position", "zrl_forbidden", "far_pred", "start_pred", "no_code_cheaper",
              "zrl_forbidden_cheaper"):
        if ev[k]:
            t[k] = tuple(ev[k])
    for k in ("clamped", "last_at_se", "band_zeroed", "eob_tie", "eob_no_code"):
        if ev[k]:
            t[k] = tuple(ev["front"] if k == "band_zeroed" else ev["path"])
    if ev["nrec"] <= 16 and ev["maxq"] < 16:
        t["first_tier_16"] = tuple(ev["path"])
    if ev["near_pred_all"] and ev["nrec"] >= 12:
        t["near_pred_all"] = tuple(ev["path"])
    for i, g in enumerate(ev["gaps"]):
        t.setdefault("gap=%d" % g, (ev["path"][i],))
    return t


# ---- pixel blocks -------------------------------------------------------------------------------------------------------------------
_X = np.arange(8)
_COS = np.cos((2 * _X[:, None] + 1) * np.arange(8)[None, :] * np.pi / 16)       # [sample, frequency]
_A = np.where(np.arange(8) == 0, np.sqrt(0.5), 1.0)


def coef_block(q_nat, amps, dither=None):
    """8x8 samples whose DCT is amps[k] quantizer steps at zig-zag position k and (to within the rounding of the samples) nothing
    elsewhere; dither: seed of a perturbation below the rounding, which moves the raw coefficients by a few units"""
    blk = np.full((8, 8), 128.0)
    for k, m in amps.items():
        v, u = divmod(int(ZZ[k]), 8)
        blk += float(m) * float(q_nat[int(ZZ[k])]) * 0.25 * _A[u] * _A[v] * np.outer(_COS[:, v], _COS[:, u])
    if dither is not None:
        blk += np.random.default_rng(dither).uniform(-0.5, 0.5, (8, 8))
    if blk.min() < 0 or blk.max() > 254:
        return None          # leaves the sample range (or would take the deringing path)
    return np.rint(blk).astype(np.uint8)


def spec_block(q_nat, spec):
    """one 8x8 pixel block of a spec tuple:
      ("coef", {position: steps}, dither)    dictated multiples of the quantizer step
      ("rand", seed, n, lo, hi, pmax)         n positions out of 1..pmax drawn with the seed, each +-[lo, hi) steps
      ("head", seed, n, lo, hi) / ("tail", ..)  the first / last n positions, each +-[lo, hi) steps
      ("weak", seed, first, n, strong_at, w)  n coefficients of +-w steps (just above half a step) from `first` on, and +-3 steps at
                                              each position of strong_at
      ("noise", seed, sigma) ("flat", value) ("s44", polarity) ("checker",)"""
    kind = spec[0]
    if kind == "coef":
        b = coef_block(q_nat, spec[1], spec[2] if len(spec) > 2 else None)
    elif kind in ("rand", "head", "tail"):
        rng = np.random.default_rng(spec[1])
        n, lo, hi = spec[2], spec[3], spec[4]
        if kind == "rand":
            pos = sorted(rng.choice(np.arange(1, spec[5] + 1), n, replace=False).tolist()) if n else []
        else:
            pos = list(range(1, n + 1)) if kind == "head" else list(range(64 - n, 64))
        b = coef_block(q_nat, {int(p): float(rng.uniform(lo, hi) * rng.choice([-1.0, 1.0])) for p in pos}, spec[1])
    elif kind == "weak":
        rng = np.random.default_rng(spec[1])
        amps = {p: float(spec[5] * rng.choice([-1.0, 1.0])) for p in range(spec[2], spec[2] + spec[3])}
        for p in spec[4]:
            amps[p] = float(3.0 * rng.choice([-1.0, 1.0]))
        b = coef_block(q_nat, amps, spec[1])
    elif kind == "noise":
        b = np.clip(128 + np.random.default_rng(spec[1]).normal(0, spec[2], (8, 8)), 0, 254).astype(np.uint8)
    elif kind == "flat":
        b = np.full((8, 8), spec[1], np.uint8)
    elif kind == "s44":
        s = np.sign(np.outer(_COS[:, 4], _COS[:, 4]))
        b = np.where(s * spec[1] > 0, 255, 0).astype(np.uint8)
    elif kind == "checker":
        yy, xx = np.mgrid[0:8, 0:8]
        b = np.where((xx + yy) % 2 == 0, 0, 255).astype(np.uint8)
    else:
        raise ValueError(kind)
    assert b is not None, "spec %r leaves the sample range" % (spec,)
    return b


# ---- cases --------------------------------------------------------------------------------------------------------------------------
DYADIC_TABLE = [1] * 64          # every step 2^0; lambda2 <= 0 and an integer lambda1: lambda = 2^(lambda1 - 12), lambda_tbl = 1


class Case(object):
    """blocks: one spec per 8x8 block of the one block row; dictated: {block index: tokens it has to show}"""

    def __init__(self, name, kw, blocks, dictated, table=None, lambda1=None, lambda2=None, wave=None, loops=1):
        self.name, self.kw, self.blocks, self.dictated = name, dict(kw), list(blocks), dict(dictated)
        self.table, self.lambda1, self.lambda2 = table, lambda1, lambda2
        self.loops = loops       # the trellis loop whose pass shows the claimed events (2: priced with the first loop's result)
        self.wave = wave         # the largest quantized magnitude EVERY block of the image has to stay within, reached by one
        self.w, self.h = 8 * len(self.blocks), 8

    @property
    def ordinary(self):
        return self.table is None and self.lambda1 is None

    def params(self, make, extra=None):
        """parameter struct of the oracle (make = O.make_params) or of the product (M.make_params)"""
        kw = dict(self.kw)
        kw.update(extra or {})
        p = make(self.w, self.h, gray=True, grayin=True, **kw)
        tab = p.qtbl if hasattr(p, "qtbl") else p.quantval
        if self.table is not None:
            for t in range(4):
                for i in range(64):
                    tab[t][i] = self.table[i]
        if self.lambda1 is not None:
            p.lambda_log_scale1 = self.lambda1
        if self.lambda2 is not None:
            p.lambda_log_scale2 = self.lambda2
        return p

    def q_nat(self):
        p = self.params(O.make_params)
        return [int(v) for v in p.qtbl[p.quant_tbl_no[0]][:]]

    def image(self):
        q = self.q_nat()
        img = np.empty((8, self.w), np.uint8)
        for b, spec in enumerate(self.blocks):
            img[:, 8 * b:8 * b + 8] = spec_block(q, spec)
        return img[..., None]


def _fill(seed, sigma=30):
    return ("noise", seed, sigma)


def _interleave(dictated_specs, seed0, sigma=30, every=1):
    """dictated blocks with `every` filler blocks behind each; returns (blocks, indices of the dictated ones)"""
    blocks, idx = [], []
    for i, s in enumerate(dictated_specs):
        idx.append(len(blocks))
        blocks.append(s)
        for j in range(every):
            blocks.append(_fill(seed0 + 7 * i + j, sigma))
    return blocks, idx


COUNTS = (0, 1, 15, 16, 17, 23, 24, 25, 31, 32, 33, 47, 48, 49, 62, 63)
MAGS = (1, 2, 3, 4, 7, 8, 15, 16, 17, 255)
GAPS = (15, 16, 17, 31, 32, 33, 47, 48, 62)
Q92, Q75, Q50, Q97, Q88 = (dict(quality=q, baseline=True) for q in (92, 75, 50, 97, 88))


def _counts_case():
    specs, want = [], []
    for n in COUNTS:
        specs += [("head", 100 + n, n, 1.0, 2.4), ("tail", 200 + n, n, 1.0, 2.4)]
        want += ["nrec=%d" % n] * 2
    blocks, idx = _interleave(specs, 1000)
    return Case("counts_q92", Q92, blocks, {b: [t] for b, t in zip(idx, want)})


def _mags_case(name, kw, mags, at):
    specs, want = [], []
    for m in mags:
        for p in at:
            specs.append(("coef", {p: float(m), p + 3: 1.0, p + 9: -1.0}, 300 + m))
            want.append("maxq=%d" % m)
    blocks, idx = _interleave(specs, 2000)
    return Case(name, kw, blocks, {b: [t] for b, t in zip(idx, want)})


def _mags255_case():
    """steps of 1: the rounding of the samples moves a raw coefficient by a few units, so the seed decides"""
    blocks, idx = _interleave([("coef", {1: 255.0, 4: 1.0, 10: -1.0}, 0), ("coef", {2: 255.0, 5: 1.0, 11: -1.0}, 1000)], 2000)
    return Case("mags_q97", Q97, blocks, {b: ["maxq=255"] for b in idx})


def _gaps_case():
    specs, want = [], []
    for g in GAPS:
        specs.append(("coef", {g + 1: 3.0}, 400 + g))                                   # the run counted from the start of the block
        specs.append(("coef", {1: 3.0, g + 2: -3.0}, 500 + g) if g < 62 else ("coef", {63: -3.0}, 500 + g))
        want += ["gap=%d" % g] * 2
    blocks, idx = _interleave(specs, 3000)
    return Case("gaps_q92", Q92, blocks, {b: [t] for b, t in zip(idx, want)})


def _wave_case(name, bound, seed):
    """64 blocks = one wave of every first tier: every block's largest quantized magnitude is at most `bound`"""
    blocks = [("rand", seed + b, 1 + b % 9, 0.55, bound + 0.4, 30) for b in range(64)]
    blocks[5] = ("coef", {2: float(bound), 7: 1.0}, seed)
    blocks[44] = ("coef", {4: -float(bound), 1: 1.0}, seed + 1)
    return Case(name, Q75, blocks, {5: ["maxq=%d" % bound], 44: ["maxq=%d" % bound]}, wave=bound)


def _clamp_case():
    blocks = [_fill(41, 50), ("s44", 1), ("checker",), ("s44", -1), _fill(42, 50), ("checker",), ("s44", 1), _fill(43, 50)]
    return Case("clamp_q100", dict(quality=100, baseline=True), blocks,
                {1: ["clamped", "maxq=1023"], 3: ["clamped", "maxq=1023"], 6: ["clamped", "maxq=1023"]})


def _dyadic(name, specs, want, lambda1):
    return Case(name, dict(quality=75, baseline=True), specs, want, table=DYADIC_TABLE, lambda1=lambda1, lambda2=-1.0)


# ---- the generators `search` was run over; FOUND_SEEDS = what it found, with the events each dictated block was found to show -------
def gen_dyadic(s):
    """dyadic setting, lambda = 1/4: every cost is an exact multiple of 1/4, equal costs are common"""
    specs = [("rand", 10 * s + i, 3 + (s + i) % 5, 0.55, 3.4, 16) for i in range(4)]
    blocks, idx = _interleave(specs, 4000 + s, 6)
    return _dyadic("dyadic_%d" % s, blocks, {b: [] for b in idx}, 10.0)


def gen_dyadic2(s):
    """dyadic setting with every step 2 and lambda = 1: the rounding of the samples stays below half a step, so the blocks keep the few
    records they were given -- at most 16, magnitudes below 16: they stay in the first tier at every capacity"""
    specs = [("rand", 10 * s + i, 3 + (s + i) % 5, 0.55, 3.4, 16) for i in range(4)]
    blocks, idx = _interleave(specs, 4000 + s, 12)
    return Case("dyadic2_%d" % s, dict(quality=75, baseline=True), blocks, {b: [] for b in idx}, table=[2] * 64, lambda1=12.0, lambda2=-1.0)


def gen_nozrl(s):
    """dyadic setting, steps of 2, lambda = 1/4: two strong coefficients 18 to 23 positions apart and a weak one half way, among
    dense filler: no block of the image has a run of 16, so the table has no ZRL; zeroing the weak coefficient would pay if the run
    of 17 and more it leaves could be coded"""
    rng = np.random.default_rng(s)
    specs = []
    for i in range(2):
        a = 1 + int(rng.integers(0, 6))
        specs.append(("coef", {a: 2.0, a + 9: 0.56, a + 18 + int(rng.integers(0, 6)): -2.0}, 10 * s + i))
    blocks, idx = _interleave(specs, 7000 + s, 12)
    return Case("nozrl_%d" % s, dict(quality=75, baseline=True), blocks, {b: [] for b in idx}, table=[2] * 64, lambda1=10.0, lambda2=-1.0)


def gen_weak(s):
    """runs of coefficients just above half a step between strong ones: zeroing the whole run is the cheapest path, so a position
    chooses a predecessor (or the virtual start) far behind its nearest live one.  Behind each such block one that holds the strong
    coefficients alone: its symbols give the long run a code."""
    w = 0.53
    specs = [("weak", s, 30, 12, (29, 42), w), ("coef", {29: 3.0, 42: -3.0}, s), ("weak", s + 500, 33, 10, (31, 43), w),
             ("coef", {31: 3.0, 43: 3.0}, s), ("weak", s + 900, 20, 10, (30,), w), ("coef", {30: 3.0}, s),
             ("weak", s + 1300, 24, 9, (33,), w), ("coef", {33: -3.0}, s)]
    blocks, idx = _interleave(specs, 5000 + s)
    return Case("weak_%d" % s, Q92, blocks, {b: [] for b in idx})


def gen_small(s):
    """three blocks, each ending at position 63 (no end-of-block symbol in the histogram) and none with a run of 16 (no ZRL): the
    table has codes for these blocks' own symbols only"""
    rng = np.random.default_rng(s)
    specs = []
    for b in range(3):
        pos = [1 + b, 12 + b, 24 + int(rng.integers(0, 3)), 37, 49 + b, 63]
        amps = {p: float(rng.choice([-1, 1]) * rng.choice([1.0, 2.0, 3.0])) for p in pos}
        amps[int(rng.integers(2, 11)) + 3] = 0.53
        amps[63] = 1.0 + b % 2
        specs.append(("coef", amps, s + b))
    return Case("small_%d" % s, Q92, specs, {b: [] for b in range(3)})


def gen_zeroed(s):
    specs = [("coef", {3 + s % 7: 0.56 + 0.02 * (s % 5)}, s), ("coef", {1 + s % 4: -0.6, 12: 0.58}, s + 50)]
    blocks, idx = _interleave(specs, 6000 + s)
    return Case("zeroed_%d" % s, Q75, blocks, {b: [] for b in idx})


def gen_loops2(s):
    """four blocks alone: the second loop prices with the table of the first loop's result, which has lost symbols the second loop's
    candidates need -- a position can be left without any code"""
    rng = np.random.default_rng(s)
    specs = []
    for b in range(4):
        pos = sorted(rng.choice(np.arange(1, 30), 6 + b, replace=False).tolist())
        specs.append(("coef", {int(p): float(rng.choice([-1, 1]) * rng.uniform(0.52, 2.4)) for p in pos}, s + b))
    return Case("loops2_%d" % s, Q92, specs, {b: [] for b in range(4)}, loops=2)


FOUND_SEEDS = [
    (gen_dyadic, 0, {4: ["tie_pred"], 6: ["tie_pred", "tie_cand"], 0: ["eob_tie"]}),
    (gen_dyadic, 2, {0: ["eob_tie"], 4: ["eob_tie", "tie_pred"], 6: ["eob_tie"]}),
    (gen_dyadic, 5, {0: ["tie_cand"], 2: ["tie_cand"]}),
    (gen_dyadic2, 36, {2: ["tie_pred", "first_tier_16"]}),
    (gen_dyadic2, 70, {6: ["tie_pred", "first_tier_16"]}),
    (gen_dyadic2, 8, {2: ["tie_cand", "first_tier_16"], 6: ["tie_cand", "first_tier_16"]}),
    (gen_dyadic2, 28, {6: ["eob_tie", "first_tier_16"], 0: ["tie_cand", "first_tier_16"]}),
    (gen_dyadic2, 6, {2: ["eob_tie", "first_tier_16"]}),
    (gen_nozrl, 2, {0: ["zrl_forbidden_cheaper", "first_tier_16"], 2: ["zrl_forbidden_cheaper", "first_tier_16"]}),
    (gen_nozrl, 3, {0: ["zrl_forbidden_cheaper", "first_tier_16"]}),
    (gen_weak, 0, {0: ["far_pred", "no_code_cheaper"], 4: ["far_pred", "no_code_cheaper"], 8: ["start_pred"]}),
    (gen_weak, 4, {0: ["far_pred"], 8: ["start_pred"], 12: ["start_pred"]}),
    (gen_small, 2, {0: ["eob_no_code", "zrl_forbidden", "no_code", "last_at_se"], 1: ["eob_no_code", "zrl_forbidden", "no_code", "last_at_se"],
                    2: ["eob_no_code", "zrl_forbidden", "last_at_se"]}),
    (gen_small, 10, {b: ["eob_no_code", "zrl_forbidden", "no_code", "last_at_se"] for b in range(3)}),
    (gen_zeroed, 0, {0: ["band_zeroed"], 2: ["band_zeroed"]}),
    (gen_loops2, 14, {3: ["dead_position"]}),
    (gen_loops2, 21, {2: ["dead_position"]}),
]


def found_cases():
    out = []
    for gen, seed, claims in FOUND_SEEDS:
        c = gen(seed)
        c.dictated = {b: list(claims.get(b, [])) for b in c.dictated}
        out.append(c)
    return out


def section2_cases():
    cs = [_counts_case(),
          _mags_case("mags_q75", Q75, (1, 2, 3, 4, 7, 8, 15, 16, 17), (1, 6)),
          _mags_case("mags_q50", Q50, (1, 2, 3, 4, 7), (2, 5)),
          _mags_case("mags_q88", Q88, (1, 3, 8, 15, 17), (3, 7)),
          _mags255_case(),
          _gaps_case(), _clamp_case(),
          _wave_case("wave_nc1", 1, 600), _wave_case("wave_nc2", 3, 700), _wave_case("wave_nc4", 7, 800)]
    cs += found_cases()
    for c in cs:      # what the blocks of the constructed cases show besides what they were built for
        if c.name == "counts_q92":
            for b, t in c.dictated.items():
                if int(t[0].split("=")[1]) >= 15:
                    t.append("near_pred_all")
        if c.name == "gaps_q92":
            for b in [b for b, t in c.dictated.items() if t[0] == "gap=62"]:
                c.dictated[b].append("last_at_se")
    return cs


@functools.lru_cache(maxsize=None)
def cases():
    return {c.name: c for c in section2_cases()}


# ---- what the oracle and the restatement say about a case ----------------------------------------------------------------------------
class Facts(object):
    pass


def _zz_blocks(tap):
    """[blocks of the one block row][64 zig-zag] of a tap [hpad][wpad][64 natural]"""
    return tap[0][:, ZZ]


@functools.lru_cache(maxsize=None)
def _facts_cached(case_id, loops, progressive):
    return _facts(_BY_ID[case_id], loops, progressive)


def facts(case, loops=1, progressive=False):
    _BY_ID[id(case)] = case
    return _facts_cached(id(case), loops, progressive)


_BY_ID = {}


def _facts(case, loops, progressive):
    """oracle file and taps of the case, and for every dictated block the restated block and its events (of the LAST loop)"""
    extra = dict(trellis_loops=loops)
    if progressive:
        extra.update(baseline=False, fastcrush=True)
    f = Facts()
    f.extra = extra
    f.img = case.image()
    po = case.params(O.make_params, extra)
    f.file, taps = O.encode(po, f.img, want_taps=True)
    nb = len(case.blocks)
    f.uq, f.q0, f.q = (taps[(n, 0)][:, :nb] for n in ("coef_uq", "coef_q0", "coef_q"))
    front = f.q0
    if loops == 2:      # the second loop's table and stale values: the first loop's result
        front = facts(case, 1, progressive).q
    f.size = pass_lengths(_zz_blocks(front), progressive)
    qt = case.q_nat()
    f.events, f.restated = {}, {}
    for b in case.dictated:
        blk, ev = restate_block(f.uq[0, b], front[0, b], qt, f.size, po.lambda_log_scale1, po.lambda_log_scale2)
        ev["ndiff_q0"] = int(np.count_nonzero(np.asarray(blk)[1:] != f.q0[0, b, 1:]))
        f.events[b], f.restated[b] = ev, np.asarray(blk, np.int16)
    x = np.abs(f.uq[0].astype(np.int64))
    q8 = 8 * np.asarray(qt, np.int64)[None, :]
    f.qval = np.minimum((x + q8 // 2) // q8, 1023)[:, 1:]          # [block][natural 1..63]
    f.image_ndiff = int(np.count_nonzero(f.q[0, :, 1:] != f.q0[0, :, 1:]))
    return f


def check_restatement(case, loops=1, progressive=False):
    f = facts(case, loops, progressive)
    for b in case.dictated:
        want = f.q[0, b]
        got = f.restated[b]
        bad = [k for k in range(1, 64) if got[ZZ[k]] != want[ZZ[k]]]
        assert not bad, "%s block %d: the restatement differs from the oracle at positions %s" % (case.name, b, bad)


def check_premise(case, progressive=False, want=None):
    f = facts(case, case.loops, progressive)
    assert f.image_ndiff > 0, "%s: a trellis that does nothing would pass" % case.name
    for b, toks in (want or case.dictated).items():
        have = tokens(f.events[b])
        for t in toks:
            assert t in have, "%s block %d: %s not shown (has %s)" % (case.name, b, t, sorted(have))
        for t in toks:
            if t.startswith("nrec="):
                assert f.events[b]["maxq"] < 16, "%s block %d: a magnitude of 16 or more" % (case.name, b)
            if t.startswith("maxq="):
                assert f.events[b]["nrec"] <= 8, "%s block %d: more than 8 records" % (case.name, b)
    if case.wave is not None:
        top = f.qval.max(axis=1)
        assert top.max() == case.wave and top.min() >= 1, "%s: magnitudes %d..%d" % (case.name, top.min(), top.max())


REQUIRED = (["nrec=%d" % n for n in COUNTS] + ["maxq=%d" % m for m in MAGS + (1023,)] + ["gap=%d" % g for g in GAPS] +
            ["clamped", "tie_pred", "tie_cand", "eob_tie", "no_code", "dead_position", "zrl_forbidden", "eob_no_code", "far_pred",
             "start_pred", "near_pred_all", "last_at_se", "band_zeroed", "no_code_cheaper", "zrl_forbidden_cheaper"])
# no_code_cheaper / zrl_forbidden_cheaper: the candidate (predecessor) a missing code keeps out would have cost LESS than the choice if
# the missing code were a code of length 0 -- only then does dropping the rule change the block.
# The ties and the forbidden run also need two blocks that stay in a first tier of 16 records (first_tier_16).
IN_FIRST_TIER = ("tie_pred", "tie_cand", "eob_tie", "zrl_forbidden_cheaper")


def coverage(entries):
    """entries: cases.  {token: [(case name, block, where)]} over the tokens the cases CLAIM and show"""
    out = {}
    for case in entries:
        f = facts(case, case.loops)
        for b, toks in case.dictated.items():
            have = tokens(f.events[b])
            for t in toks:
                if t in have:
                    out.setdefault(t, []).append((case.name, b, have[t]))
    return out


# events that can happen at one place only: a gap of 62 zeros ends at position 63, no records and 63 records are one set of positions
# each, and 8-bit samples reach 1024 steps only in the (4, 4) coefficient of its own sign pattern (test_large_magnitudes)
ONE_PLACE = ("gap=62", "nrec=0", "nrec=63", "clamped", "maxq=1023")


def check_coverage():
    """every required event is claimed and shown by at least two dictated blocks, in different lanes (block index modulo 64) and --
    where the event can move -- at different positions"""
    cov = coverage(cases().values())
    for t in REQUIRED:
        e = cov.get(t, [])
        assert len(e) >= 2, "%s: shown by %d blocks" % (t, len(e))
        assert len(set(b % 64 for _, b, _ in e)) >= 2, "%s: one lane" % t
        if t not in ONE_PLACE:
            assert len(set(w for _, _, w in e)) >= 2, "%s: one position (%s)" % (t, e)
        if t in IN_FIRST_TIER:
            small = set((name, b) for name, b, _ in cov.get("first_tier_16", []))
            assert len([1 for name, b, _ in e if (name, b) in small]) >= 2, "%s: not twice within 16 records" % t
    return cov


# ---- schedules ----------------------------------------------------------------------------------------------------------------------
# name -> (environment around Encoder(...), debug taps, table entry above 255, make_params keywords on top of the case's)
def _env(**kw):
    return {k: str(v) for k, v in kw.items()}


SCHEDULES = {"default": (_env(), False, False, {})}
for _v in (0, 2, 3, 4):
    SCHEDULES["sorted_v%d" % _v] = (_env(MJH_SMALL_BATCH=1, MJH_TRELLIS_VARIANT=_v), False, False, {})
for _n in (2, 8):
    SCHEDULES["sorted_v0_passes%d" % _n] = (_env(MJH_SMALL_BATCH=1, MJH_TRELLIS_VARIANT=0, MJH_TRELLIS_V3=_n), False, False, {})
for _v in (0, 1, 2, 3):
    SCHEDULES["general_v%d" % _v] = (_env(MJH_TRELLIS_V3=0, MJH_TRELLIS_VARIANT=_v), False, False, {})
SCHEDULES["planes_v0"] = (_env(MJH_SMALL_BATCH=1, MJH_TRELLIS_VARIANT=0, MJH_DENSE_CAP=0), False, False, {})
FIRST_FIVE = list(SCHEDULES)                      # the schedules of the two first tiers: what the wave / tile shapes run under
# debug taps: the same compact kernels as "default" (compact records depend on the coding parameters alone), plus the comparison of
# TAP_COEF_Q with the oracle's blocks; the one-plane-per-position instantiations run under the two-loop schedules below
SCHEDULES["taps"] = (_env(), True, False, {})
SCHEDULES["wide_table"] = (_env(), False, True, {})
for _v in (0, 2, 3, 4):     # FD = false at every capacity of the tile-sorted tier
    SCHEDULES["wide_table_sorted_v%d" % _v] = (_env(MJH_SMALL_BATCH=1, MJH_TRELLIS_VARIANT=_v), False, True, {})
SCHEDULES["progressive"] = (_env(), False, False, dict(baseline=False, fastcrush=True))
SCHEDULES["loops2"] = (_env(), False, False, dict(trellis_loops=2))
for _v in (0, 1, 2, 3):     # two loops: one plane per position, k_trellis_ac_q<16 / 20 / 24 / 32, false, false>
    SCHEDULES["loops2_v%d" % _v] = (_env(MJH_TRELLIS_VARIANT=_v), False, False, dict(trellis_loops=2))
SCHEDULES["progressive_loops2"] = (_env(), False, False, dict(baseline=False, fastcrush=True, trellis_loops=2))
ALL_SCHEDULES = list(SCHEDULES)
WIDE_AT, WIDE_STEP = 63, 300                      # natural index and value of the table entry above 255


def encode_product(M, params, imgs, env, taps=False):
    """the product's files of a batch under a schedule; with taps also the TAP_COEF_Q planes of image 0, component 0"""
    saved = {k: os.environ.get(k) for k in env}
    enc = None
    try:
        os.environ.update(env)                       # (read when the encoder is made)
        enc = M.Encoder(params, max_batch=len(imgs))
        if taps:
            enc.set_debug_taps(True)
        files = enc.encode_host(np.stack(imgs))
        tap = enc.read_tap(M.TAP_COEF_Q, 0, 0).copy() if taps else None      # [64 zig-zag][blocks]
        return files, tap
    finally:
        if enc is not None:
            enc.close()
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def case_schedules():
    """(case name, schedule) of section 2: every case under every schedule; the table entry above 255 on the ordinary setting only"""
    return [(n, s) for n, c in cases().items() for s in ALL_SCHEDULES if c.ordinary or not SCHEDULES[s][2]]


def shape_schedules():
    return [(n, s) for n in shape_cases() for s in FIRST_FIVE]


def _real(case, f):
    """the real reference's file of an ordinary-setting gray case, once per case (None where the reference is not built)"""
    if not hasattr(f, "real"):
        f.real = O.ref_encode(f.img, gray=True, **case.kw)[0] if O.have_ref() and case.ordinary else None
    return f.real


_WANT = {}
_FILES = {}      # (case name, parameters) -> (schedule, file): schedules that share their parameters must give one file


def run_case(M, case, sched):
    """one section-2 case under one schedule: the product's file against the oracle's (and the real reference's)"""
    env, taps, wide, extra = SCHEDULES[sched]
    assert case.ordinary or not wide
    key = (case.name, wide, tuple(sorted(extra.items())))
    pg = case.params(M.make_params, extra)
    if wide:
        pg.quantval[0][WIDE_AT] = WIDE_STEP
    if key not in _WANT:          # the oracle's file and blocks, and the real reference's file: once per set of parameters
        po = case.params(O.make_params, extra)
        if wide:
            po.qtbl[0][WIDE_AT] = WIDE_STEP
        img = case.image()
        want, otaps = O.encode(po, img, want_taps=True)
        real = None
        if O.have_ref() and case.ordinary and not wide:
            kw = dict(case.kw)
            kw.update(extra)
            real = O.ref_encode(img, gray=True, **kw)[0]
        _WANT[key] = (img, want, otaps[("coef_q", 0)][0, :len(case.blocks)][:, ZZ], real)
    img, want, ref, real = _WANT[key]          # ref: [block][zig-zag]
    got, tap = encode_product(M, pg, [img], env, taps)
    if taps:
        bad = np.argwhere(tap.T[:, 1:] != ref[:, 1:])
        assert bad.size == 0, "%s/%s: TAP_COEF_Q differs first at block %d position %d: %d, the oracle %d" % (
            case.name, sched, bad[0][0], bad[0][1] + 1, tap.T[bad[0][0], bad[0][1] + 1], ref[bad[0][0], bad[0][1] + 1])
    assert got[0] == want, "%s/%s: the file differs from the oracle's (%d vs %d bytes)" % (case.name, sched, len(got[0]), len(want))
    if real is not None:
        assert real == got[0], "%s/%s: the file differs from the real reference's" % (case.name, sched)
    first = _FILES.setdefault(key, (sched, got[0]))
    assert first[1] == got[0], "%s: schedules %s and %s give different files" % (case.name, first[0], sched)
    return got[0]


# ---- wave and tile shapes (section 3) ------------------------------------------------------------------------------------------------
def _busy(seed, nb, sigma=35):
    return [("noise", seed + b, sigma) for b in range(nb)]


def _with_dictated(blocks):
    """a few dictated blocks among the filler: in the first lane, across the wave boundary, in the last block"""
    nb = len(blocks)
    if nb == 1:
        return blocks
    marks = {0: ("coef", {1: 2.0, 18: -2.0}, 1), nb - 1: ("coef", {63: 1.5, 2: 1.0}, 2)}
    for b in (63, 64, 255, 256, 511, 512):
        if b < nb - 1:
            marks[b] = ("head", 900 + b, 17 + b % 5, 1.0, 2.0)
    for b, s in marks.items():
        blocks[b] = s
    return blocks


SHAPE_COUNTS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513)


@functools.lru_cache(maxsize=None)
def shape_cases():
    cs = {}
    for nb in SHAPE_COUNTS:
        cs["blocks_%d" % nb] = Case("blocks_%d" % nb, Q75, _with_dictated(_busy(10 * nb, nb)), {})
    cs["flat_image"] = Case("flat_image", Q75, [("flat", 77)] * 256, {})
    cs["flat_tile_in_busy"] = Case("flat_tile_in_busy", Q75, _busy(5, 256) + [("flat", 128)] * 256 + _busy(6, 65), {})
    one = [("flat", 100)] * 256
    one[201] = ("coef", {3: 2.0, 40: -1.0}, 3)
    cs["one_in_flat_tile"] = Case("one_in_flat_tile", Q75, one + _busy(8, 64), {})
    cs["same_key"] = Case("same_key", Q92, [("rand", 50 + b, 9, 1.2, 2.4, 40) for b in range(256)], {})
    clampk = _busy(9, 256, 20)
    for b in (7, 100, 255):
        clampk[b] = ("head", 60 + b, 63, 1.0, 2.0)
    cs["key_63"] = Case("key_63", Q92, clampk, {})
    return cs


def check_shape_premise(name, case):
    """the keys of the tile sort (non-zero conventionally quantized AC coefficients per block) are what the case is named for"""
    f = facts(case)
    keys = np.count_nonzero(f.q0[0, :, 1:], axis=1)
    if name == "flat_image":
        assert keys.max() == 0
    elif name == "flat_tile_in_busy":
        assert keys[256:512].max() == 0 and keys[:256].min() > 0 and keys[512:].min() > 0
    elif name == "one_in_flat_tile":
        assert np.count_nonzero(keys[:256]) == 1 and keys[201] > 0
    elif name == "same_key":
        assert keys.min() == keys.max() == 9
    elif name == "key_63":
        assert keys.max() == 63 and np.count_nonzero(keys == 63) == 3
    else:
        assert len(keys) == int(name.split("_")[1]) and keys.max() > 16
    if name != "flat_image":
        assert f.image_ndiff > 0


def run_shape(M, case, sched):
    env, _, _, extra = SCHEDULES[sched]
    f = facts(case)
    got, _ = encode_product(M, case.params(M.make_params, extra), [f.img], env)
    assert got[0] == f.file, "%s/%s: the file differs from the oracle's (%d vs %d bytes)" % (case.name, sched, len(got[0]), len(f.file))
    if _real(case, f) is not None:
        assert f.real == got[0], "%s/%s: the file differs from the real reference's" % (case.name, sched)
    first = _FILES.setdefault((case.name, "shape"), (sched, got[0]))
    assert first[1] == got[0], "%s: schedules %s and %s give different files" % (case.name, first[0], sched)
    return got[0]


@functools.lru_cache(maxsize=None)
def batch_images():
    """three distinct images of 65 blocks for one call"""
    return [Case("batch_%d" % i, Q75, _with_dictated(_busy(70 + 100 * i, 65, 20 + 15 * i)), {}) for i in range(3)]


def run_batch(M, sched):
    env, _, _, extra = SCHEDULES[sched]
    cases = batch_images()
    want = [facts(c).file for c in cases]
    assert len(set(want)) == 3
    got, _ = encode_product(M, cases[0].params(M.make_params, extra), [facts(c).img for c in cases], env)
    for i in range(3):
        assert got[i] == want[i], "batch/%s: image %d differs from the oracle's" % (sched, i)
        if _real(cases[i], facts(cases[i])) is not None:
            assert facts(cases[i]).real == got[i], "batch/%s: image %d differs from the real reference's" % (sched, i)


# ---- three components, 4:2:0 -------------------------------------------------------------------------------------------------------
COLOR_W, COLOR_H = 200, 120                       # 375 + 104 + 104 blocks
COLOR_KW = dict(quality=75, baseline=True, yccin=True)
COLOR_DICTATED = {(0, 0, 0): [2, 9, 30], (0, 7, 23): [1, 17], (0, 14, 24): [5, 63], (1, 0, 11): [3, 20], (1, 6, 5): [1, 2, 40],
                  (2, 3, 0): [4, 36], (2, 6, 11): [63]}      # (component, block row, block column): non-zero positions; whole blocks
                                                             # (the last chroma row and column of blocks are half padding)


@functools.lru_cache(maxsize=None)
def color_facts():
    """a Y / Cb / Cr image (in_color_space = YCbCr: the samples are the planes) whose chroma planes are doubled in both directions,
    so that the 2x2 box filter gives them back: dictated luma and chroma blocks among noise"""
    f = Facts()
    po = O.make_params(COLOR_W, COLOR_H, **COLOR_KW)
    rng = np.random.default_rng(420)
    planes = [np.clip(128 + rng.normal(0, s, shp), 0, 254).astype(np.uint8) for s, shp in ((30, (120, 200)), (15, (60, 100)), (15, (60, 100)))]
    for (ci, by, bx), pos in COLOR_DICTATED.items():
        q = [int(v) for v in po.qtbl[po.quant_tbl_no[ci]][:]]
        blk = coef_block(q, {p: (2.0 if i % 2 == 0 else -1.5) for i, p in enumerate(pos)})
        part = planes[ci][8 * by:8 * by + 8, 8 * bx:8 * bx + 8]
        part[...] = blk[:part.shape[0], :part.shape[1]]
    f.img = np.stack([planes[0], np.repeat(np.repeat(planes[1], 2, 0), 2, 1), np.repeat(np.repeat(planes[2], 2, 0), 2, 1)], axis=-1)
    f.file, f.taps = O.encode(po, f.img, want_taps=True)
    f.po = po
    return f


def check_color_premise():
    f = color_facts()
    gs, _, _ = O.geometry(f.po)
    assert [g.wib * g.hib for g in gs] == [375, 104, 104]
    for ci, g in enumerate(gs):
        q0 = f.taps[("coef_q0", ci)][:g.hib, :g.wib]
        size = pass_lengths(q0.reshape(-1, 64)[:, ZZ])
        qt = [int(v) for v in f.po.qtbl[f.po.quant_tbl_no[ci]][:]]
        assert np.count_nonzero(f.taps[("coef_q", ci)][:g.hib, :g.wib, 1:] != q0[..., 1:]) > 0
        for (c2, by, bx), pos in COLOR_DICTATED.items():
            if c2 != ci:
                continue
            got = [k for k in range(1, 64) if q0[by, bx, ZZ[k]] != 0]
            assert got == pos, "component %d block (%d, %d): non-zeros at %s, intended %s" % (ci, by, bx, got, pos)
            blk, _ = restate_block(f.taps[("coef_uq", ci)][by, bx], q0[by, bx], qt, size, f.po.lambda_log_scale1, f.po.lambda_log_scale2)
            want = f.taps[("coef_q", ci)][by, bx]
            bad = [k for k in range(1, 64) if blk[ZZ[k]] != want[ZZ[k]]]
            assert not bad, "component %d block (%d, %d): the restatement differs from the oracle at %s" % (ci, by, bx, bad)


def run_color(M, sched):
    env, _, _, extra = SCHEDULES[sched]
    f = color_facts()
    kw = dict(COLOR_KW)
    kw.update(extra)
    got, _ = encode_product(M, M.make_params(COLOR_W, COLOR_H, **kw), [f.img], env)
    assert got[0] == f.file, "4:2:0/%s: the file differs from the oracle's (%d vs %d bytes)" % (sched, len(got[0]), len(f.file))
    if O.have_ref():
        if not hasattr(f, "real"):
            f.real = O.ref_encode(f.img, **kw)[0]
        assert f.real == got[0], "4:2:0/%s: the file differs from the real reference's" % sched


# ---- the EXT instantiations (schedule 8): band-limited passes, the end-of-band-run optimisation, re-estimated tables -----------------
EXT_OPTIONS = {"scans": (dict(use_scans_in_trellis=True), 8), "scans_split1": (dict(use_scans_in_trellis=True, trellis_freq_split=1), 1),
               "scans_split62": (dict(use_scans_in_trellis=True, trellis_freq_split=62), 62), "eob_opt": (dict(trellis_eob_opt=True), 8),
               "q_opt": (dict(trellis_q_opt=True), 8)}
EXT_CODINGS = {"sequential": dict(baseline=True), "progressive": dict(fastcrush=True)}
EXT_BLOCK = 7


def ext_case(option, coding):
    """20 blocks of noise and one dictated block whose only non-zeros sit at `split` and `split + 1`: the last position of the first
    band and the first of the second"""
    opts, split = EXT_OPTIONS[option]
    kw = dict(quality=75)
    kw.update(EXT_CODINGS[coding])
    kw.update(opts)
    blocks = _busy(80, 20, 25)
    blocks[EXT_BLOCK] = ("coef", {split: 1.2, split + 1: -1.2})
    return Case("ext_%s_%s" % (option, coding), kw, blocks, {}), split


def run_ext(M, option, coding):
    case, split = ext_case(option, coding)
    img = case.image()
    want, taps = O.encode(case.params(O.make_params), img, want_taps=True)
    q0 = taps[("coef_q0", 0)][0, EXT_BLOCK]
    assert [k for k in range(1, 64) if q0[ZZ[k]] != 0] == [split, split + 1]
    assert np.count_nonzero(taps[("coef_q", 0)][0, :20, 1:] != taps[("coef_q0", 0)][0, :20, 1:]) > 0
    got, _ = encode_product(M, case.params(M.make_params), [img], {})
    assert got[0] == want, "%s: the file differs from the oracle's (%d vs %d bytes)" % (case.name, len(got[0]), len(want))
    if O.have_ref():
        assert O.ref_encode(img, gray=True, **case.kw)[0] == got[0], "%s: the file differs from the real reference's" % case.name


# ---- trellis_eob_opt: ties in the chain over a block row (k_trellis_eob_chain's wave_first_min) ---------------------------------------
EOB_CHAIN_SEEDS = {"progressive": (3, 19), "sequential": (11, 22)}      # found by running eob_chain_facts over seeds 0..59
EOB_CHAIN_CASES = [(c, s) for c, seeds in EOB_CHAIN_SEEDS.items() for s in seeds]


def eob_chain_case(coding, seed):
    """16 sparse blocks in the dyadic setting (lambda = 1/4): the costs of the run starts are exact, and equal ones are common"""
    rng = np.random.default_rng(seed)
    blocks = [("rand", 100 * seed + b, int(rng.integers(0, 4)), 0.55, 1.45, 12) for b in range(16)]
    kw = dict(quality=75, trellis_eob_opt=True)
    kw.update(EXT_CODINGS[coding])
    return Case("eobchain_%s_%d" % (coding, seed), kw, blocks, {}, table=DYADIC_TABLE, lambda1=10.0, lambda2=-1.0)


@functools.lru_cache(maxsize=None)
def eob_chain_facts(coding, seed):
    """every block of the row restated, then the chain: (image, oracle file, restatement equals the oracle's blocks, zeroed blocks,
    ties that decide a chosen run start)"""
    c = eob_chain_case(coding, seed)
    img = c.image()
    po = c.params(O.make_params)
    want, taps = O.encode(po, img, want_taps=True)
    nb = len(c.blocks)
    uq, q0, q = (taps[(n, 0)][0, :nb] for n in ("coef_uq", "coef_q0", "coef_q"))
    size = pass_lengths(q0[:, ZZ], coding == "progressive")
    qt = c.q_nat()
    info, out = [], []
    for b in range(nb):
        blk, ev = restate_block(uq[b], q0[b], qt, size, po.lambda_log_scale1, po.lambda_log_scale2)
        info.append((ev["cost_all_zeros"], ev["best_cost_skip"], ev["has_eob"]))
        out.append(np.asarray(blk))
    zeroed, ties = restate_eob_chain(info, size)
    for b in zeroed:
        out[b][1:] = 0
    same = all(np.array_equal(out[b][1:], q[b][1:]) for b in range(nb))
    return c, img, want, same, zeroed, ties


def check_eob_chain_premise(coding, seed):
    _, _, _, same, zeroed, ties = eob_chain_facts(coding, seed)
    assert same, "the restatement of the blocks and the chain differs from the oracle"
    assert ties and zeroed, "no tie decides a run start (ties %s, zeroed %s)" % (ties, zeroed)


def run_eob_chain(M, coding, seed):
    c, img, want, _, _, _ = eob_chain_facts(coding, seed)
    got, _ = encode_product(M, c.params(M.make_params), [img], {})
    assert got[0] == want, "%s: the file differs from the oracle's (%d vs %d bytes)" % (c.name, len(got[0]), len(want))


# ---- the search the committed seeds come from (not run by any test) ------------------------------------------------------------------
def search(make_case, token, seeds, block=None, loops=1, progressive=False):
    """seeds for which the case make_case(seed) shows `token` in its dictated block `block` (default: any), with the restatement
    agreeing with the oracle"""
    found = []
    for s in seeds:
        try:
            c = make_case(s)
            f = _facts(c, loops, progressive)
        except AssertionError:
            continue
        for b in ([block] if block is not None else list(c.dictated)):
            if token in tokens(f.events[b]) and not [k for k in range(1, 64) if f.restated[b][ZZ[k]] != f.q[0, b, ZZ[k]]]:
                found.append((s, b, tokens(f.events[b])[token]))
    return found
