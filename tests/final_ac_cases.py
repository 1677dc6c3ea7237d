"""Shared by test_simt_final_ac.py (CPU suite, emulator) and test_gpu_final_ac.py (-m gpu): the AC trellis kernels of mjh_trellis.hip
count the final AC symbols of the blocks they finish (the CF instantiations of k_trellis_ac_v3, k_trellis_ac_q and k_trellis_ac_qd)
instead of a k_stats_ac_compact pass behind them; MJH_FUSE_FINAL_AC=0 keeps the pass.

Every case is encoded with the knob on and off.  The histograms of the four final table slots (Encoder.final_counts) must be equal
entry by entry, and equal to the plain count over the oracle's final blocks (hist_cases.ac_histogram, one end-of-block symbol per
dummy block of the interleaved scan); the files must equal each other, the oracle's, and the real reference's where it is built and
its switches express the case.  Counts are integers: equality is exact.

The gray cases are the dictated blocks and the wave / tile shapes of trellis_cases.py, whose premises test_simt_trellis_pins.py
proves (which block has how many records, which magnitude, which run); what a case is here for is said next to it."""
import numpy as np

import oracle_lib as O
import hist_cases as HC
import trellis_cases as T
from enc_pack_groups_cases import env

KNOB = "MJH_FUSE_FINAL_AC"
SORTED = dict(MJH_SMALL_BATCH=1)          # the large-batch schedule (four passes per tile, late DC chains) on small images


# ---- what the oracle says ------------------------------------------------------------------------------------------------------------
def expected_counts(po, taps):
    """[4 slots: DC0, AC0, DC1, AC1][256] with the AC rows filled: the plain count over the oracle's final blocks of every component
    (tap [hpad][wpad][64 natural]: the blocks beyond hib x wib are the dummy blocks of the interleaved scan, one end-of-block each)"""
    gs, _, _ = O.geometry(po)
    want = np.zeros((4, 256), np.int64)
    for ci, g in enumerate(gs):
        tap = np.asarray(taps[("coef_q", ci)])
        real = tap[:g.hib, :g.wib].reshape(-1, 64)[:, T.ZZ]
        row = 2 * int(po.ac_tbl_no[ci]) + 1
        want[row] += HC.ac_histogram(real)
        if len(gs) > 1:
            want[row][0] += tap.shape[0] * tap.shape[1] - g.hib * g.wib
    return want


class Job(object):
    """one case: parameter factories for the product and the oracle, the frames of each call, the environment, whether the schedule
    may count in the trellis, and the switches of the real reference (None: not expressible)"""

    def __init__(self, name, make, frames, envkw=None, fused=True, ref_kw=None, calls=None, plain=True):
        self.name, self.make, self.frames, self.env = name, make, frames, dict(envkw or {})
        self.fused, self.ref_kw = fused, ref_kw
        self.plain = plain          # one sequential scan: the final slots hold the histograms of the whole image
        self.calls = calls          # frames of further calls through the same encoder (lists of frames)


def _gray(case, envkw=None, extra=None, fused=True, name=None, plain=True):
    make = lambda mk: case.params(mk, extra)
    kw = dict(case.kw)
    kw.update(extra or {})
    return Job(name or case.name, make, [case.image()], envkw, fused, dict(kw, gray=True) if case.ordinary else None, plain=plain)


def _frame(w, h, seed):
    """oracle_lib.synthetic_frame; an image of at most 64 x 64 is cut out next to the saturated tile the frame starts with"""
    if w <= 64 and h <= 64:
        return np.ascontiguousarray(O.synthetic_frame(64 + w, h, seed)[:, 64:])
    return O.synthetic_frame(w, h, seed)


def _colour(name, w, h, kw, seeds, envkw=None, fused=True, calls=None, plain=True):
    make = lambda mk: mk(w, h, **kw)
    frames = [_frame(w, h, s) for s in seeds]
    more = [[_frame(w, h, s) for s in c] for c in calls] if calls else None
    return Job(name, make, frames, envkw, fused, dict(kw), more, plain)


def jobs():
    S, CS = T.shape_cases(), T.cases()
    base = dict(quality=75, baseline=True)
    out = []
    # components of 1, 63, 65, 255 and 257 blocks: ragged tiles, tail lanes; with one pass per tile and with four
    for nb in (1, 63, 65, 255, 257):
        out.append(_gray(S["blocks_%d" % nb]))
        out.append(_gray(S["blocks_%d" % nb], SORTED, name="blocks_%d_sorted" % nb))
    # a tile whose later passes are all key 0 (one busy block in 256 flat ones); an all-zero image; a flat tile between busy ones
    out.append(_gray(S["one_in_flat_tile"], SORTED))
    out.append(_gray(S["flat_image"], SORTED))
    out.append(_gray(S["flat_image"], name="flat_image_one_pass"))
    out.append(_gray(S["flat_tile_in_busy"], SORTED))
    # runs of 15 .. 62 zeros from the start of the block and between two coefficients (ZRL once, twice, three times); a block whose
    # last non-zero is position 63 (gap=62 and its partner: no end-of-block symbol)
    out.append(_gray(CS["gaps_q92"], SORTED))
    # 0 .. 63 records at the head and at the tail of the block: exactly 16 and 17 (the 32-record tier), 33 and more (the 63-record tier),
    # tails that end at position 63 -- under every capacity of the tile-sorted tier (16 / 24 / 32 / 48) and of the general first tier
    for v in (0, 2, 3, 4):
        out.append(_gray(CS["counts_q92"], dict(SORTED, MJH_TRELLIS_VARIANT=v), name="counts_q92_sorted_v%d" % v))
        out.append(_gray(CS["mags_q75"], dict(SORTED, MJH_TRELLIS_VARIANT=v), name="mags_q75_sorted_v%d" % v))
    for v in (0, 1, 2, 3):
        out.append(_gray(CS["counts_q92"], dict(MJH_TRELLIS_V3=0, MJH_TRELLIS_VARIANT=v), name="counts_q92_general_v%d" % v))
    out.append(_gray(CS["counts_q92"], name="counts_q92_one_pass"))          # (24 records, one pass per tile)
    # magnitudes 1 .. 17: 15 stays, 16 and 17 are deferred for their magnitude; 255 and 1023: sizes 8 and 10 in the general tiers
    out.append(_gray(CS["mags_q75"], dict(MJH_TRELLIS_V3=0), name="mags_q75_general"))
    out.append(_gray(CS["mags_q97"], SORTED))
    out.append(_gray(CS["clamp_q100"], SORTED))
    # a work list larger than its share of the dense copies: the rest comes from the planes
    out.append(_gray(CS["counts_q92"], dict(SORTED, MJH_TRELLIS_VARIANT=0, MJH_DENSE_CAP=5), name="counts_q92_dense_cap"))
    out.append(_gray(S["key_63"], dict(SORTED, MJH_TRELLIS_VARIANT=0, MJH_DENSE_CAP=1)))
    # dummy blocks in both directions (17x17: 3x3 luma blocks in 2x2 MCUs; 33x9: 5x2 in 3x1), 4:4:4 without any; per-image tables
    out.append(_colour("420_17x17", 17, 17, base, [11]))
    out.append(_colour("420_17x17_sorted", 17, 17, base, [11], SORTED))
    out.append(_colour("420_33x9", 33, 9, base, [12], SORTED))
    out.append(_colour("444_40x24", 40, 24, dict(base, sample=(1, 1)), [13], SORTED))
    out.append(_colour("420_200x120", 200, 120, base, [14], SORTED))          # 375 + 104 + 104 blocks: two luma tiles, late DC chains
    out.append(_colour("three_images", 33, 9, base, [21, 22, 23]))
    out.append(_colour("three_images_sorted", 72, 40, base, [24, 25, 26], SORTED))
    # deferred blocks of three images and three components in ONE wave of a general tier (quality 95: most blocks have more than 16
    # records, and all of them are fewer than 64): the wave counts table by table.  The general first tier adds the dummy blocks' EOBs
    out.append(_colour("three_images_q95_sorted", 33, 9, dict(base, quality=95), [27, 28, 29], dict(SORTED, MJH_TRELLIS_VARIANT=0)))
    out.append(_colour("three_images_q95_general", 33, 9, dict(base, quality=95), [27, 28, 29], dict(MJH_TRELLIS_V3=0)))
    out.append(_colour("420_33x9_general", 33, 9, base, [12], dict(MJH_TRELLIS_V3=0)))
    # two image ranges of the first tier, each with its own work list
    out.append(_colour("two_ranges", 72, 40, base, [31, 32, 33, 34, 35], dict(SORTED, MJH_TRELLIS_CHUNKS=2)))
    # consecutive calls with different inputs through one encoder (on the chip: two batches in flight, test_gpu_final_ac.py)
    out.append(_colour("consecutive_calls", 72, 40, base, [41, 42, 43], SORTED, calls=[[44, 45, 46], [41, 42, 43]]))
    # schedules that must keep the pass: two trellis loops (the tables are reset in front of the second pass, and its kernels write
    # one plane per position), a progressive script, a sequential script of several scans
    out.append(_gray(CS["counts_q92"], extra=dict(trellis_loops=2), fused=False, name="counts_q92_loops2"))
    out.append(_gray(CS["gaps_q92"], extra=dict(baseline=False, fastcrush=True), fused=False, name="gaps_q92_progressive", plain=False))
    out.append(_colour("script_seq_y_cbcr", 72, 40, dict(quality=75, scans=[((0,), 0, 63, 0, 0), ((1, 2), 0, 63, 0, 0)]), [51], fused=False, plain=False))
    return out


JOBS = {j.name: j for j in jobs()}


# ---- running -------------------------------------------------------------------------------------------------------------------------
_oracle = {}


def oracle(job):
    """the oracle's files and expected histograms, and the real reference's files: once per case"""
    if job.name not in _oracle:
        po = job.make(O.make_params)
        sets = [job.frames] + (job.calls or [])
        files, counts, real = [], [], []
        for frames in sets:
            res = [O.encode(po, f, want_taps=True) for f in frames]
            files.append([r[0] for r in res])
            counts.append([expected_counts(po, r[1]) for r in res] if job.plain else None)
            if O.have_ref() and job.ref_kw is not None:
                real.append([O.ref_encode(f, **job.ref_kw)[0] for f in frames])
            else:
                real.append(None)
        _oracle[job.name] = (files, counts, real)
    return _oracle[job.name]


def encode(M, job, knob):
    """the files and final histograms of every call of the case, and whether each call counted inside the trellis kernels"""
    e = dict(job.env)
    e[KNOB] = knob
    with env(**e):
        enc = M.Encoder(job.make(M.make_params), max_batch=len(job.frames))
    try:
        res = []
        for frames in [job.frames] + (job.calls or []):
            files = enc.encode_host(np.stack(frames))
            res.append((files, [enc.final_counts(i).astype(np.int64) for i in range(len(frames))], enc.final_ac_fused()[0]))
        return res
    finally:
        enc.close()


def run(M, name):
    job = JOBS[name]
    want_files, want_counts, real = oracle(job)
    on, off = encode(M, job, None), encode(M, job, 0)
    for c, ((f1, h1, fused1), (f0, h0, fused0)) in enumerate(zip(on, off)):
        assert not fused0, "%s: MJH_FUSE_FINAL_AC=0 still counts in the trellis" % name
        assert fused1 == job.fused, "%s call %d: counted in the trellis: %s, expected %s" % (name, c, fused1, job.fused)
        for i in range(len(f1)):
            where = "%s call %d image %d" % (name, c, i)
            bad = np.argwhere(h1[i] != h0[i])
            assert bad.size == 0, "%s: slot %d symbol 0x%02X counted %d times in the trellis, %d by the pass" % (
                where, bad[0][0], bad[0][1], h1[i][tuple(bad[0])], h0[i][tuple(bad[0])])
            if want_counts[c] is not None:
                for row in (1, 3):
                    bad = np.flatnonzero(h1[i][row] != want_counts[c][i][row])
                    assert bad.size == 0, "%s: AC slot %d symbol 0x%02X counted %d times, the oracle's blocks have %d" % (
                        where, row // 2, bad[0], h1[i][row][bad[0]], want_counts[c][i][row][bad[0]])
            assert f1[i] == f0[i], "%s: the files of the two schedules differ" % where
            assert f1[i] == want_files[c][i], "%s: the file differs from the oracle's (%d vs %d bytes)" % (where, len(f1[i]), len(want_files[c][i]))
            if real[c] is not None:
                assert real[c][i] == f1[i], "%s: the file differs from the real reference's" % where


def check_knobs_are_independent(M):
    """MJH_FUSE_FINAL_AC and MJH_ENCP_GROUPS given together: each encoder takes both as they were set"""
    w, h = 33, 9
    frame = _frame(w, h, 61)
    want = O.encode(O.make_params(w, h, quality=75, baseline=True), frame)
    for knob, groups in ((0, 2), (1, 8), (0, 8), (1, 2)):
        with env(MJH_FUSE_FINAL_AC=knob, MJH_ENCP_GROUPS=groups, MJH_ENC_ONEPASS=None):
            enc = M.Encoder(M.make_params(w, h, quality=75, baseline=True), max_batch=1)
        try:
            got = enc.encode_host(np.stack([frame]))
            assert enc.enc_pack_groups()[0] == groups, (knob, groups, enc.enc_pack_groups())
            assert enc.final_ac_fused()[0] == bool(knob), (knob, groups, enc.final_ac_fused())
            assert got[0] == want, (knob, groups)
        finally:
            enc.close()
