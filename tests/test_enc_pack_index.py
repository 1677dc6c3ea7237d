"""Host only: the index arithmetic of k_enc_write_pack (enc_scan_position_nodiv in mjh_kernels.hip: scan position -> component,
block row and column, the block whose DC is coded and its predecessor's) has no integer division; the library exports the same
inline functions the kernel compiles (mjh_enc_scan_positions).  Compared here with `//` and `%` over every legal geometry:
blocks_per_mcu 1 to 10 from sampling factors 1 to 4, mcus_per_row 1 to 8192, positions up to 8192 MCU rows."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import mozjpeg_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def positions(comps, wib, hib, mpr, p):
    n = len(comps)
    arr = lambda v: (C.c_int * n)(*v)
    p = np.ascontiguousarray(p, dtype=np.int32)
    out = np.empty((len(p), 5), np.int32)
    rc = M.lib().mjh_enc_scan_positions(n, arr([c[0] for c in comps]), arr([c[1] for c in comps]), arr(wib), arr(hib), mpr,
                                        p.ctypes.data_as(C.POINTER(C.c_int)), len(p), out.ctypes.data_as(C.POINTER(C.c_int)))
    assert rc == 0
    return out


def with_divisions(comps, wib, hib, mpr, p):
    """enc_scan_position, mcu_prev_block (no restart interval) and dc_source_block of mjh_device.h, with / and %"""
    p = p.astype(np.int64)
    hs, vs = np.array([c[0] for c in comps]), np.array([c[1] for c in comps])
    blk0 = np.concatenate([[0], np.cumsum(hs * vs)[:-1]])
    bpm = int((hs * vs).sum())
    wib, hib = np.array(wib), np.array(hib)
    mcu, bi = p // bpm, p % bpm
    comp = np.zeros(len(p), np.int64)
    for ci in range(1, len(comps)):
        comp[bi >= blk0[ci]] = ci
    h, v, W, H = hs[comp], vs[comp], wib[comp], hib[comp]
    local = bi - blk0[comp]
    yi, xi = local // h, local % h
    mrow, mcol = mcu // mpr, mcu % mpr
    r, c = mrow * v + yi, mcol * h + xi

    def source(r, c):
        below = r >= H
        c = np.where(below, (c // h) * h + h - 1, c)
        r = np.where(below, H - 1, r)
        return r * W + np.minimum(c, W - 1)

    pm = mcu - 1
    pr = np.where(xi > 0, r, np.where(yi > 0, r - 1, (pm // mpr) * v + v - 1))
    pc = np.where(xi > 0, c - 1, np.where(yi > 0, c + h - 1, (pm % mpr) * h + h - 1))
    has = (xi > 0) | (yi > 0) | (mcu > 0)
    pred = np.where(has, source(np.maximum(pr, 0), np.maximum(pc, 0)), -1)
    return np.stack([comp, r, c, source(r, c), pred], axis=1).astype(np.int32)


def geometries():
    """every multiset of sampling factors that makes 1 to 10 blocks per MCU: one component, and three (luma, two chroma)"""
    hv = [(h, v) for h in range(1, 5) for v in range(1, 5)]
    out = [[a] for a in hv if a[0] * a[1] <= 10]
    out += [[a, b, c] for a, b, c in itertools.product(hv, repeat=3) if a[0] * a[1] + b[0] * b[1] + c[0] * c[1] <= 10]
    out += [[(1, 1)] * 4, [(2, 2), (1, 1), (1, 1), (2, 2)], [(4, 1), (1, 1), (1, 1), (4, 1)]]     # four components
    return out


def sample_positions(rng, bpm, mpr, rows, count):
    """every boundary (first / last block of an MCU, of an MCU row, of the scan; multiples of 256 and their neighbours) and seeded samples"""
    N = bpm * mpr * rows
    edge = [0, 1, bpm - 1, bpm, bpm + 1, bpm * mpr - 1, bpm * mpr, bpm * mpr + 1, N - bpm * mpr - 1, N - bpm * mpr, N - bpm, N - 2, N - 1]
    edge += [k * 256 + d for k in (1, 2, N // 512, N // 256) for d in (-1, 0, 1)]
    edge += [(1 << k) + d for k in range(8, 31) for d in (-1, 0, 1)]
    p = np.concatenate([np.array(edge, np.int64), rng.integers(0, N, count)])
    return np.unique(p[(p >= 0) & (p < N)]).astype(np.int32)


def check(comps, mpr, rows, p, rng):
    hmax, vmax = max(c[0] for c in comps), max(c[1] for c in comps)
    # real blocks: anything from one block to the padded size (the right and bottom MCUs may be mostly dummy blocks)
    wib = [int(rng.integers(max(1, (mpr - 1) * c[0] + 1), mpr * c[0] + 1)) for c in comps]
    hib = [int(rng.integers(max(1, (rows - 1) * c[1] + 1), rows * c[1] + 1)) for c in comps]
    got, want = positions(comps, wib, hib, mpr, p), with_divisions(comps, wib, hib, mpr, p)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (comps, wib, hib, mpr, rows, int(p[bad[0]]), got[bad[0]].tolist(), want[bad[0]].tolist())


def test_small_geometries_exhaustively():
    """every geometry, every mcus_per_row 1..40 and a few MCU rows: every position"""
    rng = np.random.default_rng(20261020)
    for comps in geometries():
        bpm = sum(h * v for h, v in comps)
        for mpr in list(range(1, 41)):
            rows = 1 + (mpr * 7) % 5
            check(comps, mpr, rows, np.arange(bpm * mpr * rows, dtype=np.int32), rng)


def test_every_mcus_per_row():
    """mcus_per_row 1..8192, blocks_per_mcu 1..10 in turn: boundaries and samples of the largest scan (8192 MCU rows)"""
    rng = np.random.default_rng(20261021)
    geo = {}
    for comps in geometries():
        geo.setdefault(sum(h * v for h, v in comps), []).append(comps)
    for mpr in range(1, 8193):
        bpm = 1 + mpr % 10
        comps = geo[bpm][mpr % len(geo[bpm])]
        rows = 8192 if mpr % 3 else int(rng.integers(1, 8193))
        check(comps, mpr, rows, sample_positions(rng, bpm, mpr, rows, 200), rng)


def test_a_million_samples_of_the_largest_scans():
    rng = np.random.default_rng(20261022)
    for comps, mpr in [([(2, 2), (1, 1), (1, 1)], 8192), ([(4, 2), (1, 1), (1, 1)], 8192), ([(1, 1)], 8192), ([(3, 1), (2, 2), (1, 3)], 8191),
                       ([(2, 2), (1, 1), (1, 1)], 4097), ([(1, 1), (1, 1), (1, 1)], 5461), ([(2, 1), (1, 1), (1, 1)], 8190), ([(1, 4), (1, 2), (2, 2)], 6001)]:
        bpm = sum(h * v for h, v in comps)
        check(comps, mpr, 8192, sample_positions(rng, bpm, mpr, 8192, 125000), rng)


def test_the_check_tool_agrees():
    """tools/check_encdiv.py: the multiply-high quotient alone, every divisor and every numerator boundary"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_encdiv.py")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr
