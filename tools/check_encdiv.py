#!/usr/bin/env python3
"""Check of the multiply-high division k_enc_write_pack uses for its scan positions (udiv_m31 / mjh_enc_div_magic in
mjh_kernels.hip): floor(n / d) == (((2 n) * m) >> 32) >> s with s = ceil(log2 d), m = ceil(2^(31 + s) / d), for every divisor the
kernel can meet (blocks_per_mcu 1..10, mcus_per_row 1..8192) -- every n below 2^20, and around every multiple of d that is a
power-of-two fraction of the range, up to 2^31 - 1; m and 2 n must fit 32 bits."""
import numpy as np


def magic(d):
    s = 0
    while (1 << s) < d:
        s += 1
    return ((1 << (31 + s)) + d - 1) // d, s


small = np.arange(0, 1 << 20, dtype=np.uint64)
top = (1 << 31) - 1
for d in range(1, 8193):
    m, s = magic(d)
    assert m < (1 << 32) and (1 << s) >= d
    k = np.unique(np.concatenate([np.uint64(top) >> np.arange(0, 31, dtype=np.uint64), np.arange(1, 4097, dtype=np.uint64) * np.uint64(top // 4097)]))
    q = k // np.uint64(d)
    edges = np.concatenate([q * np.uint64(d), q * np.uint64(d) + np.uint64(d - 1), np.maximum(q * np.uint64(d), np.uint64(1)) - np.uint64(1), np.array([top], np.uint64)])
    n = np.concatenate([small if d <= 10 or d % 64 == 1 or d > 8128 else small[::61], edges[edges <= top]])
    assert np.array_equal((((n << np.uint64(1)) * np.uint64(m)) >> np.uint64(32)) >> np.uint64(s), n // np.uint64(d)), d
print("ok: exact for d = 1..8192, n < 2^31 (boundaries), n < 2^20 (all)")
