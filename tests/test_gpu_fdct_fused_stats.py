"""GPU (-m gpu): the AC statistics fused into the FDCT kernel (k_dct_quant<uint8_t, true, FD>, sequential mode with trellis
quantization).  They run only without debug taps, so the stage checker never sees them: every case here encodes WITHOUT taps and
compares the files with the C restatement (O.encode), with the real reference where oracle/_ref/refenc exists, and with the same
encoder run with set_debug_taps(True) -- the unfused schedule (a k_stats_ac pass over the stored planes).  The fused loop keeps
the position of the previous non-zero coefficient instead of a run counter, retires the lanes beyond the component's last block
once per set of 64 blocks, and clamps the magnitude category instead of the value: the shapes are the smallest at which each of
these can go wrong."""
import numpy as np
import pytest

import mozjpeg_amd as M
import oracle_lib as O

ZZ = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
               28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
               54, 47, 55, 62, 63])     # natural index of zig-zag position k


def three_way(w, h, imgs, **kw):
    """files of the fused schedule == the C restatement == the real reference (where built) == the unfused schedule"""
    po = O.make_params(w, h, **kw)
    want = [O.encode(po, im) for im in imgs]
    enc = M.Encoder(M.make_params(w, h, **kw), max_batch=len(imgs))
    fused = enc.encode_host(np.stack(imgs))
    enc.set_debug_taps(True)
    unfused = enc.encode_host(np.stack(imgs))
    enc.close()
    for i in range(len(imgs)):
        assert fused[i] == want[i], "image %d: fused statistics differ from the restatement (%d vs %d bytes)" % (i, len(fused[i]), len(want[i]))
        assert unfused[i] == fused[i], "image %d: fused and unfused schedules differ" % i
        if O.have_ref():
            assert O.ref_encode(imgs[i], **kw)[0] == fused[i], "image %d: differs from the real reference" % i
    return want


def noise(w, h, seed, hi=256):
    return np.random.default_rng(seed).integers(0, hi, (h, w, 3), dtype=np.uint8)


# ---- ragged block counts: tail lanes, and the break between the four sets of a wave -------------------------------------------
# noise content: every block has its own symbols, a tail lane (it redoes the last block) counted once too often moves the tables
@pytest.mark.gpu
@pytest.mark.parametrize("w,h,sample", [(8, 8, (1, 1)),          # one block: 63 tail lanes
                                        (136, 128, (1, 1)),      # 272 = 256 + 16 blocks: a second wave with one partial set
                                        (200, 120, (2, 2)),      # 375 luma blocks (a wave of 1 full + 1 partial set), 104 chroma
                                        (512, 32, (1, 1))],      # exactly 256: one whole wave, no tail lane
                         ids=["8x8", "136x128_444", "200x120_420", "512x32_444"])
def test_ragged_block_counts(w, h, sample):
    three_way(w, h, [noise(w, h, 11 * w + h)], quality=75, baseline=True, sample=sample)


# ---- dictated runs ------------------------------------------------------------------------------------------------------------
def basis_block(q_nat, positions):
    """8x8 samples whose DCT is one quantizer step at each of the zig-zag positions given and (to within the rounding of the
    samples, far below half a step) nothing elsewhere"""
    x = np.arange(8)
    c = np.cos((2 * x[:, None] + 1) * np.arange(8)[None, :] * np.pi / 16)       # [sample, frequency]
    a = np.where(np.arange(8) == 0, np.sqrt(0.5), 1.0)
    blk = np.full((8, 8), 128.0)
    for k in positions:
        n = int(ZZ[k])
        v, u = divmod(n, 8)
        blk += float(q_nat[n]) * 0.25 * a[u] * a[v] * np.outer(c[:, v], c[:, u])
    assert blk.min() >= 0 and blk.max() <= 254, "pattern leaves the sample range (or would take the deringing path)"
    return np.rint(blk).astype(np.uint8)


# zig-zag positions of the non-zero AC coefficients of each dictated block
PATTERNS = [[63],                                     # 62 zeros in front: three ZRLs, no end-of-block
            [1, 63],                                  # 61 zeros between: three ZRLs
            [1, 17], [1, 18], [1, 33], [1, 34], [1, 49], [1, 50],      # gaps of exactly 15, 16, 31, 32, 47, 48 zeros
            [16], [17], [32], [33], [48], [49],       # the same runs counted from the start of the block
            [62],                                     # last non-zero at 62: end-of-block
            [5, 63],                                  # last non-zero at 63: none
            []]                                       # all-zero AC: end-of-block alone


@pytest.mark.gpu
def test_dictated_runs_in_a_wave_of_ordinary_blocks():
    w, h, kw = 136, 64, dict(quality=50, baseline=True, gray=True, grayin=True)       # 17 x 8 = 136 blocks: two sets and a partial one
    po = O.make_params(w, h, **kw)
    q_nat = np.array(po.qtbl[po.quant_tbl_no[0]][:], dtype=np.int64)
    rng = np.random.default_rng(5)
    img = np.clip(128 + rng.normal(0, 40, (h, w)), 0, 254).astype(np.uint8)           # the ordinary blocks
    where = {}
    for i, pos in enumerate(PATTERNS):
        b = 3 + 7 * i                                  # blocks 3, 10, ..., 115: lanes of both full sets, ordinary blocks between
        by, bx = divmod(b, 17)
        img[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = basis_block(q_nat, pos)
        where[(by, bx)] = pos
    # the fixture is what it claims: the restatement's conventionally quantized (pre-trellis) coefficients of each dictated
    # block are non-zero at exactly the intended zig-zag positions
    _, taps = O.encode(po, img[..., None], want_taps=True)
    q0 = taps[("coef_q0", 0)]
    for (by, bx), pos in where.items():
        got = [k for k in range(1, 64) if q0[by, bx, ZZ[k]] != 0]
        assert got == pos, "block (%d, %d): non-zeros at %s, intended %s" % (by, bx, got, pos)
    ordinary = [int(np.count_nonzero(q0[by, bx, 1:])) for by in range(8) for bx in range(17) if (by, bx) not in where]
    assert min(ordinary) > 0 and max(ordinary) > 10
    three_way(w, h, [img[..., None]], **kw)


@pytest.mark.gpu
def test_dictated_runs_alone_decide_their_image_s_table():
    """One small image per pattern, all in one batch: the dictated block between two smooth ones (a few low positions, no run
    of 16).  Each image has a histogram of its own, so the pattern's symbols -- its ZRLs, its end-of-block -- are a large share
    of the counts its trellis' rate table is made from, where the 136-block frame above would bury one miscounted symbol."""
    w, h, kw = 24, 8, dict(quality=50, baseline=True, gray=True, grayin=True)
    po = O.make_params(w, h, **kw)
    q_nat = np.array(po.qtbl[po.quant_tbl_no[0]][:], dtype=np.int64)
    imgs = []
    for i, pos in enumerate(PATTERNS):
        img = np.empty((h, w), np.uint8)
        img[:, 0:8] = basis_block(q_nat, [1, 2, 4])
        img[:, 8:16] = basis_block(q_nat, pos)
        img[:, 16:24] = basis_block(q_nat, [1, 3, 5, 6])
        _, taps = O.encode(po, img[..., None], want_taps=True)
        q0 = taps[("coef_q0", 0)]
        assert [[k for k in range(1, 64) if q0[0, b, ZZ[k]] != 0] for b in range(3)] == [[1, 2, 4], pos, [1, 3, 5, 6]], pos
        imgs.append(img[..., None])
    three_way(w, h, imgs, **kw)


# ---- large magnitudes ---------------------------------------------------------------------------------------------------------
def _category(v):
    return int(v).bit_length()


@pytest.mark.gpu
@pytest.mark.parametrize("noovershoot", [False, True], ids=["deringing", "noovershoot"])
def test_large_magnitudes(noovershoot):
    """Quality 100 (every step 1): a 0/255 checkerboard (the 7,7 basis' sign pattern) and, beside it, the sign pattern of the 4,4
    basis in both polarities, whose coefficient is the largest that 8-bit samples can give an AC position
    (0.25 * (4 / sqrt 2)^2 * 127.5 = 1020).  Without deringing no AC coefficient reaches 1024 and nothing is clamped (the clamp is
    part of the deringing switch): category 10 is the natural top.  With deringing the overshoot lifts the saturated samples and the
    4,4 coefficient quantizes to 1028 -- category 11 -- which the reference clamps to 1023, category 10: the clamp IS reachable with
    8-bit samples, and this block is where clamping the category instead of the value has to give the same symbol.  Both facts
    are asserted from the restatement's coefficients."""
    w, h = 32, 16
    yy, xx = np.mgrid[0:h, 0:w]
    g = np.where((xx + yy) % 2 == 0, 0, 255).astype(np.uint8)                        # blocks 0..3, 4..5: checkerboard
    s44 = np.sign(np.outer(np.cos((2 * np.arange(8) + 1) * 4 * np.pi / 16), np.cos((2 * np.arange(8) + 1) * 4 * np.pi / 16)))
    g[8:16, 16:24] = np.where(s44 > 0, 255, 0)
    g[8:16, 24:32] = np.where(s44 > 0, 0, 255)
    kw = dict(quality=100, baseline=True, gray=True, grayin=True, noovershoot=noovershoot)
    po = O.make_params(w, h, **kw)
    _, taps = O.encode(po, g[..., None], want_taps=True)
    q0 = np.abs(taps[("coef_q0", 0)][:2, :4].astype(np.int64))[..., 1:]
    unclamped = (np.abs(taps[("coef_uq", 0)][:2, :4].astype(np.int64))[..., 1:] + 4) // 8        # every step is 1: (|x| + 4q) / 8q
    top, top_unclamped = int(q0.max()), int(unclamped.max())
    print("largest pre-trellis AC magnitude: %d (category %d), before the clamp %d (category %d)"
          % (top, _category(top), top_unclamped, _category(top_unclamped)))
    assert int(q0[0, 0, 62]) > 512                                                   # the checkerboard's own coefficient (7,7): category 10
    if noovershoot:
        assert top == top_unclamped == 1020
    else:
        assert top == 1023 and _category(top) == 10 and top_unclamped >= 1024 and _category(top_unclamped) == 11
    three_way(w, h, [g[..., None]], **kw)


# ---- a batch: the per-image histograms stay apart -----------------------------------------------------------------------------
@pytest.mark.gpu
def test_batch_of_three_different_images():
    w, h = 72, 40                                       # 45 luma blocks: every wave has tail lanes
    imgs = [noise(w, h, 1), O.synthetic_frame(w, h, 2), np.clip(noise(w, h, 3, 64) + np.uint8(100), 0, 255).astype(np.uint8)]
    want = three_way(w, h, imgs, quality=75, baseline=True)
    assert len(set(want)) == 3


# ---- deringing in some lanes of a wave only -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_isolated_saturated_pixels():
    w, h = 96, 64                                       # 96 luma blocks
    img = np.clip(O.synthetic_frame(w, h, 9).astype(np.int32), 0, 250).astype(np.uint8)
    for (y, x) in [(3, 5), (12, 40), (13, 41), (30, 77), (63, 95), (40, 0)]:
        img[y, x] = 255                                 # a handful of blocks take the deringing pass, their neighbours do not
    three_way(w, h, [img], quality=75, baseline=True, sample=(1, 1))


# ---- the statistics arm without the fast division -----------------------------------------------------------------------------
@pytest.mark.gpu
def test_steps_above_255_take_the_general_statistics_arm():
    """k_dct_quant<uint8_t, true, false>: sequential mode, trellis, 8-bit samples, a quantizer step above 255 -- a sequential scan
    script without -baseline (16-bit tables) at a low quality"""
    w, h = 200, 120
    kw = dict(quality=5, scans=[((0,), 0, 63, 0, 0), ((1, 2), 0, 63, 0, 0)])
    po = O.make_params(w, h, **kw)
    assert max(po.qtbl[0][:]) > 255 and po.trellis_quant
    three_way(w, h, [noise(w, h, 21)], **kw)
