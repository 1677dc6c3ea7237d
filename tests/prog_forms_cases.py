"""Shared by test_simt_prog_forms.py (CPU suite, emulator) and test_gpu_prog_forms.py (-m gpu): the three forms of the
progressive entropy coder in mjh_prog.hip, each of which restates the same pieces of jcphuff.c --
  records : the parallel chain over the AC trellis' compact records (the default profile),
  planes  : the parallel chain over one-plane-per-position coefficients (notrellis),
  ordered : the ordered walk k_prog_scan (restart intervals).
Every case compares byte for byte against the oracle computed here, never against another form of the library.

The frame is 376 x 368.  At 1 x 1 sampling that is 47 x 46 = 2162 blocks: two 2048-block chunks, the second holding 114 blocks (one
full wave and one of 50 lanes) -- the smallest frame with a chunk border, a ragged last wave and room for this content:
  block rows  0-20  seeded noise: at q95 a block of a refinement scan buffers more than 32 correction bits;
  block rows 21-39  a sparse texture: one high-frequency basis function per block (or none), so a band holds runs longer than
                    15 zeros (ZRL) and short EOB runs between the blocks;
  block rows 40-44  flat, full width: more than 64 consecutive empty blocks (whole empty waves); the EOB run crosses block 2048
                    in row 43, i.e. the chunk border (carry_p / next_after);
  block row  45     noise again: the run is flushed inside the second chunk.
A second, entirely flat frame rides in the same batch: every wave empty and the run still pending at the end of the scan."""
import functools

import numpy as np

import mozjpeg_amd as M
import oracle_lib as O

W, H = 376, 368
QUALITIES = (75, 95)
SAMPLINGS = {"gray": dict(gray=True), "444": dict(sample=(1, 1)), "420": dict(sample=(2, 2))}
FORMS = {"records": dict(), "planes": dict(notrellis=True), "ordered": dict(restart=1)}

# (id, parameters): scan search (its Al choice per image) and the fixed script, every form, every sampling
CASES = []
for _form, _fkw in FORMS.items():
    for _samp, _skw in SAMPLINGS.items():
        for _q in QUALITIES:
            CASES.append(("%s_%s_q%d_search" % (_form, _samp, _q), dict(_fkw, quality=_q, **_skw)))
            CASES.append(("%s_%s_q%d_fastcrush" % (_form, _samp, _q), dict(_fkw, quality=_q, fastcrush=True, **_skw)))
    # the non-interleaved DC scans (one component each), once per form
    CASES.append(("%s_420_q75_dcscanopt2" % _form, dict(_fkw, quality=75, dc_scan_opt=2, **SAMPLINGS["420"])))
# libjpeg's own script (jpeg_simple_progression as -revert writes it): DC with Al = 1 and its refinement scan, AC refinement scans
# over the whole band 1..63, where a noise block at q95 buffers more than 32 correction bits.  No trellis there, so no records
for _form, _fkw in (("planes", dict()), ("ordered", dict(restart=1))):
    for _samp in ("gray", "420"):
        for _q in QUALITIES:
            CASES.append(("%s_%s_q%d_libjpeg_script" % (_form, _samp, _q), dict(_fkw, quality=_q, revert=True, progressive=True, **SAMPLINGS[_samp])))
CASE_IDS = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def frames():
    rng = np.random.default_rng(376368)
    img = np.empty((H, W, 3), np.uint8)
    img[:21 * 8] = rng.integers(0, 256, (21 * 8, W, 3), dtype=np.uint8)
    # one basis function cos((2x+1) u pi/16) cos((2y+1) v pi/16) of high frequency per block and channel, a third of the blocks flat
    t = (2 * np.arange(8) + 1) * np.pi / 16
    for br in range(21, 40):
        for bc in range(W // 8):
            blk = np.full((8, 8, 3), 128.0)
            if rng.integers(0, 3):
                for c in range(3):
                    u, v = (int(k) for k in rng.integers(5, 8, 2))
                    blk[..., c] += float(rng.integers(20, 100)) * np.outer(np.cos(v * t), np.cos(u * t))
            img[br * 8:br * 8 + 8, bc * 8:bc * 8 + 8] = np.clip(np.rint(blk), 0, 255).astype(np.uint8)
    img[40 * 8:45 * 8] = 93
    img[45 * 8:] = rng.integers(0, 256, (8, W, 3), dtype=np.uint8)
    out = np.stack([img, np.full_like(img, 77)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(cid):
    kw = CASES[CASE_IDS.index(cid)][1]
    po = O.make_params(W, H, **kw)
    return tuple(O.encode(po, f) for f in frames())


def check_case(cid):
    kw = CASES[CASE_IDS.index(cid)][1]
    fr = frames()
    enc = M.Encoder(M.make_params(W, H, **kw), max_batch=len(fr))
    got = enc.encode_host(fr)
    enc.close()
    want = expected(cid)
    for i in range(len(fr)):
        assert bytes(got[i]) == want[i], "frame %d differs from the oracle" % i
