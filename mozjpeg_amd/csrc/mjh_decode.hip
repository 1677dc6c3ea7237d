// mjh_decode.hip -- K-D: Huffman decoding of sequential JPEG files on the device (mjh_transcode_host): the front half of the
// "jpegrescan" path.  Input: the files as they are + per (image, scan) / restart segment descriptors the host made from the
// marker segments.  Output: the pipeline's quantized coefficient planes (coefficient-major, zig-zag order, real blocks only:
// what k_import_coefs leaves) and a per-image status.  Semantics: decode_mcu_slow (jdhuff.c:560-650) + jdcoefct.c.
//
// Parallelism: restart segments are independent; inside a segment, self-synchronising subsequences (Klein & Wiseman 2003;
// Weissenberger & Schmidt 2018): every lane decodes S bytes from a guessed state, then lanes walk on into the following
// subsequences -- one subsequence per launch -- until the state they arrive with is the one recorded there.  No launch waits
// for another workgroup; a round extends the correctly decoded prefix of every segment by at least one subsequence.
// Every read is bounded by the segment's length and every store by the component's block count, whatever the bytes say.
//
// Lossless transforms (transupp.c's flips, rotations, transpositions, trim, crop, grayscale) are fused into the stores: k_dec_store_x
// and k_dec_dc_x decode in the source frame's geometry and write every coefficient to its place in the destination frame (MjhXform).
#include <hip/hip_runtime.h>
#include "mjh_device.h"
#include "mjh_decode.h"
#include "mjh_decode_dev.h"

// Where block (row, col) of a source component goes in the destination frame (-1: trimmed or cropped away, or the component is
// dropped) and, in cls, whether it was mirrored in x (1) / y (2).  The inverse of the do_* routines of transupp.c, which exists
// because each of them permutes the blocks it keeps.  The result is checked against the destination's block grid whatever
// the descriptors say.
__device__ __forceinline__ int dec_xf_block(const MjhXform &X, const MjhXformComp &xc, int row, int col, unsigned &cls)
{
  int x = X.transpose ? row : col, y = X.transpose ? col : row;
  cls = 0;
  if (X.mirror_x && x < xc.cw) { x = xc.cw - 1 - x; cls |= 1u; }
  if (X.mirror_y && y < xc.ch) { y = xc.ch - 1 - y; cls |= 2u; }
  x -= xc.xcb; y -= xc.ycb;
  if (x < 0 || y < 0 || x >= xc.wib || y >= xc.hib) return -1;
  const int blk = y * xc.wib + x;
  return blk < xc.nblk ? blk : -1;
}

// Decodes from (p, k, b) while the next code word starts in front of end_bits.  STORE: also while ord < total (the segment's
// blocks), coefficients and DC differences written; returns true when the segment's last block was completed here.
template <bool STORE, bool XF = false>
__device__ __forceinline__ bool dec_run(const MjhComp *lc, const MjhDecScan &sc, const MjhDecTable *T, DecReader &R, unsigned end_bits,
                                        unsigned &p, int &k, int &b, unsigned &n, unsigned ord, unsigned total, int mcu,
                                        int16_t *coef_img, int16_t *diff_img, unsigned &flags, int lim, const MjhXform *X = nullptr)
{
  DecWhere wh{ 0, -1, 0 };
  unsigned cls = 0;
  // XF: wh.blk becomes the block's index in the DESTINATION component
  auto remap = [&]() {
    if (XF && wh.blk >= 0) { const int wib = lc[wh.j].wib, row = wh.blk / wib; wh.blk = dec_xf_block(*X, X->c[sc.comp[wh.j]], row, wh.blk - row * wib, cls); }
  };
  int j = 0;
  {
    int t = b;
    while (j < sc.ncomp - 1 && t >= sc.nb[j]) { t -= sc.nb[j]; j++; }
  }
  if (STORE) { wh = dec_locate(lc, sc, mcu, b); remap(); }
  bool bad = false;
  while (p < end_bits) {
    if (STORE && ord >= total) break;
    const unsigned long long w = R.fetch(p);
    int nb;
    bool done = false;
    if (k == 0) {
      const int s = dec_symbol(T[2 * j], w, nb, bad) & 15;
      if (STORE) {
        int diff = 0;
        if (s) {
          const int r = (int)((w << nb) >> (64 - s));
          diff = r < (1 << (s - 1)) ? r - (1 << s) + 1 : r;       // HUFF_EXTEND
        }
        diff_img[wh.m] = (int16_t)diff;
      }
      p = R.advance(p, nb + s);
      k = 1;
    } else {
      const int sym = dec_symbol(T[2 * j + 1], w, nb, bad);
      const int r = sym >> 4, s = sym & 15;
      if (s) {
        k += r;
        if (STORE) {
          const int v = (int)((w << nb) >> (64 - s));
          const int val = v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
          if (val > lim || val < -lim) flags |= MJH_DEC_BADCOEF;
          // a run that passes position 63 lands in the spare entries of jpeg_natural_order, all 63 (jdhuff.c:619-628)
          if (XF) {
            if (wh.blk >= 0) {
              const MjhXformComp &xc = X->c[sc.comp[j]];
              const int kk = k > 63 ? 63 : k, kd = X->transpose ? (int)X->zz_t[kk] : kk;
              const bool neg = (((cls & 1u) && ((X->odd_col >> kd) & 1ull)) != ((cls & 2u) && ((X->odd_row >> kd) & 1ull)));
              coef_img[xc.coef_off + (long long)kd * xc.kstride + wh.blk] = (int16_t)(neg ? -val : val);
            }
          } else
          if (wh.blk >= 0) coef_img[lc[j].coef_off + (long long)(k > 63 ? 63 : k) * lc[j].kstride + wh.blk] = (int16_t)val;
        }
        p = R.advance(p, nb + s);
        k++;
        done = k >= 64;
      } else {
        p = R.advance(p, nb);
        if (r == 15) { k += 16; done = k >= 64; }
        else done = true;
      }
    }
    if (done) {
      n++;
      k = 0;
      b++;
      if (b >= sc.bpm) { b = 0; j = 0; mcu++; }
      else { int t = b; j = 0; while (j < sc.ncomp - 1 && t >= sc.nb[j]) { t -= sc.nb[j]; j++; } }
      if (STORE) {
        ord++;
        if (ord >= total) { if (bad) flags |= MJH_DEC_CORRUPT; return true; }
        wh = dec_locate(lc, sc, mcu, b);
        remap();
      }
    }
  }
  if (STORE && bad) flags |= MJH_DEC_CORRUPT;
  return false;
}

__global__ void __launch_bounds__(MJH_DEC_WG)
k_dec_sync(MjhConst C, MjhDecBatch B, int q, int first)
{
  __shared__ MjhDecScan sc;
  __shared__ MjhDecTable T[2 * MJH_MAXC];
  __shared__ MjhComp lc[MJH_MAXC];
  if (!first && q > 0 && B.changed[q - 1] == 0u) return;      // (uniform: the round before this one changed nothing)
  const unsigned g = blockIdx.x * MJH_DEC_WG + threadIdx.x;
  const unsigned sg0 = B.sub_seg[blockIdx.x * MJH_DEC_WG];
  dec_load_scan(C, B, B.segs[sg0].scan, &sc, T, lc);
  const unsigned sg = B.sub_seg[g];
  if (sg == 0xFFFFFFFFu) return;
  const MjhDecSeg seg = B.segs[sg];
  const unsigned i = g - (unsigned)seg.sub0, S = (unsigned)B.S;
  DecReader R;
  R.d = B.bytes + seg.off;
  R.len = seg.len;
  unsigned p, n = 0, flags = 0;
  int k, b;
  unsigned j;
  if (first) {
    p = dec_sub_start(R.d, R.len, i, S) * 8u;
    k = 0; b = 0;
    j = i;
  } else {
    const MjhDecCarry c = B.carry[g];
    if (!c.active) return;
    p = c.p; k = (int)(c.kb & 0xFFu); b = (int)(c.kb >> 8);
    j = (unsigned)c.next;
  }
  (void)dec_run<false>(lc, sc, T, R, dec_sub_end_bits(R.len, j, (unsigned)seg.nsub, S), p, k, b, n, 0u, 0u, 0, nullptr, nullptr, flags, 0);
  b = sc.canon[b];
  const unsigned kb = (unsigned)k | ((unsigned)b << 8);
  MjhDecState *st = B.state + seg.sub0 + j;
  bool same = false;
  if (!first) { const MjhDecState old = *st; same = old.p == p && old.kb == kb; }
  st->p = p; st->kb = kb; st->n = n; st->pad = 0;          // (the lane that comes from further back knows the entry state better: its count stands)
  MjhDecCarry c;
  c.p = p; c.kb = kb; c.next = (int)j + 1;
  c.active = (!same && j + 1 < (unsigned)seg.nsub) ? 1 : 0;
  B.carry[g] = c;
  if (!first && !same) B.changed[q] = 1u;
}

// block index of every subsequence's first unfinished block: exclusive prefix sum of the counts over the segment
__global__ void __launch_bounds__(64)
k_dec_prefix(MjhDecBatch B)
{
  __shared__ unsigned sh[64];
  const MjhDecSeg seg = B.segs[blockIdx.x];
  unsigned base = 0;
  for (int c0 = 0; c0 < seg.nsub; c0 += 64) {
    const int i = c0 + (int)threadIdx.x;
    const unsigned v = i < seg.nsub ? B.state[seg.sub0 + i].n : 0u;
    sh[threadIdx.x] = v;
    __syncthreads();
    unsigned inc = v;
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned a = (int)threadIdx.x >= o ? sh[threadIdx.x - o] : 0u;
      __syncthreads();
      inc += a;
      sh[threadIdx.x] = inc;
      __syncthreads();
    }
    if (i < seg.nsub) B.ord[seg.sub0 + i] = base + inc - v;
    base += sh[63];
    __syncthreads();
  }
}

// every subsequence again from its now known entry state, storing
__global__ void __launch_bounds__(MJH_DEC_WG)
k_dec_store(MjhConst C, MjhDecBatch B, int16_t *__restrict__ coef_q)
{
  __shared__ MjhDecScan sc;
  __shared__ MjhDecTable T[2 * MJH_MAXC];
  __shared__ MjhComp lc[MJH_MAXC];
  const unsigned g = blockIdx.x * MJH_DEC_WG + threadIdx.x;
  const unsigned sg0 = B.sub_seg[blockIdx.x * MJH_DEC_WG];
  dec_load_scan(C, B, B.segs[sg0].scan, &sc, T, lc);
  const unsigned sg = B.sub_seg[g];
  if (sg == 0xFFFFFFFFu) return;
  const MjhDecSeg seg = B.segs[sg];
  const unsigned i = g - (unsigned)seg.sub0, S = (unsigned)B.S;
  DecReader R;
  R.d = B.bytes + seg.off;
  R.len = seg.len;
  unsigned p = 0, n = 0, flags = 0;
  int k = 0, b = 0;
  if (i > 0) { const MjhDecState e = B.state[g - 1]; p = e.p; k = (int)(e.kb & 0xFFu); b = (int)(e.kb >> 8); }
  const unsigned ord = B.ord[g], total = (unsigned)seg.nmcu * (unsigned)sc.bpm;
  const bool last = i + 1 == (unsigned)seg.nsub;
  if (ord < total) {
    // (the entry state's b is ord mod bpm whenever the chain of states is the true one; a damaged stream may leave anything: the
    //  block index decides where stores go, the state only how the bits are read)
    b = (int)(ord % (unsigned)sc.bpm);
    const int mcu = seg.mcu0 + (int)(ord / (unsigned)sc.bpm);
    const bool fin = dec_run<true>(lc, sc, T, R, dec_sub_end_bits(R.len, i, (unsigned)seg.nsub, S), p, k, b, n, ord, total, mcu,
                                   coef_q + (size_t)sc.image * C.coefs_per_image, B.diff + (size_t)sc.image * C.total_mcu_blocks, flags, B.coef_limit);
    if (fin) {
      // the last block ends here: nothing but the padding of its last byte may follow (jdmarker.c next_marker: "extraneous bytes"),
      // and it must not have read past the end ("Premature end of JPEG file" / JWRN_HIT_MARKER)
      unsigned nbp = p >> 3;
      if (p & 7u) { const unsigned byte = nbp < R.len ? (unsigned)R.d[nbp] : 0u; nbp += 1u + (byte == 0xFFu ? 1u : 0u); }
      if (p > R.len * 8u || nbp < R.len) flags |= MJH_DEC_CORRUPT;
    } else if (last) flags |= MJH_DEC_CORRUPT;               // the data ends in front of the segment's last block
  } else if (i == 0) flags |= MJH_DEC_CORRUPT;
  if (flags) atomicOr(&B.status[sc.image], flags);
}

// the descriptor of the transform into LDS: lanes index its tables by their own k
__device__ __forceinline__ void dec_load_xform(const MjhXform *Xg, MjhXform *X)
{
  const unsigned *src = reinterpret_cast<const unsigned *>(Xg);
  unsigned *dst = reinterpret_cast<unsigned *>(X);
  for (unsigned i = threadIdx.x; i < sizeof(MjhXform) / 4; i += MJH_DEC_WG) dst[i] = src[i];
  __syncthreads();
}

// k_dec_store with a transform: C = the SOURCE frame's geometry, the stores go where *Xg says (the destination's planes)
__global__ void __launch_bounds__(MJH_DEC_WG)
k_dec_store_x(MjhConst C, MjhDecBatch B, int16_t *__restrict__ coef_q, const MjhXform *__restrict__ Xg)
{
  __shared__ MjhDecScan sc;
  __shared__ MjhDecTable T[2 * MJH_MAXC];
  __shared__ MjhComp lc[MJH_MAXC];
  __shared__ MjhXform X;
  dec_load_xform(Xg, &X);
  const unsigned g = blockIdx.x * MJH_DEC_WG + threadIdx.x;
  const unsigned sg0 = B.sub_seg[blockIdx.x * MJH_DEC_WG];
  dec_load_scan(C, B, B.segs[sg0].scan, &sc, T, lc);
  const unsigned sg = B.sub_seg[g];
  if (sg == 0xFFFFFFFFu) return;
  const MjhDecSeg seg = B.segs[sg];
  const unsigned i = g - (unsigned)seg.sub0, S = (unsigned)B.S;
  DecReader R;
  R.d = B.bytes + seg.off;
  R.len = seg.len;
  unsigned p = 0, n = 0, flags = 0;
  int k = 0, b = 0;
  if (i > 0) { const MjhDecState e = B.state[g - 1]; p = e.p; k = (int)(e.kb & 0xFFu); b = (int)(e.kb >> 8); }
  const unsigned ord = B.ord[g], total = (unsigned)seg.nmcu * (unsigned)sc.bpm;
  const bool last = i + 1 == (unsigned)seg.nsub;
  if (ord < total) {
    // (the entry state's b is ord mod bpm whenever the chain of states is the true one; a damaged stream may leave anything: the
    //  block index decides where stores go, the state only how the bits are read)
    b = (int)(ord % (unsigned)sc.bpm);
    const int mcu = seg.mcu0 + (int)(ord / (unsigned)sc.bpm);
    const bool fin = dec_run<true, true>(lc, sc, T, R, dec_sub_end_bits(R.len, i, (unsigned)seg.nsub, S), p, k, b, n, ord, total, mcu,
                                   coef_q + (size_t)sc.image * X.coefs_per_image, B.diff + (size_t)sc.image * C.total_mcu_blocks, flags, B.coef_limit, &X);
    if (fin) {
      // the last block ends here: nothing but the padding of its last byte may follow (jdmarker.c next_marker: "extraneous bytes"),
      // and it must not have read past the end ("Premature end of JPEG file" / JWRN_HIT_MARKER)
      unsigned nbp = p >> 3;
      if (p & 7u) { const unsigned byte = nbp < R.len ? (unsigned)R.d[nbp] : 0u; nbp += 1u + (byte == 0xFFu ? 1u : 0u); }
      if (p > R.len * 8u || nbp < R.len) flags |= MJH_DEC_CORRUPT;
    } else if (last) flags |= MJH_DEC_CORRUPT;               // the data ends in front of the segment's last block
  } else if (i == 0) flags |= MJH_DEC_CORRUPT;
  if (flags) atomicOr(&B.status[sc.image], flags);
}

// DC values = per component and restart segment the running sum of the stored differences (dummy blocks take part, jdhuff.c:588-592)
__global__ void __launch_bounds__(MJH_DEC_WG)
k_dec_dc(MjhConst C, MjhDecBatch B, int16_t *__restrict__ coef_q)
{
  __shared__ int s_sum[MJH_DEC_WG];
  __shared__ int s_rst[MJH_DEC_WG];
  const MjhDecScan *scp = B.scans + blockIdx.y;        // (uniform: read through scalar loads, no private copy)
  const int j = blockIdx.x, ncomp = scp->ncomp;
  if (j >= ncomp) return;
  const int mcus = scp->mcus, mpr = scp->mcus_per_row, image = scp->image;
  long long doff = scp->diff_off;
  for (int t = 0; t < j; t++) doff += (long long)scp->nb[t] * mcus;
  const MjhComp cc = C.c[scp->comp[j]];
  const int nbj = scp->nb[j];
  const int N = mcus * nbj, L = scp->ri * nbj;     // blocks of the component in the scan / per restart segment
  const int per = (N + MJH_DEC_WG - 1) / MJH_DEC_WG;
  const int m0 = per * (int)threadIdx.x < N ? per * (int)threadIdx.x : N, m1 = m0 + per < N ? m0 + per : N;
  const int16_t *diff = B.diff + (size_t)image * C.total_mcu_blocks + doff;
  int sum = 0, rst = 0;
  {
    int ph = m0 % L;
    for (int m = m0; m < m1; m++) {
      if (ph == 0) { sum = 0; rst = 1; }
      sum += diff[m];
      if (++ph == L) ph = 0;
    }
  }
  s_sum[threadIdx.x] = sum; s_rst[threadIdx.x] = rst;
  __syncthreads();
  int pred = 0;
  for (int t = 0; t < (int)threadIdx.x; t++) pred = s_rst[t] ? s_sum[t] : pred + s_sum[t];
  int16_t *dc = coef_q + (size_t)image * C.coefs_per_image + cc.coef_off;
  int ph = m0 % L;
  int mcu = m0 / nbj, t = m0 - mcu * nbj;
  int my = mcu / mpr, mx = mcu - my * mpr;
  for (int m = m0; m < m1; m++) {
    if (ph == 0) pred = 0;
    pred += diff[m];
    int blk;
    if (ncomp == 1) blk = m;
    else {
      const int by = t / cc.h, bx = t - by * cc.h;
      const int row = my * cc.v + by, col = mx * cc.h + bx;
      blk = (row < cc.hib && col < cc.wib) ? row * cc.wib + col : -1;
    }
    if (blk >= 0 && blk < cc.nblk) dc[blk] = (int16_t)pred;
    if (++ph == L) ph = 0;
    if (++t == nbj) { t = 0; if (++mx == mpr) { mx = 0; my++; } }
  }
}

// k_dec_dc with a transform: C = the SOURCE frame's geometry (the prediction chain is the source's, dummy blocks included); only the
// final store is mapped
__global__ void __launch_bounds__(MJH_DEC_WG)
k_dec_dc_x(MjhConst C, MjhDecBatch B, int16_t *__restrict__ coef_q, const MjhXform *__restrict__ X)
{
  __shared__ int s_sum[MJH_DEC_WG];
  __shared__ int s_rst[MJH_DEC_WG];
  const MjhDecScan *scp = B.scans + blockIdx.y;        // (uniform: read through scalar loads, no private copy)
  const int j = blockIdx.x, ncomp = scp->ncomp;
  if (j >= ncomp) return;
  const MjhXformComp xc = X->c[scp->comp[j]];
  if (xc.nblk == 0) return;      // (uniform: a dropped component)
  const int mcus = scp->mcus, mpr = scp->mcus_per_row, image = scp->image;
  long long doff = scp->diff_off;
  for (int t = 0; t < j; t++) doff += (long long)scp->nb[t] * mcus;
  const MjhComp cc = C.c[scp->comp[j]];
  const int nbj = scp->nb[j];
  const int N = mcus * nbj, L = scp->ri * nbj;     // blocks of the component in the scan / per restart segment
  const int per = (N + MJH_DEC_WG - 1) / MJH_DEC_WG;
  const int m0 = per * (int)threadIdx.x < N ? per * (int)threadIdx.x : N, m1 = m0 + per < N ? m0 + per : N;
  const int16_t *diff = B.diff + (size_t)image * C.total_mcu_blocks + doff;
  int sum = 0, rst = 0;
  {
    int ph = m0 % L;
    for (int m = m0; m < m1; m++) {
      if (ph == 0) { sum = 0; rst = 1; }
      sum += diff[m];
      if (++ph == L) ph = 0;
    }
  }
  s_sum[threadIdx.x] = sum; s_rst[threadIdx.x] = rst;
  __syncthreads();
  int pred = 0;
  for (int t = 0; t < (int)threadIdx.x; t++) pred = s_rst[t] ? s_sum[t] : pred + s_sum[t];
  int16_t *dc = coef_q + (size_t)image * X->coefs_per_image + xc.coef_off;
  int ph = m0 % L;
  int mcu = m0 / nbj, t = m0 - mcu * nbj;
  int my = mcu / mpr, mx = mcu - my * mpr;
  for (int m = m0; m < m1; m++) {
    if (ph == 0) pred = 0;
    pred += diff[m];
    int blk;
    if (ncomp == 1) blk = m;
    else {
      const int by = t / cc.h, bx = t - by * cc.h;
      const int row = my * cc.v + by, col = mx * cc.h + bx;
      blk = (row < cc.hib && col < cc.wib) ? row * cc.wib + col : -1;
    }
    if (blk >= 0 && blk < cc.nblk) {
      unsigned cls;
      const int row = blk / cc.wib;
      blk = dec_xf_block(*X, xc, row, blk - row * cc.wib, cls);
      if (blk >= 0) dc[blk] = (int16_t)pred;
    }
    if (++ph == L) ph = 0;
    if (++t == nbj) { t = 0; if (++mx == mpr) { mx = 0; my++; } }
  }
}

// a damaged image continues through the schedule as zeroed blocks; its status goes where the coefficient checks report
__global__ void __launch_bounds__(256)
k_dec_scrub(MjhConst C, MjhDecBatch B, int16_t *__restrict__ coef_q, MjhImageMeta *__restrict__ meta)
{
  const int img = blockIdx.y;
  if (B.status[img] == 0u) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) meta[img].bad_coef = 1u;
  int16_t *q = coef_q + (size_t)img * C.coefs_per_image;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < C.coefs_per_image; i += (long long)gridDim.x * 256) q[i] = 0;
}

__global__ void __launch_bounds__(64)
k_dec_finish(const uint8_t *__restrict__ jfif7, int patch, uint8_t *__restrict__ out, size_t out_stride, const MjhImageMeta *__restrict__ meta,
             unsigned *__restrict__ status, int n)
{
  const int img = blockIdx.x * 64 + threadIdx.x;
  if (img >= n) return;
  if (meta[img].bad_coef && status[img] == 0u) status[img] = MJH_DEC_BADCOEF;
  if (patch)
    for (int i = 0; i < 7; i++) out[(size_t)img * out_stride + 11 + i] = jfif7[img * 8 + i];
}

void mjh_launch_dec_sync(const MjhConst &C, const MjhDecBatch &B, int q, int first, hipStream_t s)
{
  hipLaunchKernelGGL(k_dec_sync, dim3(B.nsub_padded / MJH_DEC_WG), dim3(MJH_DEC_WG), 0, s, C, B, q, first);
}
void mjh_launch_dec_prefix(const MjhDecBatch &B, hipStream_t s)
{
  hipLaunchKernelGGL(k_dec_prefix, dim3(B.nseg), dim3(64), 0, s, B);
}
void mjh_launch_dec_store(const MjhConst &C, const MjhDecBatch &B, int16_t *coef_q, hipStream_t s)
{
  hipLaunchKernelGGL(k_dec_store, dim3(B.nsub_padded / MJH_DEC_WG), dim3(MJH_DEC_WG), 0, s, C, B, coef_q);
}
void mjh_launch_dec_dc(const MjhConst &C, const MjhDecBatch &B, int16_t *coef_q, hipStream_t s)
{
  hipLaunchKernelGGL(k_dec_dc, dim3(C.ncomp, B.nscan), dim3(MJH_DEC_WG), 0, s, C, B, coef_q);
}
void mjh_launch_dec_store_x(const MjhConst &Cs, const MjhDecBatch &B, int16_t *coef_q, const MjhXform *X, hipStream_t s)
{
  hipLaunchKernelGGL(k_dec_store_x, dim3(B.nsub_padded / MJH_DEC_WG), dim3(MJH_DEC_WG), 0, s, Cs, B, coef_q, X);
}
void mjh_launch_dec_dc_x(const MjhConst &Cs, const MjhDecBatch &B, int16_t *coef_q, const MjhXform *X, hipStream_t s)
{
  hipLaunchKernelGGL(k_dec_dc_x, dim3(Cs.ncomp, B.nscan), dim3(MJH_DEC_WG), 0, s, Cs, B, coef_q, X);
}
void mjh_launch_dec_scrub(const MjhConst &C, const MjhDecBatch &B, int16_t *coef_q, void *meta, hipStream_t s)
{
  hipLaunchKernelGGL(k_dec_scrub, dim3(64, B.n), dim3(256), 0, s, C, B, coef_q, (MjhImageMeta *)meta);
}
void mjh_launch_dec_finish(const uint8_t *jfif7, int patch, uint8_t *out, size_t out_stride, const void *meta, unsigned *status, int n, hipStream_t s)
{
  hipLaunchKernelGGL(k_dec_finish, dim3((n + 63) / 64), dim3(64), 0, s, jfif7, patch, out, out_stride, (const MjhImageMeta *)meta, status, n);
}
