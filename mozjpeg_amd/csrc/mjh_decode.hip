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
//
// This file: dec_run (one sequential block: DC symbol, then AC symbols), k_dec_prefix, the scrub and the finish, and the launchers of
// all phases.  The phases themselves (first pass and sync rounds, storing pass, DC sums) are the bodies of mjh_decode_dev.h, which the
// first scans of progressive files share (mjh_decode_prog.hip); k_dec_sync, k_dec_store[_x] and k_dec_dc[_x] instantiate them.
#include <hip/hip_runtime.h>
#include "mjh_device.h"
#include "mjh_decode.h"
#include "mjh_decode_dev.h"

// The run function of a sequential scan (declared in mjh_decode_dev.h).  XF: every store goes through *X.
template <bool STORE, bool XF>
__device__ __forceinline__ bool dec_run(const MjhComp *lc, const MjhDecScan &sc, const MjhDecTable *T, DecReader &R, unsigned end_bits,
                                        unsigned &p, int &k, int &b, unsigned &n, unsigned ord, unsigned total, int mcu,
                                        int16_t *coef_img, int16_t *diff_img, unsigned &flags, int lim, const MjhXform *X)
{
  DecWhere wh{ 0, -1, 0 };
  unsigned cls = 0;
  // XF: wh.blk becomes the block's index in the DESTINATION component
  auto remap = [&]() {
    if (XF && wh.blk >= 0) { const int wib = lc[wh.j].wib, row = wh.blk / wib; wh.blk = dec_xf_block(*X, X->c[sc.comp[wh.j]], row, wh.blk - row * wib, cls); }
  };
  int j = dec_comp_of_block(sc, b);
  if (STORE) { wh = dec_locate(lc, sc, mcu, b); remap(); }
  bool bad = false;
  while (p < end_bits) {
    if (STORE && ord >= total) break;
    const unsigned long long w = R.fetch(p);
    int nb;
    bool done = false;
    if (k == 0) {
      const int s = dec_symbol(T[2 * j], w, nb, bad) & 15;
      if (STORE) diff_img[wh.m] = (int16_t)(s ? dec_extend(w, nb, s) : 0);
      p = R.advance(p, nb + s);
      k = 1;
    } else {
      const int sym = dec_symbol(T[2 * j + 1], w, nb, bad);
      const int r = sym >> 4, s = sym & 15;
      if (s) {
        k += r;
        if (STORE) {
          const int val = dec_extend(w, nb, s);
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
      if (b >= sc.bpm) { b = 0; mcu++; }
      j = dec_comp_of_block(sc, b);
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
k_dec_sync(MjhConst C, MjhDecBatch B, int q, int first) { dec_sync_body<MJH_DEC_SEQ>(C, B, nullptr, q, first); }

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

// the storing pass and the DC sums, plain and with a transform (C = the SOURCE frame's geometry, *X = where things go)
__global__ void __launch_bounds__(MJH_DEC_WG)
k_dec_store(MjhConst C, MjhDecBatch B, int16_t *__restrict__ coef_q) { dec_store_body<MJH_DEC_SEQ, false>(C, B, nullptr, coef_q, nullptr); }
__global__ void __launch_bounds__(MJH_DEC_WG)
k_dec_store_x(MjhConst C, MjhDecBatch B, int16_t *__restrict__ coef_q, const MjhXform *__restrict__ X) { dec_store_body<MJH_DEC_SEQ, true>(C, B, nullptr, coef_q, X); }
__global__ void __launch_bounds__(MJH_DEC_WG)
k_dec_dc(MjhConst C, MjhDecBatch B, int16_t *__restrict__ coef_q) { dec_dc_body<MJH_DEC_SEQ, false>(C, B, nullptr, coef_q, nullptr); }
__global__ void __launch_bounds__(MJH_DEC_WG)
k_dec_dc_x(MjhConst C, MjhDecBatch B, int16_t *__restrict__ coef_q, const MjhXform *__restrict__ X) { dec_dc_body<MJH_DEC_SEQ, true>(C, B, nullptr, coef_q, X); }

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

// PS != nullptr: the first scans of progressive files (the wrappers of mjh_decode_prog.hip); X != nullptr: a transform (sequential only)
void mjh_launch_dec_sync(const MjhConst &C, const MjhDecBatch &B, const MjhDecProg *PS, int q, int first, hipStream_t s)
{
  const dim3 grid(B.nsub_padded / MJH_DEC_WG), wg(MJH_DEC_WG);
  if (PS) hipLaunchKernelGGL(k_pdec_sync, grid, wg, 0, s, C, B, PS, q, first);
  else hipLaunchKernelGGL(k_dec_sync, grid, wg, 0, s, C, B, q, first);
}
void mjh_launch_dec_prefix(const MjhDecBatch &B, hipStream_t s)
{
  hipLaunchKernelGGL(k_dec_prefix, dim3(B.nseg), dim3(64), 0, s, B);
}
void mjh_launch_dec_store(const MjhConst &C, const MjhDecBatch &B, const MjhDecProg *PS, const MjhXform *X, int16_t *coef_q, hipStream_t s)
{
  const dim3 grid(B.nsub_padded / MJH_DEC_WG), wg(MJH_DEC_WG);
  if (PS) hipLaunchKernelGGL(k_pdec_store, grid, wg, 0, s, C, B, PS, coef_q);
  else if (X) hipLaunchKernelGGL(k_dec_store_x, grid, wg, 0, s, C, B, coef_q, X);
  else hipLaunchKernelGGL(k_dec_store, grid, wg, 0, s, C, B, coef_q);
}
void mjh_launch_dec_dc(const MjhConst &C, const MjhDecBatch &B, const MjhDecProg *PS, const MjhXform *X, int16_t *coef_q, hipStream_t s)
{
  const dim3 grid(C.ncomp, B.nscan), wg(MJH_DEC_WG);
  if (PS) hipLaunchKernelGGL(k_pdec_dc, grid, wg, 0, s, C, B, PS, coef_q);
  else if (X) hipLaunchKernelGGL(k_dec_dc_x, grid, wg, 0, s, C, B, coef_q, X);
  else hipLaunchKernelGGL(k_dec_dc, grid, wg, 0, s, C, B, coef_q);
}
void mjh_launch_dec_scrub(const MjhConst &C, const MjhDecBatch &B, int16_t *coef_q, void *meta, hipStream_t s)
{
  hipLaunchKernelGGL(k_dec_scrub, dim3(64, B.n), dim3(256), 0, s, C, B, coef_q, (MjhImageMeta *)meta);
}
void mjh_launch_dec_finish(const uint8_t *jfif7, int patch, uint8_t *out, size_t out_stride, const void *meta, unsigned *status, int n, hipStream_t s)
{
  hipLaunchKernelGGL(k_dec_finish, dim3((n + 63) / 64), dim3(64), 0, s, jfif7, patch, out, out_stride, (const MjhImageMeta *)meta, status, n);
}
