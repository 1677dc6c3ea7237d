// mjh_lossless.hip -- gfx950 kernels of lossless JPEG (SOF3, process 14 with Huffman coding): jclossls.c (prediction + point
// transform), jclhuff.c (statistics, bit writer), jcdiffct.c (row order).
//
// Every difference of an image depends on original samples only (the predictor reads the row above and the sample to the left
// after the point transform, never a reconstructed value), so all of them are independent and only the bit offsets form a scan.
// Work unit: LL_UNIT consecutive pixels of one row of one image (a 4K row is four units), one 256-thread workgroup each.
//   (every kernel that reads pixels stages the unit's row and the row above in LDS first: coalesced loads, no re-reads)
//   k_ll_stats   symbol histogram of the unit (category = bit length of the difference mod 2^16, 0..16), packed 4-bit
//                counters per thread, wave sums of two bins at a time, ONE global atomic per non-zero bin and workgroup; the unit's
//                histogram is kept
//   (k_gen_tables_list of mjh_kernels.hip builds the optimal table from it: jpeg_gen_optimal_table, 17 symbols)
//   k_ll_len     bits of every unit from its histogram and the table (no second pass over the pixels)
//   k_ll_scan    one workgroup per image: exclusive prefix of the unit lengths, restart segments (whole rows, jclossls.c:289-294)
//                padded to bytes + 16 marker bits; final offsets, RSTn byte positions, total
//   k_ll_zero    clears exactly the stream words the writer ORs into
//   k_ll_write   the unit's symbols (kept in registers from the length sum) with their value bits in one accumulator step,
//                assembled in an LDS window, RSTn at segment ends
// The final pad, the header, byte stuffing and the hand-over are the sequential coder's (mjh_launch_finish_bits, mjh_launch_header,
// mjh_launch_stuff, k_pack_results).
//
// A script of several scans (validate_script jcmaster.c:302-311, :390-416; the reference keeps the whole image in a sample buffer,
// jcdiffct.c:235-335, and walks it once per scan): every scan has its own components, predictor, point transform, statistics and
// table, and the MCU of a scan is one sample of each of ITS components (jcdiffct.c:160-215).  The scan is a dimension of the data,
// not of the launches: "virtual image" v = scan * n + image indexes the histograms, bit lengths, offsets, marker positions, totals
// and streams (n = images of the call), so the scans of a batch are the same five launches.  k_ll_stats and k_ll_write stage the
// unit's rows ONCE, before the point transform, and walk the scans over the staged samples (the MS = true instantiations; a
// one-scan image runs the MS = false ones, whose rows are staged after the point transform as before).  Restart segments are whole
// rows of the image in every scan (1x1 sampling, jcmaster.c:1072-1082); the RSTn counter and the first-row predictor start again
// with every scan.
// Reference behaviour is cited as file:line of the reference tree.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mjh_internal.h"
#include "mjh_device.h"
#include "mjh_lossless.h"

#define LL_THREADS 256
#define LL_PER_THREAD 4
#define LL_WIN 4096          // LDS window of the bit writer in words, one scan of a unit at a time; the widest scan holds all three components: 1024 pixels x 3 samples x 31 bits + pad + marker = 95 256 bits < 131 072

// one input sample after the point transform (simple_downscale jclossls.c:262-268)
template <class T>
__device__ __forceinline__ int ll_load(const T *__restrict__ row, int x, int px, int off, int pt)
{
  return (int)row[(size_t)x * px + off] >> pt;
}

// The unit's samples after the point transform, staged in LDS as uint16 (coalesced loads, each input sample read once per row it is
// used in): cur[j * ncomp + c] = component c of pixel x0 - 1 + j of row y, abv[...] the same of row y - 1 (j = 0: the pixel left
// of the unit, when there is one).  n = pixels of the unit.  pt: the one scan's point transform, or 0 when the scans of a script
// apply their own to the staged samples (ll_diff).
#define LL_STAGE ((LL_UNIT + 1) * 3)
template <class T>
__device__ __forceinline__ void ll_stage(const LlConst &L, const uint8_t *__restrict__ pix, size_t row_pitch, size_t img_stride, int img, int y,
                                         int x0, int n, int pt, uint16_t *cur, uint16_t *abv)
{
  const T *row = reinterpret_cast<const T *>(pix + (size_t)img * img_stride + (size_t)y * row_pitch);
  const T *up = reinterpret_cast<const T *>(pix + (size_t)img * img_stride + (size_t)(y > 0 ? y - 1 : 0) * row_pitch);
  const int nc = L.ncomp, cnt = (n + 1) * nc;
  for (int i = threadIdx.x; i < cnt; i += LL_THREADS) {
    const int j = i / nc, c = i - j * nc, x = x0 - 1 + j;
    if (x >= 0) {
      const size_t o = (size_t)x * L.px_size + L.off[c];
      cur[i] = (uint16_t)((int)row[o] >> pt);
      abv[i] = (uint16_t)((int)up[o] >> pt);
    }
  }
  __syncthreads();
}

// jclossls.c:75-134 (DIFFERENCE_1D / DIFFERENCE_2D) + jpeg_difference_first_row :195-233: the first row of the scan and of every
// restart interval predicts its first sample with 2^(P-Pt-1) and the others with Ra; every other row predicts its first sample with
// Rb and the others with predictor PSV (jlossls.h:37-43).  i = (x - x0 + 1) * nc + c: the sample's index in the staged rows (nc =
// staged samples per pixel); pt = what is left to shift (0: staged after the point transform).
__device__ __forceinline__ int ll_diff(int nc, int psv, int pt, int init_pred, const uint16_t *cur, const uint16_t *abv, int x, int i, bool first_row)
{
  const int s = cur[i] >> pt;
  int pred;
  if (first_row) pred = x == 0 ? init_pred : cur[i - nc] >> pt;
  else if (x == 0) pred = abv[i] >> pt;
  else {
    const int Ra = cur[i - nc] >> pt, Rb = abv[i] >> pt, Rc = abv[i - nc] >> pt;
    switch (psv) {
      case 1: pred = Ra; break;
      case 2: pred = Rb; break;
      case 3: pred = Rc; break;
      case 4: pred = Ra + Rb - Rc; break;
      case 5: pred = Ra + ((Rb - Rc) >> 1); break;
      case 6: pred = Rb + ((Ra - Rc) >> 1); break;
      default: pred = (Ra + Rb) >> 1; break;
    }
  }
  return s - pred;
}

// jclhuff.c:353-390: the difference mod 2^16; category = bit length of its magnitude, 16 for a magnitude of 32768 (no value bits);
// a negative difference sends the one's complement of its magnitude
__device__ __forceinline__ int ll_category(int d, unsigned &val)
{
  unsigned t = (unsigned)d & 0xFFFFu;
  if (t & 0x8000u) {
    const unsigned m = (unsigned)(-d) & 0x7FFFu;
    if (m == 0u) { val = 0u; return 16; }
    val = ~m;
    return bitlen(m);
  }
  val = t;
  return bitlen(t);
}

__device__ __forceinline__ bool ll_first_row(const LlConst &L, int y) { return L.rows_per_seg ? y % L.rows_per_seg == 0 : y == 0; }

// ---- statistics (encode_mcus_gather jclhuff.c:520-560) ----------------------------------------------------------------------------
// The unit's histogram goes to hist[virtual image][unit][17] as well: the bits of a unit are then sum(count * (code length +
// category)) once the table exists, without a second pass over the pixels.  MS: every scan of the script over the rows staged once.
template <class T, bool MS>
__global__ void __launch_bounds__(LL_THREADS)
k_ll_stats(LlConst L, const uint8_t *__restrict__ pix, size_t row_pitch, size_t img_stride, MjhHuffTable *__restrict__ tabs, int spi, int slot,
           unsigned *__restrict__ hist)
{
  __shared__ uint16_t s_cur[LL_STAGE], s_abv[LL_STAGE];
  __shared__ unsigned s_bins[LL_THREADS / 64][17];
  const int img = blockIdx.z, y = blockIdx.y, x0 = blockIdx.x * LL_UNIT, tid = threadIdx.x;
  const int n = min(LL_UNIT, L.W - x0);
  ll_stage<T>(L, pix, row_pitch, img_stride, img, y, x0, n, MS ? 0 : L.pt, s_cur, s_abv);
  const bool first = ll_first_row(L, y);
  const int nscan = MS ? L.nscan : 1;
  for (int sc = 0; sc < nscan; sc++) {
    const int snc = MS ? L.sc[sc].ncomp : L.ncomp, psv = MS ? L.sc[sc].psv : L.psv, pt = MS ? L.sc[sc].pt : 0;
    const int ipred = MS ? L.sc[sc].init_pred : L.init_pred, tslot = MS ? L.sc[sc].slot : slot;
    const int co0 = MS ? L.sc[sc].comp[0] : 0, co1 = MS ? L.sc[sc].comp[1] : 0, co2 = MS ? L.sc[sc].comp[2] : 0;     // (MS only)
    // 4-bit counters: at most LL_PER_THREAD * 3 = 12 samples per thread and scan; bins 0..7 in c0, 8..15 in c1, 16 in c2
    unsigned c0 = 0u, c1 = 0u, c2 = 0u;
#pragma unroll
    for (int k = 0; k < LL_PER_THREAD; k++) {
      const int j = tid + LL_THREADS * k;
      if (j < n) {
        for (int c = 0; c < snc; c++) {
          unsigned v;
          const int ci = MS ? (c == 0 ? co0 : c == 1 ? co1 : co2) : c;
          const int nb = ll_category(ll_diff(L.ncomp, psv, pt, ipred, s_cur, s_abv, x0 + j, (j + 1) * L.ncomp + ci, first), v);
          c0 += nb < 8 ? 1u << (4 * nb) : 0u;
          c1 += (nb >> 3) == 1 ? 1u << (4 * (nb & 7)) : 0u;
          c2 += nb == 16 ? 1u : 0u;
        }
      }
    }
    // the wave's totals: two bins per 32-bit word in 16-bit fields (at most 64 x 12 = 768 per bin), nine wave sums instead of 17
    const int lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int k = 0; k < 9; k++) {
      const unsigned src = k < 4 ? c0 : k < 8 ? c1 : c2;
      const int sh = 8 * (k & 3);
      const unsigned v = k < 8 ? ((src >> sh) & 15u) | (((src >> (sh + 4)) & 15u) << 16) : c2;
      const unsigned tot = wave_incl_scan(v);
      if (lane == 63) {
        s_bins[w][2 * k] = tot & 0xFFFFu;
        if (k < 8) s_bins[w][2 * k + 1] = tot >> 16;
      }
    }
    __syncthreads();
    if (tid < 17) {
      unsigned s = 0u;
#pragma unroll
      for (int i = 0; i < LL_THREADS / 64; i++) s += s_bins[i][tid];
      const size_t v = (size_t)sc * gridDim.z + img;
      hist[(v * L.units + (size_t)y * L.units_x + blockIdx.x) * 17 + tid] = s;
      if (s) atomicAdd(&tabs[(size_t)img * spi + tslot].counts[tid], s);
    }
    if (MS) __syncthreads();     // (s_bins serves the next scan)
  }
}

// the table as (size << 16 | code) per category, in LDS
__device__ __forceinline__ void ll_load_table(unsigned *s_tab, const MjhHuffTable *__restrict__ T, int tid)
{
  if (tid < 17) s_tab[tid] = ((unsigned)T->ehufsi[tid] << 16) | T->ehufco[tid];
  __syncthreads();
}

__device__ __forceinline__ unsigned ll_bits(const unsigned *s_tab, int nb) { return (s_tab[nb] >> 16) + (nb == 16 ? 0u : (unsigned)nb); }

// ---- bits per unit: the unit's histogram against the table of its scan (one lane per unit; blockIdx.y = virtual image) ------------
__global__ void __launch_bounds__(LL_THREADS)
k_ll_len(LlConst L, const MjhHuffTable *__restrict__ tabs, int spi, int nimg, const unsigned *__restrict__ hist, unsigned *__restrict__ len)
{
  __shared__ unsigned s_tab[17];
  const int v = blockIdx.y, sc = v / nimg, img = v - sc * nimg, tid = threadIdx.x;
  ll_load_table(s_tab, tabs + (size_t)img * spi + L.sc[sc].slot, tid);
  const int u = blockIdx.x * LL_THREADS + tid;
  if (u >= L.units) return;
  const unsigned *h = hist + ((size_t)v * L.units + u) * 17;
  unsigned bits = 0u;
#pragma unroll
  for (int b = 0; b < 17; b++) bits += h[b] * ll_bits(s_tab, b);
  len[(size_t)v * L.units + u] = bits;
}

// ---- offsets (one workgroup per image, its scans one after the other) -------------------------------------------------------------
// off[u] = final bit offset of unit u; segment s (rows [s R, s R + R)) but the last is padded with 1-bits to a byte boundary and
// followed by RSTn (emit_restart jclhuff.c:237-262): seg_E[s] = bits those add in front of segment s.  mpos[s] = byte position of
// the 0xFF of the marker behind segment s.  totals[v] = bits of the scan before the final pad; 0xFFFFFFFF: a scan of the image does
// not fit the 32-bit offsets / its stream buffer (every scan is checked on its own; one that does not fit marks ALL scans of the
// image, so that none of them is written and the host sees the report at the image's first scan).
__global__ void __launch_bounds__(256)
k_ll_scan(LlConst L, const unsigned *__restrict__ len, unsigned *__restrict__ off, unsigned *__restrict__ seg_E, unsigned *__restrict__ mpos,
          unsigned *__restrict__ totals, unsigned long long stream_bits)
{
  __shared__ unsigned sh[4];
  __shared__ unsigned s_bad;
  const int img = blockIdx.x, nimg = gridDim.x, tid = threadIdx.x;
  bool any_bad = false;
  for (int sc = 0; sc < L.nscan; sc++) {
    const size_t v = (size_t)sc * nimg + img;
    const unsigned *l = len + v * L.units;
    unsigned *o = off + v * L.units;
    unsigned carry = 0u;
    unsigned long long wide = 0ull;
    for (int base = 0; base < L.units; base += 256) {
      const int u = base + tid;
      const unsigned x = u < L.units ? l[u] : 0u;
      unsigned tot;
      const unsigned ex = block_excl_scan_256(x, sh, &tot);
      if (u < L.units) o[u] = carry + ex;
      carry += tot;
      wide += tot;
    }
    __syncthreads();     // (the raw offsets of every unit are read below)
    // segment extras: pad of every segment but the last + 16 marker bits
    const int upseg = L.rows_per_seg * L.units_x;
    unsigned ecarry = 0u;
    if (L.nseg > 1)
      for (int base = 0; base < L.nseg; base += 256) {
        const int s = base + tid;
        unsigned x = 0u;
        if (s < L.nseg - 1) {
          const unsigned a = o[(size_t)s * upseg], b = o[(size_t)(s + 1) * upseg];
          x = ((8u - ((b - a) & 7u)) & 7u) + 16u;
        }
        unsigned tot;
        const unsigned ex = block_excl_scan_256(x, sh, &tot);
        if (s < L.nseg) seg_E[v * L.nseg + s] = ecarry + ex;
        if (s < L.nseg - 1) mpos[v * L.nseg + s] = (o[(size_t)(s + 1) * upseg] + ecarry + ex + x - 16u) >> 3;
        ecarry += tot;
        wide += tot;
      }
    if (tid == 0) s_bad = wide + 64ull > stream_bits || wide >= 0xFFF00000ull;
    __syncthreads();
    // final offsets of the units behind the first segment
    if (L.nseg > 1)
      for (int u = upseg + tid; u < L.units; u += 256) o[u] += seg_E[v * L.nseg + u / upseg];
    any_bad = any_bad || s_bad;
    if (tid == 0) totals[v] = carry + ecarry;
    __syncthreads();     // (s_bad and sh serve the next scan)
  }
  if (any_bad && tid < L.nscan) totals[(size_t)tid * nimg + img] = 0xFFFFFFFFu;
}

// blockIdx.y = virtual image
__global__ void __launch_bounds__(256)
k_ll_zero(unsigned *__restrict__ stream, size_t stream_words_per_image, const unsigned *__restrict__ totals)
{
  const int img = blockIdx.y;
  if (totals[img] == 0xFFFFFFFFu) return;
  const unsigned nw = (totals[img] >> 5) + 2u;   // (+ the word of the final pad)
  unsigned *p = stream + (size_t)img * stream_words_per_image;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < nw; i += gridDim.x * 256) p[i] = 0u;
}

// ---- bit writer (encode_mcus_huff jclhuff.c:329-410: interleaved MCU = one sample of every component of the scan, in component
// order) --------------------------------------------------------------------------------------------------------------------------
// A thread codes LL_PER_THREAD consecutive pixels; their symbols stay in registers between the length sum and the bit writer.
// MS: the scans of the script one after the other over the rows staged once, each into the stream of its virtual image.
template <class T, bool MS>
__global__ void __launch_bounds__(LL_THREADS)
k_ll_write(LlConst L, const uint8_t *__restrict__ pix, size_t row_pitch, size_t img_stride, const MjhHuffTable *__restrict__ tabs, int spi, int slot,
           const unsigned *__restrict__ off, const unsigned *__restrict__ totals, unsigned *__restrict__ stream, size_t stream_words_per_image)
{
  __shared__ unsigned s_tab[17];
  __shared__ unsigned sh[4];
  __shared__ uint16_t s_cur[LL_STAGE], s_abv[LL_STAGE];
  __shared__ unsigned s_win[LL_WIN];
  const int img = blockIdx.z, y = blockIdx.y, tid = threadIdx.x;
  if (totals[img] == 0xFFFFFFFFu) return;     // (k_ll_scan marks every scan of an image that has one out of range)
  const int x0 = blockIdx.x * LL_UNIT, n = min(LL_UNIT, L.W - x0);
  if (!MS) ll_load_table(s_tab, tabs + (size_t)img * spi + slot, tid);
  ll_stage<T>(L, pix, row_pitch, img_stride, img, y, x0, n, MS ? 0 : L.pt, s_cur, s_abv);
  const int u = y * L.units_x + blockIdx.x;
  const bool first = ll_first_row(L, y);
  const int ja = tid * LL_PER_THREAD;
  const int segi = L.rows_per_seg ? y / L.rows_per_seg : 0;
  const bool seg_end = L.nseg > 1 && segi < L.nseg - 1 && (int)blockIdx.x == L.units_x - 1 && (y + 1) % L.rows_per_seg == 0;
  const bool last_unit = u == L.units - 1;
  const int nscan = MS ? L.nscan : 1;
  for (int sc = 0; sc < nscan; sc++) {
    const int snc = MS ? L.sc[sc].ncomp : L.ncomp, psv = MS ? L.sc[sc].psv : L.psv, pt = MS ? L.sc[sc].pt : 0;
    const int ipred = MS ? L.sc[sc].init_pred : L.init_pred;
    const int co0 = MS ? L.sc[sc].comp[0] : 0, co1 = MS ? L.sc[sc].comp[1] : 0, co2 = MS ? L.sc[sc].comp[2] : 0;     // (MS only)
    if (MS) {
      __syncthreads();     // (the previous scan's table and window have been read)
      ll_load_table(s_tab, tabs + (size_t)img * spi + L.sc[sc].slot, tid);
    }
    unsigned e[LL_PER_THREAD * 3], val[LL_PER_THREAD * 3];    // (size << 16 | code), value bits << 8 | category; e = 0: no sample
    unsigned mybits = 0u;
#pragma unroll
    for (int k = 0; k < LL_PER_THREAD; k++)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const int j = ja + k;
        e[3 * k + c] = 0u; val[3 * k + c] = 0u;
        if (j < n && c < snc) {
          unsigned v;
          const int ci = MS ? (c == 0 ? co0 : c == 1 ? co1 : co2) : c;
          const int nb = ll_category(ll_diff(L.ncomp, psv, pt, ipred, s_cur, s_abv, x0 + j, (j + 1) * L.ncomp + ci, first), v);
          const unsigned nv = nb == 16 ? 0u : (unsigned)nb;
          e[3 * k + c] = s_tab[nb] | 0x80000000u;
          val[3 * k + c] = ((v & ((1u << nv) - 1u)) << 8) | nv;
          mybits += (s_tab[nb] >> 16) + nv;
        }
      }
    unsigned utot;
    const unsigned ex = block_excl_scan_256(mybits, sh, &utot);
    // the unit's bit range [start, end): the last unit of a segment but the last one also holds the pad and the marker
    const size_t vi = (size_t)sc * gridDim.z + img;
    const size_t ib = vi * L.units;
    const unsigned start = off[ib + u];
    const unsigned end = last_unit ? totals[vi] : off[ib + u + 1];
    const unsigned w0 = start >> 5, nw = ((end + 31u) >> 5) - w0;
    for (unsigned i = tid; i < nw; i += LL_THREADS) s_win[i] = 0u;
    __syncthreads();
    BitSink<true> bw;
    bw.init(s_win, start + ex - (w0 << 5));
#pragma unroll
    for (int i = 0; i < LL_PER_THREAD * 3; i++)
      if (e[i]) bw.put_sym(e[i] & 0x7FFFFFFFu, val[i] >> 8, (int)(val[i] & 0xFFu));
    if (seg_end && tid == LL_THREADS - 1) {     // (the window holds the whole unit: the last thread writes the tail behind every sample)
      const unsigned bitpos = start + utot;
      BitSink<true> tw;
      tw.init(s_win, bitpos - (w0 << 5));
      const int pad = (int)((8u - (bitpos & 7u)) & 7u);
      if (pad) tw.put((1u << pad) - 1u, pad);
      tw.put(0xFFD0u + (unsigned)(segi & 7), 16);
      tw.flush();
    }
    bw.flush();
    __syncthreads();
    unsigned *g = stream + vi * stream_words_per_image;
    for (unsigned i = tid; i < nw; i += LL_THREADS) {
      const unsigned v = s_win[i];
      if (v == 0u) continue;                           // (k_ll_zero has cleared the range)
      if (i == 0u || i == nw - 1u) atomicOr(&g[w0 + i], v);   // shared with the neighbouring units
      else g[w0 + i] = v;
    }
  }
}

// =============================================================================================
// host-callable launch wrappers
// =============================================================================================
template <class T, bool MS>
static void ll_launch(const LlConst &L, const void *pix, size_t row_pitch, size_t img_stride, MjhHuffTable *tabs, int spi,
                      unsigned *hist, unsigned *len, unsigned *off, unsigned *seg_E, unsigned *mpos, unsigned *totals, unsigned *stream, size_t stream_words,
                      int n, hipStream_t s, int phase)
{
  const dim3 grid(L.units_x, L.H, n);
  const uint8_t *p = (const uint8_t *)pix;
  const int slot = L.sc[0].slot, nv = n * L.nscan;
  if (phase == 0) {
    hipLaunchKernelGGL((k_ll_stats<T, MS>), grid, dim3(LL_THREADS), 0, s, L, p, row_pitch, img_stride, tabs, spi, slot, hist);
  } else if (phase == 1) {
    hipLaunchKernelGGL(k_ll_len, dim3((L.units + LL_THREADS - 1) / LL_THREADS, nv), dim3(LL_THREADS), 0, s, L, (const MjhHuffTable *)tabs, spi, n,
                       (const unsigned *)hist, len);
    hipLaunchKernelGGL(k_ll_scan, dim3(n), dim3(256), 0, s, L, (const unsigned *)len, off, seg_E, mpos, totals, (unsigned long long)stream_words * 32ull);
    hipLaunchKernelGGL(k_ll_zero, dim3(64, nv), dim3(256), 0, s, stream, stream_words, (const unsigned *)totals);
  } else {
    hipLaunchKernelGGL((k_ll_write<T, MS>), grid, dim3(LL_THREADS), 0, s, L, p, row_pitch, img_stride, (const MjhHuffTable *)tabs, spi, slot,
                       (const unsigned *)off, (const unsigned *)totals, stream, stream_words);
  }
}

void mjh_launch_ll(const LlConst &L, const void *pix, size_t row_pitch, size_t img_stride, MjhHuffTable *tabs, int spi,
                   unsigned *hist, unsigned *len, unsigned *off, unsigned *seg_E, unsigned *mpos, unsigned *totals, unsigned *stream, size_t stream_words,
                   int n, hipStream_t s, int phase)
{
#define LL_GO(T, MS) ll_launch<T, MS>(L, pix, row_pitch, img_stride, tabs, spi, hist, len, off, seg_E, mpos, totals, stream, stream_words, n, s, phase)
  if (L.nscan > 1) { if (L.precision == 8) LL_GO(uint8_t, true); else LL_GO(uint16_t, true); }
  else { if (L.precision == 8) LL_GO(uint8_t, false); else LL_GO(uint16_t, false); }
#undef LL_GO
}
