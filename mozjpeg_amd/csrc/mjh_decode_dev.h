// mjh_decode_dev.h -- device code shared by the Huffman decoder's kernel files (mjh_decode.hip: sequential files, mjh_decode_prog.hip:
// progressive files, mjh_decode_lossless.hip: lossless files): the bit reader, one Huffman symbol, where a block of a scan lies, the workgroup's scan into LDS, and the ONE body
// of each phase of the self-synchronising scheme (first pass and sync rounds, storing pass, DC running sums).  The __global__ kernels
// of both files are one-line wrappers around these bodies; what differs between the source kinds is a compile-time parameter:
//   KIND  the run function: MJH_DEC_SEQ dec_run (sequential), MJH_DEC_PROG pdec_run (first scans of a progressive file, MjhDecProg
//         per scan), MJH_DEC_LL ldec_run (a scan of a lossless file: one difference symbol per sample, no coefficient planes)
//   XF    an MjhXform maps the stores into the destination frame
// Only <SEQ, false>, <SEQ, true>, <PROG, false> and <LL, false> are instantiated: a transform of anything but a sequential file is
// refused on the host.
// The bodies are `static`: their __shared__ variables then have internal linkage like a kernel's own, and the compiler drops the ones
// an instantiation never reads (the sync kernels' component geometry: 352 bytes of LDS).
#ifndef MJH_DECODE_DEV_H
#define MJH_DECODE_DEV_H
#include <hip/hip_runtime.h>
#include "mjh_device.h"
#include "mjh_decode.h"

struct DecReader {
  const uint8_t *d;
  unsigned len;
  unsigned long long acc;   // the 6 data bytes from byte p >> 3 on (stuffed zeros removed), in the low 48 bits
  // the next 41+ bits at bit position p, left-aligned in 64 bits; bytes behind the segment's end read as zero
  __device__ __forceinline__ unsigned long long fetch(unsigned p)
  {
    unsigned idx = p >> 3;
    unsigned long long a = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
      const unsigned byte = idx < len ? (unsigned)d[idx] : 0u;
      a = (a << 8) | byte;
      idx += 1u + (byte == 0xFFu ? 1u : 0u);
    }
    acc = a;
    return a << (16 + (p & 7u));
  }
  // p + nbits (nbits <= 33) in the segment's byte numbering: a consumed 0xFF takes its stuffed zero along
  __device__ __forceinline__ unsigned advance(unsigned p, int nbits) const
  {
    const unsigned tot = (p & 7u) + (unsigned)nbits;
    const int nbytes = (int)(tot >> 3);
    unsigned bp = p >> 3;
#pragma unroll
    for (int i = 0; i < 5; i++)
      if (i < nbytes) bp += 1u + ((((unsigned)(acc >> (40 - 8 * i))) & 0xFFu) == 0xFFu ? 1u : 0u);
    return (bp << 3) | (tot & 7u);
  }
};

// one Huffman symbol at the top of w: its length in nb (jpeg_huff_decode jdhuff.c:455-492); a code no table entry exists for
// reads as symbol 0 of 16 bits and sets bad
__device__ __forceinline__ int dec_symbol(const MjhDecTable &T, unsigned long long w, int &nb, bool &bad)
{
  const unsigned e = T.look[(unsigned)(w >> 56)];
  if (e) { nb = (int)(e >> 8); return (int)(e & 0xFFu); }
  int l = 9;
  int code = (int)(w >> (64 - 9));
  while (l <= 16 && code > T.maxcode[l]) { l++; code = (int)(w >> (64 - l)); }
  if (l > 16) { nb = 16; bad = true; return 0; }
  nb = l;
  return (int)T.huffval[(code + T.valoff[l]) & 0xFF];
}

// the s > 0 value bits behind a symbol of nb bits at the top of w, sign-extended (HUFF_EXTEND, jdhuff.c)
__device__ __forceinline__ int dec_extend(unsigned long long w, int nb, int s)
{
  const int r = (int)((w << nb) >> (64 - s));
  return r < (1 << (s - 1)) ? r - (1 << s) + 1 : r;
}

// component-in-scan of block b of an MCU
__device__ __forceinline__ int dec_comp_of_block(const MjhDecScan &sc, int b)
{
  int j = 0;
  while (j < sc.ncomp - 1 && b >= sc.nb[j]) { b -= sc.nb[j]; j++; }
  return j;
}

// where block b of MCU `mcu` of the scan lies: component-in-scan j, the block's index in the component's planes (-1: a dummy
// block) and its index in the scan-order DC-difference array of the component
struct DecWhere { int j; int blk; long long m; };
__device__ __forceinline__ DecWhere dec_locate(const MjhComp *lc, const MjhDecScan &sc, int mcu, int b)
{
  DecWhere w;
  int j = 0, t = b;
  long long doff = sc.diff_off;
  while (j < sc.ncomp - 1 && t >= sc.nb[j]) { t -= sc.nb[j]; doff += (long long)sc.nb[j] * sc.mcus; j++; }
  w.j = j;
  const MjhComp &cc = lc[j];
  if (sc.ncomp == 1) { w.blk = mcu < cc.nblk ? mcu : -1; w.m = doff + mcu; return w; }
  const int my = mcu / sc.mcus_per_row, mx = mcu - my * sc.mcus_per_row;
  const int by = t / cc.h, bx = t - by * cc.h;
  const int row = my * cc.v + by, col = mx * cc.h + bx;
  w.blk = (row < cc.hib && col < cc.wib) ? row * cc.wib + col : -1;
  w.m = doff + (long long)mcu * sc.nb[j] + t;
  return w;
}

// the workgroup's (image, scan) into LDS: its descriptor, the geometry of its components and, with TABLES, its Huffman tables (every
// lane of a workgroup of WG lanes belongs to the same scan)
template <int WG = MJH_DEC_WG, bool TABLES = true>
__device__ __forceinline__ void dec_load_scan(const MjhConst &C, const MjhDecBatch &B, int scan, MjhDecScan *sc, MjhDecTable *T, MjhComp *lc)
{
  const unsigned *src = reinterpret_cast<const unsigned *>(B.scans + scan);
  unsigned *dst = reinterpret_cast<unsigned *>(sc);
  for (unsigned i = threadIdx.x; i < sizeof(MjhDecScan) / 4; i += WG) dst[i] = src[i];
  __syncthreads();
  for (int t = 0; t < sc->ncomp; t++) {            // (t is uniform: the geometry comes through scalar loads)
    const unsigned *cs = reinterpret_cast<const unsigned *>(&C.c[sc->comp[t]]);
    unsigned *cd = reinterpret_cast<unsigned *>(lc + t);
    for (unsigned i = threadIdx.x; i < sizeof(MjhComp) / 4; i += WG) cd[i] = cs[i];
  }
  if (TABLES)
    for (int t = 0; t < 2 * sc->ncomp; t++) {
      const int ti = (t & 1) ? sc->actab[t >> 1] : sc->dctab[t >> 1];
      const unsigned *ts = reinterpret_cast<const unsigned *>(B.tables + ti);
      unsigned *td = reinterpret_cast<unsigned *>(T + t);
      for (unsigned i = threadIdx.x; i < sizeof(MjhDecTable) / 4; i += WG) td[i] = ts[i];
    }
  __syncthreads();
}

// first byte of subsequence i of a segment: i * S, or the byte behind it when that one is the stuffed zero of an 0xFF
__device__ __forceinline__ unsigned dec_sub_start(const uint8_t *d, unsigned len, unsigned i, unsigned S)
{
  unsigned bp = i * S;
  if (i > 0 && bp < len && d[bp - 1] == 0xFFu && d[bp] == 0u) bp++;
  return bp;
}
__device__ __forceinline__ unsigned dec_sub_end_bits(unsigned len, unsigned i, unsigned nsub, unsigned S)
{
  return (i + 1 >= nsub) ? len * 8u : (i + 1u) * S * 8u;
}

// The segment's last block ended at bit `bit` of byte bp: true when the cursor has passed the segment's end ("Premature end of JPEG
// file" / JWRN_HIT_MARKER) or anything but the padding of that byte follows (jdmarker.c next_marker: "extraneous bytes")
__device__ __forceinline__ bool dec_end_bad(const uint8_t *d, unsigned len, unsigned bp, unsigned bit)
{
  unsigned nbp = bp;
  if (bit) { const unsigned byte = nbp < len ? (unsigned)d[nbp] : 0u; nbp += 1u + (byte == 0xFFu ? 1u : 0u); }
  return bp > len || (bp == len && bit) || nbp < len;
}

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

// the descriptor of the transform into LDS: lanes index its tables by their own k
__device__ __forceinline__ void dec_load_xform(const MjhXform *Xg, MjhXform *X)
{
  const unsigned *src = reinterpret_cast<const unsigned *>(Xg);
  unsigned *dst = reinterpret_cast<unsigned *>(X);
  for (unsigned i = threadIdx.x; i < sizeof(MjhXform) / 4; i += MJH_DEC_WG) dst[i] = src[i];
  __syncthreads();
}

// The run functions (mjh_decode.hip, mjh_decode_prog.hip): decode from the state (p, k, b) while the next code word starts in front
// of end_bits; n counts the blocks completed.  STORE: also while ord < total (the segment's blocks), coefficients and DC differences
// written; true when the segment's last block was completed here.  A file defines the one its kernels instantiate.
template <bool STORE, bool XF>
__device__ __forceinline__ bool dec_run(const MjhComp *lc, const MjhDecScan &sc, const MjhDecTable *T, DecReader &R, unsigned end_bits,
                                        unsigned &p, int &k, int &b, unsigned &n, unsigned ord, unsigned total, int mcu,
                                        int16_t *coef_img, int16_t *diff_img, unsigned &flags, int lim, const MjhXform *X);
template <bool STORE>
__device__ __forceinline__ bool pdec_run(const MjhComp *lc, const MjhDecScan &sc, const MjhDecProg ps, const MjhDecTable *T, DecReader &R, unsigned end_bits,
                                         unsigned &p, int &k, int &b, unsigned &n, unsigned ord, unsigned total, int mcu,
                                         int16_t *coef_img, int16_t *diff_img, unsigned &flags, int lim);

// ldec_run (mjh_decode_lossless.hip): b = the component inside the MCU (one sample each), mcu = the sample's index in the plane
template <bool STORE>
__device__ __forceinline__ bool ldec_run(const MjhDecScan &sc, const MjhDecTable *T, DecReader &R, unsigned end_bits, unsigned &p, int &b, unsigned &n,
                                         unsigned ord, unsigned total, int mcu, int16_t *diff_img, unsigned &flags);
#define MJH_DEC_SEQ 0
#define MJH_DEC_PROG 1
#define MJH_DEC_LL 2

// First pass (first != 0: every lane decodes its own subsequence from the guessed state) and one synchronisation round (lanes walk on
// into the next subsequence until the state they arrive with is the one recorded there).  PS: PROG only.
template <int KIND>
static __device__ __forceinline__ void dec_sync_body(const MjhConst &C, const MjhDecBatch &B, const MjhDecProg *__restrict__ PS, int q, int first)
{
  __shared__ MjhDecScan sc;
  __shared__ MjhDecTable T[2 * MJH_MAXC];
  __shared__ MjhComp lc[MJH_MAXC];
  if (!first && q > 0 && B.changed[q - 1] == 0u) return;      // (uniform: the round before this one changed nothing)
  const unsigned g = blockIdx.x * MJH_DEC_WG + threadIdx.x;
  const unsigned sg0 = B.sub_seg[blockIdx.x * MJH_DEC_WG];
  const int scan = B.segs[sg0].scan;
  dec_load_scan(C, B, scan, &sc, T, lc);
  MjhDecProg ps = { 0, 63, 0, 0 };
  if constexpr (KIND == MJH_DEC_PROG) ps = PS[scan];
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
    k = ps.Ss; b = 0;
    j = i;
  } else {
    const MjhDecCarry c = B.carry[g];
    if (!c.active) return;
    p = c.p; k = (int)(c.kb & 0xFFu); b = (int)(c.kb >> 8);
    j = (unsigned)c.next;
  }
  const unsigned end_bits = dec_sub_end_bits(R.len, j, (unsigned)seg.nsub, S), total = (unsigned)seg.nmcu * (unsigned)sc.bpm;
  if constexpr (KIND == MJH_DEC_PROG) (void)pdec_run<false>(lc, sc, ps, T, R, end_bits, p, k, b, n, 0u, total, 0, nullptr, nullptr, flags, 0);
  else if constexpr (KIND == MJH_DEC_LL) (void)ldec_run<false>(sc, T, R, end_bits, p, b, n, 0u, total, 0, nullptr, flags);
  else (void)dec_run<false, false>(lc, sc, T, R, end_bits, p, k, b, n, 0u, total, 0, nullptr, nullptr, flags, 0, nullptr);
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

// The storing pass: every subsequence again from its now known entry state and block index (k_dec_prefix).  XF: C = the SOURCE
// frame's geometry, the stores go where *Xg says (the destination's planes).
template <int KIND, bool XF>
static __device__ __forceinline__ void dec_store_body(const MjhConst &C, const MjhDecBatch &B, const MjhDecProg *__restrict__ PS, int16_t *__restrict__ coef_q,
                                               const MjhXform *__restrict__ Xg)
{
  __shared__ MjhDecScan sc;
  __shared__ MjhDecTable T[2 * MJH_MAXC];
  __shared__ MjhComp lc[MJH_MAXC];
  const MjhXform *X = nullptr;
  if constexpr (XF) { __shared__ MjhXform s_X; dec_load_xform(Xg, &s_X); X = &s_X; }
  const unsigned g = blockIdx.x * MJH_DEC_WG + threadIdx.x;
  const unsigned sg0 = B.sub_seg[blockIdx.x * MJH_DEC_WG];
  const int scan = B.segs[sg0].scan;
  dec_load_scan(C, B, scan, &sc, T, lc);
  MjhDecProg ps = { 0, 63, 0, 0 };
  if constexpr (KIND == MJH_DEC_PROG) ps = PS[scan];
  const unsigned sg = B.sub_seg[g];
  if (sg == 0xFFFFFFFFu) return;
  const MjhDecSeg seg = B.segs[sg];
  const unsigned i = g - (unsigned)seg.sub0, S = (unsigned)B.S;
  DecReader R;
  R.d = B.bytes + seg.off;
  R.len = seg.len;
  unsigned p = 0, n = 0, flags = 0;
  int k = ps.Ss, b = 0;
  if (i > 0) { const MjhDecState e = B.state[g - 1]; p = e.p; k = (int)(e.kb & 0xFFu); b = (int)(e.kb >> 8); }
  const unsigned ord = B.ord[g], total = (unsigned)seg.nmcu * (unsigned)sc.bpm;
  const bool last = i + 1 == (unsigned)seg.nsub;
  if (ord < total) {
    // (the entry state's b is ord mod bpm whenever the chain of states is the true one; a damaged stream may leave anything: the
    //  block index decides where stores go, the state only how the bits are read)
    b = (int)(ord % (unsigned)sc.bpm);
    const int mcu = seg.mcu0 + (int)(ord / (unsigned)sc.bpm);
    const unsigned end_bits = dec_sub_end_bits(R.len, i, (unsigned)seg.nsub, S);
    long long cpi = C.coefs_per_image;
    if constexpr (XF) cpi = X->coefs_per_image;
    int16_t *coef_img = coef_q + (size_t)sc.image * cpi, *diff_img = B.diff + (size_t)sc.image * C.total_mcu_blocks;
    bool fin;
    if constexpr (KIND == MJH_DEC_PROG) fin = pdec_run<true>(lc, sc, ps, T, R, end_bits, p, k, b, n, ord, total, mcu, coef_img, diff_img, flags, B.coef_limit);
    else if constexpr (KIND == MJH_DEC_LL) fin = ldec_run<true>(sc, T, R, end_bits, p, b, n, ord, total, mcu, diff_img, flags);
    else fin = dec_run<true, XF>(lc, sc, T, R, end_bits, p, k, b, n, ord, total, mcu, coef_img, diff_img, flags, B.coef_limit, X);
    if (fin) { if (dec_end_bad(R.d, R.len, p >> 3, p & 7u)) flags |= MJH_DEC_CORRUPT; }
    else if (last) flags |= MJH_DEC_CORRUPT;                 // the data ends in front of the segment's last block
  } else if (i == 0) flags |= MJH_DEC_CORRUPT;
  if (flags) atomicOr(&B.status[sc.image], flags);
}

// DC values = per component and restart segment the running sum of the stored differences (dummy blocks take part, jdhuff.c:588-592),
// into plane 0.  PROG: only the DC first scans of the batch, the sums shifted left by the scan's Al.  XF: C = the SOURCE frame's
// geometry (the prediction chain is the source's, dummy blocks included); only the final store is mapped.
template <int KIND, bool XF>
static __device__ __forceinline__ void dec_dc_body(const MjhConst &C, const MjhDecBatch &B, const MjhDecProg *__restrict__ PS, int16_t *__restrict__ coef_q,
                                            const MjhXform *__restrict__ X)
{
  __shared__ int s_sum[MJH_DEC_WG];
  __shared__ int s_rst[MJH_DEC_WG];
  const MjhDecScan *scp = B.scans + blockIdx.y;        // (uniform: read through scalar loads, no private copy)
  const int j = blockIdx.x, ncomp = scp->ncomp;
  if (j >= ncomp) return;
  int Al = 0;
  if constexpr (KIND == MJH_DEC_PROG) {
    if (PS[blockIdx.y].Ss != 0) return;                // (uniform: an AC scan has no DC)
    Al = PS[blockIdx.y].Al;
  }
  const MjhComp cc = C.c[scp->comp[j]];
  MjhXformComp xc;
  long long cpi = C.coefs_per_image, coef_off = cc.coef_off;
  if constexpr (XF) {
    xc = X->c[scp->comp[j]];
    if (xc.nblk == 0) return;                          // (uniform: a dropped component)
    cpi = X->coefs_per_image; coef_off = xc.coef_off;
  }
  const int mcus = scp->mcus, mpr = scp->mcus_per_row, image = scp->image;
  long long doff = scp->diff_off;
  for (int t = 0; t < j; t++) doff += (long long)scp->nb[t] * mcus;
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
  int16_t *dc = coef_q + (size_t)image * cpi + coef_off;
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
    if (blk >= cc.nblk) blk = -1;
    if constexpr (XF) {
      if (blk >= 0) { unsigned cls; const int row = blk / cc.wib; blk = dec_xf_block(*X, xc, row, blk - row * cc.wib, cls); }
    }
    if (blk >= 0) dc[blk] = (int16_t)((unsigned)pred << Al);
    if (++ph == L) ph = 0;
    if (++t == nbj) { t = 0; if (++mx == mpr) { mx = 0; my++; } }
  }
}

// the wrappers of mjh_decode_prog.hip that the launchers of mjh_decode.hip choose
__global__ void k_pdec_sync(MjhConst C, MjhDecBatch B, const MjhDecProg *__restrict__ PS, int q, int first);
__global__ void k_pdec_store(MjhConst C, MjhDecBatch B, const MjhDecProg *__restrict__ PS, int16_t *__restrict__ coef_q);
__global__ void k_pdec_dc(MjhConst C, MjhDecBatch B, const MjhDecProg *__restrict__ PS, int16_t *__restrict__ coef_q);
// ... and those of mjh_decode_lossless.hip (a batch of lossless scans has no DC sums: the differences are the output)
__global__ void k_ldec_sync(MjhConst C, MjhDecBatch B, int q, int first);
__global__ void k_ldec_store(MjhConst C, MjhDecBatch B);
#endif
