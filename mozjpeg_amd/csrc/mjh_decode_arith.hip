// mjh_decode_arith.hip -- K-DA: arithmetic-coded source files (SOF9, SOF10; jdarith.c) decoded on the device into the
// coefficient planes mjh_decode.hip fills for a Huffman-coded file (coefficient-major, zig-zag order, zeroed by the caller).
//
// The QM decoder adapts with every decision, so a restart segment is ONE dependent chain; what is parallel are the chains:
// (image, scan, restart segment).  One wave (a workgroup of 64) per chain, all chains of a launch side by side.  The wave is
// a scalar machine (mjh_arith_decoder.h): decoder registers in SGPRs, statistics bins in vector registers, one bin per lane.
// Its lanes do three things together:
//   input   the segment's bytes are fetched 64 at a time, one per lane; a ballot and a prefix count drop the zero behind
//           0xFF and 0xFF fill bytes and pack what stays into lanes 0.., from where the decoder takes its next byte with a
//           lane read.  From the segment's end onward the bytes are zeros (arith_decode :126-145).
//   decode  block after block into AdModel::coef, lane k = zig-zag position k.
//   store   64 consecutive blocks of the chain share an LDS tile; a refinement scan first loads the tile with what the
//           earlier scans left; behind the last block the tile goes out plane by plane, lane b = block b of the tile, so a
//           non-interleaved scan (the component's real blocks in raster order, per_scan_setup) stores 64 consecutive
//           elements of a plane at a time.  Dummy blocks of partial interleaved MCUs are decoded and not stored.
// The DC prediction is the running value per component inside the chain (reset at every restart), so no DC-sum phase follows.
// SOF9: all scans of all images in one launch.  SOF10: one launch per scan ordinal (scan i of every file that has one), in
// stream order, so a refinement finds what the earlier scans of its file stored.
// Bounds: every byte read lies inside [seg.off, seg.off + seg.len); every store is a real block (< nblk) of the scan's
// component at a position in Ss..Se <= 63; the block loop runs over the chain's unit count, whatever the bytes say.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mjh_internal.h"
#include "mjh_device.h"
#include "mjh_decode.h"
#include "mjh_arith_decoder.h"

#define ADEC_U(x) __builtin_amdgcn_readfirstlane((int)(x))
#define ADEC_TILE_STRIDE 66      // shorts between two blocks of the tile: 33 words, so the plane-wise flush (lane = block) meets no bank twice
__device__ __forceinline__ int adec_pick4(const int (&a)[4], int i) { return i == 0 ? a[0] : i == 1 ? a[1] : i == 2 ? a[2] : a[3]; }

// The segment's bytes, de-stuffed 64 at a time.  Wave-uniform but for buf (lane i = byte i of the chunk) and lane.
struct AdecSrc {
  const uint8_t *p;          // the segment
  unsigned len, rpos;        // its length; where the next chunk of raw bytes begins
  int buf, n, i;             // the chunk in hand: n bytes, the next one to hand out
  bool eof;                  // the chunk in hand reaches the segment's end (or a marker): zeros follow
  uint8_t *s_in;             // 64 bytes of LDS
  int lane;
  __device__ __forceinline__ void refill()
  {
    const unsigned pos = rpos + (unsigned)lane;
    const int b = pos < len ? (int)p[pos] : -1;
    const int nx = pos + 1u < len ? (int)p[pos + 1u] : -1;
    const int pv = pos >= 1u && pos - 1u < len ? (int)p[pos - 1u] : 0;
    // the data ends in front of the first byte beyond the segment and in front of an 0xFF that neither a zero nor a fill byte follows
    const unsigned long long stop = __builtin_amdgcn_ballot_w64(b < 0 || (b == 0xFF && nx != 0 && nx != 0xFF));
    const int first = stop ? __builtin_ctzll(stop) : 64;
    const bool keep = lane < first && !(b == 0xFF && nx == 0xFF) && !(b == 0 && pv == 0xFF);
    const unsigned long long km = __builtin_amdgcn_ballot_w64(keep);
    __syncthreads();                                   // (every lane has read the chunk before this one from s_in)
    if (keep) s_in[__builtin_popcountll(km & ((1ull << lane) - 1ull))] = (uint8_t)b;
    __syncthreads();
    buf = s_in[lane];
    n = __builtin_popcountll(km);
    i = 0;
    rpos += 64u;
    eof = first < 64;
  }
  __device__ __forceinline__ int next()
  {
    while (i >= n) {
      if (eof) return 0;
      refill();
    }
    const int v = rl(buf, i);
    i++;
    return v & 0xFF;
  }
};

// The scan of the chain, in registers and wave-uniform for the compiler; arrays are only ever indexed statically (adec_pick4)
struct AdecScan {
  int image, ncomp, bpm;
  int comp[4], td[4], ta[4], nb[4];
  int h[4], wib[4], hib[4], ks[4];
  long long coff[4];
  int Ss, Se, Ah, Al;
  int L[4], U[4], K[4];
};

__device__ __forceinline__ void adec_bind(AdModel &M, int ta, int td, const AdecScan &sc)
{
#pragma unroll
  for (int r = 0; r < 4; r++) M.cur[r] = ta == 0 ? M.ac[0][r] : ta == 1 ? M.ac[1][r] : ta == 2 ? M.ac[2][r] : M.ac[3][r];
  M.dcur = td == 0 ? M.dc[0] : td == 1 ? M.dc[1] : td == 2 ? M.dc[2] : M.dc[3];
  M.dc_lo = (int)((1L << adec_pick4(sc.L, td)) >> 1); M.dc_hi = (int)((1L << adec_pick4(sc.U, td)) >> 1); M.ac_k = adec_pick4(sc.K, ta);
}
__device__ __forceinline__ void adec_unbind(AdModel &M, int ta, int td)
{
#pragma unroll
  for (int t = 0; t < 4; t++) {
#pragma unroll
    for (int r = 0; r < 4; r++) M.ac[t][r] = ta == t ? M.cur[r] : M.ac[t][r];
    M.dc[t] = td == t ? M.dcur : M.dc[t];
  }
}

// whole: the scans of sequential files (PS is not looked at); else PS[i] belongs to B.scans[i].  AR[i]: the conditioning in force
// at scan i's SOS.  grid = B.nseg chains.
__global__ void __launch_bounds__(64)
k_adec_scans(MjhConst C, MjhDecBatch B, const MjhDecProg *__restrict__ PS, const MjhDecArith *__restrict__ AR, int whole, int16_t *__restrict__ coef_q)
{
  __shared__ short s_tile[64 * ADEC_TILE_STRIDE];
  __shared__ uint8_t s_in[64];
  const int lane = threadIdx.x;
  const MjhDecSeg *sg = B.segs + blockIdx.x;
  const int sidx = ADEC_U(sg->scan);
  const MjhDecScan *sp = B.scans + sidx;
  AdecScan sc;
  sc.image = ADEC_U(sp->image); sc.ncomp = ADEC_U(sp->ncomp); sc.bpm = ADEC_U(sp->bpm);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    sc.comp[i] = ADEC_U(sp->comp[i]) & 3; sc.td[i] = ADEC_U(sp->dctab[i]) & 3; sc.ta[i] = ADEC_U(sp->actab[i]) & 3; sc.nb[i] = ADEC_U(sp->nb[i]);
    const MjhComp &cc = C.c[sc.comp[i]];
    sc.h[i] = ADEC_U(cc.h); sc.wib[i] = ADEC_U(cc.wib); sc.hib[i] = ADEC_U(cc.hib); sc.ks[i] = ADEC_U(cc.kstride);
    sc.coff[i] = cc.coef_off;
    sc.L[i] = ADEC_U(AR[sidx].dc_L[i]) & 15; sc.U[i] = ADEC_U(AR[sidx].dc_U[i]) & 15; sc.K[i] = ADEC_U(AR[sidx].ac_K[i]);
  }
  if (whole) { sc.Ss = 0; sc.Se = 63; sc.Ah = 0; sc.Al = 0; }
  else { sc.Ss = ADEC_U(PS[sidx].Ss) & 63; sc.Se = ADEC_U(PS[sidx].Se) & 63; sc.Ah = ADEC_U(PS[sidx].Ah) & 15; sc.Al = ADEC_U(PS[sidx].Al) & 15; }
  const int mcus_per_row = ADEC_U(sp->mcus_per_row);
  const long long u0 = (long long)ADEC_U(sg->mcu0) * sc.bpm, u1 = u0 + (long long)ADEC_U(sg->nmcu) * sc.bpm;
  int16_t *const qimg = coef_q + (size_t)sc.image * C.coefs_per_image;
  const bool refine = !whole && sc.Ah != 0;

  AdModel M;
#pragma unroll
  for (int t = 0; t < 4; t++) {
#pragma unroll
    for (int r = 0; r < 4; r++) M.ac[t][r] = ARI_BIN_RESET;
    M.dc[t] = ARI_BIN_RESET;
  }
#pragma unroll
  for (int r = 0; r < 4; r++) M.cur[r] = ARI_BIN_RESET;
  M.dcur = ARI_BIN_RESET;
  M.coef = 0;
  M.dc_lo = 0; M.dc_hi = 1; M.ac_k = 5;
  M.tab[0] = (int)(((unsigned)mjh_ari_qe[lane] << 16) | ((unsigned)mjh_ari_nmps[lane] << 8) | (unsigned)mjh_ari_nlps[lane]);
  const int j2 = lane + 64 < 114 ? lane + 64 : 113;
  M.tab[1] = (int)(((unsigned)mjh_ari_qe[j2] << 16) | ((unsigned)mjh_ari_nmps[j2] << 8) | (unsigned)mjh_ari_nlps[j2]);

  AriDecoder<AdecSrc> A;
  A.src.p = B.bytes + sg->off;
  A.src.len = (unsigned)ADEC_U(sg->len); A.src.rpos = 0u;
  A.src.buf = 0; A.src.n = 0; A.src.i = 0; A.src.eof = false;
  A.src.s_in = s_in; A.src.lane = lane;
  A.start();
  int last_dc[4] = { 0, 0, 0, 0 }, ctx[4] = { 0, 0, 0, 0 };
  int big = 0;

  for (long long base = u0; base < u1 && !A.bad; base += 64) {
    // ---- lane b: where block b of this tile goes
    const long long u = base + lane;
    const bool have = u < u1;
    int ci = 0, ks = sc.ks[0];
    long long dst = 0;           // element offset of the block inside its component's plane 0, from qimg
    bool real = have;
    if (sc.ncomp == 1) dst = sc.coff[0] + (have ? u : 0);
    else {
      const long long uu = have ? u : u0;
      const int m = (int)(uu / sc.bpm);
      int j = (int)(uu - (long long)m * sc.bpm);
#pragma unroll
      for (int i = 0; i < 3; i++)
        if (ci == i && i + 1 < sc.ncomp && j >= adec_pick4(sc.nb, i)) { j -= adec_pick4(sc.nb, i); ci = i + 1; }
      const int h = adec_pick4(sc.h, ci), wib = adec_pick4(sc.wib, ci), hib = adec_pick4(sc.hib, ci);
      const int v = adec_pick4(sc.nb, ci) / h;
      const int yi = j / h, xi = j - yi * h;
      const int my = m / mcus_per_row, mx = m - my * mcus_per_row;
      const int row = my * v + yi, col = mx * h + xi;
      real = have && row < hib && col < wib;
      ks = adec_pick4(sc.ks, ci);
      dst = (ci == 0 ? sc.coff[0] : ci == 1 ? sc.coff[1] : ci == 2 ? sc.coff[2] : sc.coff[3]) + (real ? (long long)row * wib + col : 0);
    }
    __syncthreads();
    for (int t = lane; t < 64 * ADEC_TILE_STRIDE; t += 64) s_tile[t] = 0;
    __syncthreads();
    if (refine && real)
      for (int k = sc.Ss; k <= sc.Se; k++) s_tile[lane * ADEC_TILE_STRIDE + k] = qimg[dst + (long long)k * ks];
    __syncthreads();
    // ---- the chain
    const int nb = (int)(u1 - base < 64 ? u1 - base : 64);
    for (int b = 0; b < nb; b++) {
      M.coef = s_tile[b * ADEC_TILE_STRIDE + lane];
      const int c = rl(ci, b);
      const int td = adec_pick4(sc.td, c), ta = adec_pick4(sc.ta, c);
      int last = adec_pick4(last_dc, c), cx = adec_pick4(ctx, c);
      int kex = 0;
      if (refine && sc.Ss) {      // the block's last non-zero position in 1..Se (jdarith.c:462)
        const unsigned long long nz = __builtin_amdgcn_ballot_w64(M.coef != 0 && lane >= 1 && lane <= sc.Se);
        kex = nz ? 63 - __builtin_clzll(nz) : 0;
      }
      adec_bind(M, ta, td, sc);
      ad_block(A, M, whole != 0, sc.Ss, sc.Se, sc.Ah, sc.Al, kex, last, cx, &big);
      adec_unbind(M, ta, td);
      if (c == 0) { last_dc[0] = last; ctx[0] = cx; } else if (c == 1) { last_dc[1] = last; ctx[1] = cx; }
      else if (c == 2) { last_dc[2] = last; ctx[2] = cx; } else { last_dc[3] = last; ctx[3] = cx; }
      s_tile[b * ADEC_TILE_STRIDE + lane] = (short)M.coef;
      if (A.bad) break;
    }
    __syncthreads();
    // ---- the tile goes out plane by plane: lane b = block b
    if (!A.bad && real)
      for (int k = sc.Ss; k <= sc.Se; k++) qimg[dst + (long long)k * ks] = s_tile[lane * ADEC_TILE_STRIDE + k];
  }
  if (lane == 0) {
    unsigned st = 0;
    if (A.bad) st |= MJH_DEC_CORRUPT;
    if (big > B.coef_limit) st |= MJH_DEC_BADCOEF;
    if (st) atomicOr(&B.status[sc.image], st);
  }
}

void mjh_launch_adec_scans(const MjhConst &C, const MjhDecBatch &B, const MjhDecProg *PS, const MjhDecArith *AR, int whole_blocks, int16_t *coef_q, hipStream_t s)
{
  if (B.nseg < 1) return;
  hipLaunchKernelGGL(k_adec_scans, dim3(B.nseg), dim3(64), 0, s, C, B, PS, AR, whole_blocks, coef_q);
}
