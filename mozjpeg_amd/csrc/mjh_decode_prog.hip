// mjh_decode_prog.hip -- K-D, progressive: the four scan kinds of a Huffman-coded progressive file (SOF2, jdphuff.c) decoded on the
// device into the same coefficient planes mjh_decode.hip fills for a sequential file (coefficient-major, zig-zag order, zeroed by the
// caller; every kernel here stores or changes only what its scan codes).
//
// First scans (Ah = 0) do not depend on one another and go through the scheme of mjh_decode.hip: restart segments x self-synchronising
// subsequences, k_pdec_sync until the host reads "unchanged", k_dec_prefix, k_pdec_store, k_pdec_dc.  The three are the phase bodies
// of mjh_decode_dev.h instantiated with pdec_run, the run function of this file; the launchers of mjh_decode.hip start them.
//   DC first (decode_mcu_DC_first): one symbol + its value bits per block, dummy blocks included; state = (bit position, block in MCU).
//   AC first (decode_mcu_AC_first): one component, its own raster of real blocks; state = (bit position, k in Ss..Se).  An EOBn symbol
//     ends the current block and R - 1 further ones without another bit, so it adds R to the lane's block count and leaves k = Ss:
//     the run is not part of the state.
// Refinement scans (Ah > 0) change what earlier scans left and run level by level (the host orders them, mjh_encoder.cpp):
//   DC refinement (decode_mcu_DC_refine): one raw bit per block, so block i of a segment is data bit i: a workgroup per segment counts
//     the data bytes (stuffed zeros skipped) in front of every lane's share and ORs 1 << Al into plane 0.
//   AC refinement (decode_mcu_AC_refine): the bits between two code words depend on which coefficients of the block are nonzero
//     already, so nothing synchronises by itself: one wave per restart segment, one lane per coefficient position.  A ballot gives the
//     mask of the nonzero positions of the band; the symbol loop is wave-uniform work on that mask (skipping r zero positions = the
//     r-th clear bit, the correction bits of a step = a popcount); a lane with a nonzero coefficient takes its correction bit by its
//     rank in the mask, and lanes store back only what changed.
// Every byte read is bounded by the segment's length, every store by the component's block count and position 63, every loop by the
// segment's block total, whatever the bytes say.
#include <hip/hip_runtime.h>
#include "mjh_device.h"
#include "mjh_decode.h"
#include "mjh_decode_dev.h"

// Decodes a first scan from (p, k, b) while the next code word starts in front of end_bits; the counterpart of dec_run.  n counts the
// blocks completed here (saturating at total + 1: a damaged run may claim any number).  STORE: also while ord < total; returns true
// when the segment's last block was completed here.  mcu: the MCU (AC: the block of the component's raster) that block `ord` is in.
template <bool STORE>
__device__ __forceinline__ bool pdec_run(const MjhComp *lc, const MjhDecScan &sc, const MjhDecProg ps, const MjhDecTable *T, DecReader &R, unsigned end_bits,
                                         unsigned &p, int &k, int &b, unsigned &n, unsigned ord, unsigned total, int mcu,
                                         int16_t *coef_img, int16_t *diff_img, unsigned &flags, int lim)
{
  bool bad = false;
  if (ps.Ss == 0) {
    // ---- DC first: (*block)[0] = (last_dc_val += diff) << Al; the differences go to the scan-order array, k_pdec_dc sums and shifts
    int j = dec_comp_of_block(sc, b);
    while (p < end_bits) {
      if (STORE && ord >= total) break;
      const unsigned long long w = R.fetch(p);
      int nb;
      const int s = dec_symbol(T[2 * j], w, nb, bad) & 15;
      if (STORE) diff_img[dec_locate(lc, sc, mcu, b).m] = (int16_t)(s ? dec_extend(w, nb, s) : 0);
      p = R.advance(p, nb + s);
      if (n <= total) n++;
      b++;
      if (b >= sc.bpm) { b = 0; mcu++; }
      j = dec_comp_of_block(sc, b);
      if (STORE) {
        ord++;
        if (ord >= total) { if (bad) flags |= MJH_DEC_CORRUPT; return true; }
      }
    }
    if (STORE && bad) flags |= MJH_DEC_CORRUPT;
    return false;
  }
  // ---- AC first: one component, one block per MCU (jdphuff.c:403-428)
  const MjhComp &cc = lc[0];
  while (p < end_bits) {
    if (STORE && ord >= total) break;
    const unsigned long long w = R.fetch(p);
    int nb;
    const int sym = dec_symbol(T[1], w, nb, bad);
    const int r = sym >> 4, s = sym & 15;
    unsigned adv = 0;                     // blocks this code word completes
    if (s) {
      k += r;
      if (STORE) {
        const int val = (int)(int16_t)((unsigned)dec_extend(w, nb, s) << ps.Al);           // (JCOEF)LEFT_SHIFT(s, Al)
        if (val > lim || val < -lim) flags |= MJH_DEC_BADCOEF;
        // a run that passes Se lands where the reference puts it: position k, or 63 through the spare entries of jpeg_natural_order
        if (mcu >= 0 && mcu < cc.nblk) coef_img[cc.coef_off + (long long)(k > 63 ? 63 : k) * cc.kstride + mcu] = (int16_t)val;
      }
      p = R.advance(p, nb + s);
      k++;
      if (k > ps.Se) adv = 1u;
    } else if (r == 15) {
      p = R.advance(p, nb);
      k += 16;
      if (k > ps.Se) adv = 1u;
    } else {                              // EOBr: this block and 2^r + appended bits - 1 further ones
      adv = 1u << r;
      if (r) adv += (unsigned)((w << nb) >> (64 - r));
      p = R.advance(p, nb + r);
    }
    if (adv) {
      k = ps.Ss;
      n = n + adv > total + 1u ? total + 1u : n + adv;
      if (STORE) {
        ord += adv;
        mcu += (int)adv;
        if (ord >= total) {
          if (bad || ord > total) flags |= MJH_DEC_CORRUPT;      // (a run that passes the segment's last block)
          return true;
        }
      }
    }
  }
  if (STORE && bad) flags |= MJH_DEC_CORRUPT;
  return false;
}

// the phases of mjh_decode.hip for first scans: the shared bodies with pdec_run (launched by mjh_launch_dec_sync / _store / _dc)
__global__ void __launch_bounds__(MJH_DEC_WG)
k_pdec_sync(MjhConst C, MjhDecBatch B, const MjhDecProg *__restrict__ PS, int q, int first) { dec_sync_body<MJH_DEC_PROG>(C, B, PS, q, first); }
__global__ void __launch_bounds__(MJH_DEC_WG)
k_pdec_store(MjhConst C, MjhDecBatch B, const MjhDecProg *__restrict__ PS, int16_t *__restrict__ coef_q) { dec_store_body<MJH_DEC_PROG, false>(C, B, PS, coef_q, nullptr); }
__global__ void __launch_bounds__(MJH_DEC_WG)
k_pdec_dc(MjhConst C, MjhDecBatch B, const MjhDecProg *__restrict__ PS, int16_t *__restrict__ coef_q) { dec_dc_body<MJH_DEC_PROG, false>(C, B, PS, coef_q, nullptr); }

// DC refinement: one workgroup per restart segment.  Bit i of the segment's data (stuffed zeros skipped) belongs to block i of the
// segment in MCU order, dummy blocks included; a set bit ORs 1 << Al into the block's DC value.
__global__ void __launch_bounds__(MJH_DEC_WG)
k_pdec_dc_refine(MjhConst C, MjhDecBatch B, const MjhDecProg *__restrict__ PS, int16_t *__restrict__ coef_q)
{
  __shared__ MjhDecScan sc;
  __shared__ MjhComp lc[MJH_MAXC];
  __shared__ unsigned s_cnt[MJH_DEC_WG];
  const MjhDecSeg seg = B.segs[blockIdx.x];
  dec_load_scan<MJH_DEC_WG, false>(C, B, seg.scan, &sc, nullptr, lc);
  const int p1 = 1 << PS[seg.scan].Al;
  const uint8_t *d = B.bytes + seg.off;
  const unsigned len = seg.len, total = (unsigned)seg.nmcu * (unsigned)sc.bpm;
  const unsigned per = (len + MJH_DEC_WG - 1) / MJH_DEC_WG;
  const unsigned i0 = per * threadIdx.x < len ? per * threadIdx.x : len, i1 = i0 + per < len ? i0 + per : len;
  // a zero byte behind an 0xFF is stuffing (a marker cannot be inside a segment, and 0xFF 0x00 0x00 is stuffing + a data byte)
  unsigned cnt = 0;
  for (unsigned i = i0; i < i1; i++) cnt += (d[i] == 0u && i > 0u && d[i - 1] == 0xFFu) ? 0u : 1u;
  s_cnt[threadIdx.x] = cnt;
  __syncthreads();
  unsigned base = 0;
  for (unsigned t = 0; t < threadIdx.x; t++) base += s_cnt[t];
  int16_t *coef_img = coef_q + (size_t)sc.image * C.coefs_per_image;
  unsigned o = base * 8u;                   // the block of my first data bit
  for (unsigned i = i0; i < i1 && o < total; i++) {
    const unsigned byte = d[i];
    if (byte == 0u && i > 0u && d[i - 1] == 0xFFu) continue;
    for (unsigned bit = 0; bit < 8u && o + bit < total; bit++) {
      if (!((byte >> (7u - bit)) & 1u)) continue;
      const unsigned ord = o + bit;
      const DecWhere wh = dec_locate(lc, sc, seg.mcu0 + (int)(ord / (unsigned)sc.bpm), (int)(ord % (unsigned)sc.bpm));
      if (wh.blk >= 0 && wh.blk < lc[wh.j].nblk) coef_img[lc[wh.j].coef_off + wh.blk] |= (int16_t)p1;
    }
    o += 8u;
  }
  if (threadIdx.x == MJH_DEC_WG - 1) {
    // fewer bits than blocks: the data ends early; more bytes than the blocks need: extraneous bytes (as k_dec_store judges a segment)
    const unsigned bytes = base + cnt;
    if (bytes * 8ull < total || bytes > (total + 7u) / 8u) atomicOr(&B.status[sc.image], MJH_DEC_CORRUPT);
  }
}

// The bit cursor of the AC refinement: byte bp (never a stuffed zero) and bit 0..7 inside it.  win(): the next 64 data bits,
// left-aligned; bytes behind the segment's end read as zero.  skip(n): n <= 64 bits on, a consumed 0xFF takes its stuffed zero along.
struct RefCursor {
  const uint8_t *d;
  unsigned len, bp, bit;
  __device__ __forceinline__ unsigned long long win() const
  {
    unsigned idx = bp;
    unsigned long long a = 0;
    unsigned last = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
      const unsigned byte = idx < len ? (unsigned)d[idx] : 0u;
      if (i < 8) a = (a << 8) | byte; else last = byte;
      idx += 1u + (byte == 0xFFu ? 1u : 0u);
    }
    return bit ? (a << bit) | (unsigned long long)(last >> (8u - bit)) : a;
  }
  __device__ __forceinline__ void skip(unsigned nbits)
  {
    const unsigned tot = bit + nbits;
    const unsigned nbytes = tot >> 3;
    for (unsigned i = 0; i < nbytes && i < 9u; i++) {
      const unsigned byte = bp < len ? (unsigned)d[bp] : 0u;
      bp += 1u + (byte == 0xFFu ? 1u : 0u);
    }
    bit = tot & 7u;
  }
};

// bits lo..hi of a 64-bit mask (empty when lo > hi or lo > 63)
__device__ __forceinline__ unsigned long long ref_range(int lo, int hi)
{
  if (lo > hi || lo > 63) return 0ull;
  const unsigned long long upto = hi >= 63 ? ~0ull : (1ull << (hi + 1)) - 1ull;
  return upto & ~((1ull << lo) - 1ull);
}

// AC refinement (decode_mcu_AC_refine, jdphuff.c:501-645, statement by statement): one wave per restart segment, lane = zig-zag
// position.  Everything but a lane's own coefficient is wave-uniform: the cursor, the EOB run, the mask of nonzero positions.
__global__ void __launch_bounds__(64)
k_pdec_ac_refine(MjhConst C, MjhDecBatch B, const MjhDecProg *__restrict__ PS, int16_t *__restrict__ coef_q)
{
  __shared__ MjhDecScan sc;
  __shared__ MjhComp lc[MJH_MAXC];
  __shared__ MjhDecTable T;
  const MjhDecSeg seg = B.segs[blockIdx.x];
  dec_load_scan<64, false>(C, B, seg.scan, &sc, nullptr, lc);
  {
    const unsigned *ts = reinterpret_cast<const unsigned *>(B.tables + sc.actab[0]);
    unsigned *td = reinterpret_cast<unsigned *>(&T);
    for (unsigned i = threadIdx.x; i < sizeof(MjhDecTable) / 4; i += 64) td[i] = ts[i];
    __syncthreads();
  }
  const MjhDecProg ps = PS[seg.scan];
  const int Ss = ps.Ss < 1 ? 1 : ps.Ss, Se = ps.Se > 63 ? 63 : ps.Se;       // (the host checked them; the stores below rely on it)
  const int p1 = 1 << ps.Al, m1 = (int)(~0u << ps.Al);
  const int lane = (int)threadIdx.x;
  const MjhComp &cc = lc[0];
  const int nblk = cc.nblk;
  int16_t *mine = coef_q + (size_t)sc.image * C.coefs_per_image + cc.coef_off + (long long)lane * cc.kstride;
  const bool inband = lane >= Ss && lane <= Se;
  const int total = seg.nmcu;
  RefCursor R;
  R.d = B.bytes + seg.off; R.len = seg.len; R.bp = 0; R.bit = 0;
  unsigned eobrun = 0, flags = 0;
  bool bad = false;
  int c_next = (total > 0 && inband && seg.mcu0 >= 0 && seg.mcu0 < nblk) ? (int)mine[seg.mcu0] : 0;
  for (int i = 0; i < total; i++) {
    const int blk = seg.mcu0 + i;
    int c = c_next;
    // the next block's coefficients are on their way while this one is decoded
    c_next = (i + 1 < total && inband && blk + 1 >= 0 && blk + 1 < nblk) ? (int)mine[blk + 1] : 0;
    const unsigned long long M = __ballot(c != 0) & ref_range(Ss, Se);      // the positions of the band that are nonzero already
    bool changed = false;
    // the correction bits of the nonzero positions CM, in order of position, at the cursor: a lane takes its own by its rank
    auto correct = [&](unsigned long long CM) {
      const int ncor = __popcll(CM);
      if (ncor == 0) return;
      const unsigned long long w = R.win();
      if ((CM >> lane) & 1ull) {
        const int rank = __popcll(CM & ((1ull << lane) - 1ull));
        if (((w >> (63 - rank)) & 1ull) && (c & p1) == 0) { c += c >= 0 ? p1 : m1; changed = true; }
      }
      R.skip((unsigned)ncor);
    };
    int k = Ss;
    if (eobrun == 0u) {
      while (k <= Se) {
        const unsigned long long w = R.win();
        int nb;
        const int sym = dec_symbol(T, w, nb, bad);
        int r = sym >> 4;
        const int s = sym & 15;
        int newval = 0;
        if (s) {
          if (s != 1) bad = true;                                          // JWRN_HUFF_BAD_CODE: the size of a new coefficient is always 1
          newval = ((w << nb) >> 63) ? p1 : m1;
          R.skip((unsigned)nb + 1u);
        } else if (r != 15) {
          eobrun = 1u << r;
          if (r) eobrun += (unsigned)((w << nb) >> (64 - r));
          R.skip((unsigned)(nb + r));
          break;                                                           // the rest of the block is the EOB logic's
        } else R.skip((unsigned)nb);
        // over the nonzero positions and r zero ones, up to the zero position the run ends at (or past Se when the band ends first)
        unsigned long long Z = ~M & ref_range(k, Se);
        for (int t = 0; t < r && Z; t++) Z &= Z - 1ull;
        const int target = Z ? __ffsll((long long)Z) - 1 : Se + 1;
        correct(M & ref_range(k, target - 1));
        if (s && lane == (target > 63 ? 63 : target)) { c = newval; changed = true; }     // (*block)[jpeg_natural_order[k]] = s
        k = target + 1;
      }
    }
    if (eobrun > 0u) {
      correct(M & ref_range(k, Se));
      eobrun--;
    }
    if (changed && blk >= 0 && blk < nblk) mine[blk] = (int16_t)c;
    if (R.bp > R.len) break;                                               // (uniform) the data ended inside this block
  }
  // the segment's last block ends here: nothing but the padding of its last byte may follow, the cursor must not have passed the end,
  // and an EOB run must not reach beyond the segment
  if (bad || eobrun > 0u || dec_end_bad(R.d, R.len, R.bp, R.bit)) flags |= MJH_DEC_CORRUPT;
  if (flags && lane == 0) atomicOr(&B.status[sc.image], flags);
}

void mjh_launch_pdec_dc_refine(const MjhConst &C, const MjhDecBatch &B, const MjhDecProg *PS, int16_t *coef_q, hipStream_t s)
{
  hipLaunchKernelGGL(k_pdec_dc_refine, dim3(B.nseg), dim3(MJH_DEC_WG), 0, s, C, B, PS, coef_q);
}
void mjh_launch_pdec_ac_refine(const MjhConst &C, const MjhDecBatch &B, const MjhDecProg *PS, int16_t *coef_q, hipStream_t s)
{
  hipLaunchKernelGGL(k_pdec_ac_refine, dim3(B.nseg), dim3(64), 0, s, C, B, PS, coef_q);
}
