// mjh_decode_lossless.hip -- K-DL: lossless JPEG files (SOF3, Huffman-coded; jdlhuff.c, jdlossls.c, jddiffct.c) decoded on the device.
//
// Entropy decoder.  A lossless scan is a stream of DC-style symbols, one per sample: category s in 0..16 from the component's DC table,
// then s value bits extended as for DC (s = 16: the difference 32768 and no bits).  An interleaved MCU is one sample of each component
// of the scan.  That is the k == 0 branch of dec_run with one more category, so the scans go through the scheme of mjh_decode.hip as
// they are -- restart segments x self-synchronising subsequences, k_ldec_sync until the host reads "unchanged", k_dec_prefix,
// k_ldec_store -- with the phase bodies of mjh_decode_dev.h instantiated on ldec_run, the run function of this file.  The state a lane
// carries is (bit position, component inside the MCU); the count it leaves is samples.  The stores go to one plane of 16-bit
// differences per component ([H][Wp], Wp = W rounded up to 8 so that rows are 16-byte aligned); there is no DC-sum phase.
//
// Undifferencing, in place (plane of differences -> plane of reconstructed samples, both modulo 2^16):
//   k_ll_rows  one wave per row.  The first row of every restart interval is predicted from the left throughout, and its first sample
//              by 1 << (P - Pt - 1): a prefix sum along the row.  With predictor 1 every other row is one too, started from the sample
//              above its first, which is the initial prediction + the sum of column 0 down to that row (k_ll_col0, one wave per
//              interval, takes that chain first): every row of a predictor 1 component is independent of the others.
//   k_ll_wave  predictors 2..7, one wave per restart interval: a wavefront over strips of 63 rows.  Lane l > 0 owns row r0 + l and
//              runs one chunk of 8 columns behind lane l - 1, whose results of the step before are its Rb (and the last of the chunk
//              before that its Rc), taken across lanes; Ra stays in a register.  Lane 0 passes the row above the strip through (the
//              interval's first row, or the last row of the strip before), so all lanes run the same code.  Differences are loaded 8
//              steps ahead of their use.  Predictors 2, 3 and 4 are linear and could be scans of their own (down the columns, along
//              the diagonals, rows then columns); they take the wavefront here.
//   k_ll_pixels  sample << Pt, the components interleaved into the pixel layout, 4 pixels per lane.
// Every read is bounded by the segment's length, every store by the plane (row < H, column < Wp) or the pixel row, whatever the bytes say.
#include <hip/hip_runtime.h>
#include "mjh_device.h"
#include "mjh_decode.h"
#include "mjh_decode_dev.h"

// Decodes samples from (p, b) while the next code word starts in front of end_bits; the counterpart of dec_run.  n counts the samples
// completed here.  STORE: also while ord < total, the differences written; true when the segment's last sample was completed here.
// mcu: the index in the plane (row * W + column) of the sample `ord` is.
template <bool STORE>
__device__ __forceinline__ bool ldec_run(const MjhDecScan &sc, const MjhDecTable *T, DecReader &R, unsigned end_bits, unsigned &p, int &b, unsigned &n,
                                         unsigned ord, unsigned total, int mcu, int16_t *diff_img, unsigned &flags)
{
  bool bad = false;
  const int W = sc.mcus_per_row, Wp = (W + 7) & ~7;
  const long long plane = (long long)(sc.mcus / W) * Wp;
  long long at = 0;
  int col = 0;
  if (STORE) { const int row = mcu / W; col = mcu - row * W; at = (long long)row * Wp + col; }
  if (b < 0 || b >= sc.bpm) b = 0;
  while (p < end_bits) {
    if (STORE && ord >= total) break;
    const unsigned long long w = R.fetch(p);
    int nb;
    int s = dec_symbol(T[2 * b], w, nb, bad);
    if (s > 16) { s = 0; bad = true; }
    int v = 0, ext = s;
    if (s == 16) { v = 32768; ext = 0; }
    else if (s) v = dec_extend(w, nb, s);
    if (STORE && mcu >= 0 && mcu < sc.mcus) diff_img[sc.diff_off + (long long)b * plane + at] = (int16_t)v;
    p = R.advance(p, nb + ext);
    if (n <= total) n++;
    if (++b >= sc.bpm) {
      b = 0; mcu++;
      if (STORE) { at++; if (++col == W) { col = 0; at += Wp - W; } }
    }
    if (STORE) {
      ord++;
      if (ord >= total) { if (bad) flags |= MJH_DEC_CORRUPT; return true; }
    }
  }
  if (STORE && bad) flags |= MJH_DEC_CORRUPT;
  return false;
}

__global__ void __launch_bounds__(MJH_DEC_WG)
k_ldec_sync(MjhConst C, MjhDecBatch B, int q, int first) { dec_sync_body<MJH_DEC_LL>(C, B, nullptr, q, first); }
__global__ void __launch_bounds__(MJH_DEC_WG)
k_ldec_store(MjhConst C, MjhDecBatch B) { dec_store_body<MJH_DEC_LL, false>(C, B, nullptr, nullptr, nullptr); }

// 8 samples of a row as they lie in memory
__device__ __forceinline__ void ll_unpack(const uint4 v, unsigned a[8])
{
  a[0] = v.x & 0xFFFFu; a[1] = v.x >> 16; a[2] = v.y & 0xFFFFu; a[3] = v.y >> 16;
  a[4] = v.z & 0xFFFFu; a[5] = v.z >> 16; a[6] = v.w & 0xFFFFu; a[7] = v.w >> 16;
}
__device__ __forceinline__ uint4 ll_pack(const unsigned a[8])
{
  return make_uint4((a[0] & 0xFFFFu) | (a[1] << 16), (a[2] & 0xFFFFu) | (a[3] << 16), (a[4] & 0xFFFFu) | (a[5] << 16), (a[6] & 0xFFFFu) | (a[7] << 16));
}

// Predictor 1: what lies above the first sample of every row -- the initial prediction + column 0 of the interval's rows above it (the
// rows themselves are rewritten in place by k_ll_rows, so the chain is taken first).  One wave per restart interval.
__global__ void __launch_bounds__(64)
k_ll_col0(MjhLlGeom G, const MjhLlPlane *__restrict__ planes, const int16_t *__restrict__ diff, unsigned *__restrict__ above)
{
  const MjhLlPlane pl = planes[blockIdx.y];
  const int rows = pl.rows < 1 ? 1 : pl.rows, lane = (int)threadIdx.x;
  const long long first = (long long)blockIdx.x * rows;
  if (pl.psv != 1 || first >= G.H) return;                        // (uniform)
  if (pl.off < 0 || pl.off + (long long)G.H * G.Wp > G.per_image) return;
  const int y0 = (int)first, y1 = first + rows < G.H ? (int)(first + rows) : G.H;
  const uint16_t *plane = reinterpret_cast<const uint16_t *>(diff) + (size_t)(blockIdx.y / (unsigned)G.ncomp) * (size_t)G.per_image + (size_t)pl.off;
  unsigned carry = 1u << (G.precision - pl.pt - 1);
  for (int r0 = y0; r0 < y1; r0 += 64) {                          // (uniform)
    const int y = r0 + lane;
    const unsigned v = y < y1 ? (unsigned)plane[(size_t)y * G.Wp] : 0u;
    unsigned incl = v;
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned t = __shfl_up(incl, (unsigned)o);
      if (lane >= o) incl += t;
    }
    if (y < y1) above[(size_t)blockIdx.y * (size_t)G.H + (size_t)y] = carry + incl - v;
    carry += __shfl(incl, 63);
  }
}

// Rows that are a prefix sum: every row of a predictor 1 plane, the first row of every restart interval of the others.
__global__ void __launch_bounds__(64)
k_ll_rows(MjhLlGeom G, const MjhLlPlane *__restrict__ planes, int16_t *__restrict__ diff, const unsigned *__restrict__ above)
{
  const MjhLlPlane pl = planes[blockIdx.y];
  const int y = (int)blockIdx.x, lane = (int)threadIdx.x;
  const int rows = pl.rows < 1 ? 1 : pl.rows;
  if (y >= G.H || (pl.psv != 1 && y % rows != 0)) return;        // (uniform)
  if (pl.off < 0 || pl.off + (long long)G.H * G.Wp > G.per_image) return;
  uint16_t *plane = reinterpret_cast<uint16_t *>(diff) + (size_t)(blockIdx.y / (unsigned)G.ncomp) * (size_t)G.per_image + (size_t)pl.off;
  unsigned carry = pl.psv == 1 ? above[(size_t)blockIdx.y * (size_t)G.H + (size_t)y] : 1u << (G.precision - pl.pt - 1);
  uint4 *row = reinterpret_cast<uint4 *>(plane + (size_t)y * G.Wp);
  const int nchunk = G.Wp >> 3;
  for (int c0 = 0; c0 < nchunk; c0 += 64) {                       // (uniform)
    const int c = c0 + lane;
    unsigned a[8];
    ll_unpack(c < nchunk ? row[c] : make_uint4(0u, 0u, 0u, 0u), a);
#pragma unroll
    for (int t = 1; t < 8; t++) a[t] += a[t - 1];
    unsigned incl = a[7];
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned v = __shfl_up(incl, (unsigned)o);
      if (lane >= o) incl += v;
    }
    const unsigned before = carry + incl - a[7];
#pragma unroll
    for (int t = 0; t < 8; t++) a[t] += before;
    if (c < nchunk) row[c] = ll_pack(a);
    carry += __shfl(incl, 63);
  }
}

template <int PSV>
__device__ __forceinline__ unsigned ll_predict(unsigned Ra, unsigned Rb, unsigned Rc)
{
  if (PSV == 2) return Rb;
  if (PSV == 3) return Rc;
  if (PSV == 4) return Ra + Rb - Rc;
  if (PSV == 5) return Ra + (unsigned)(((int)Rb - (int)Rc) >> 1);
  if (PSV == 6) return Rb + (unsigned)(((int)Ra - (int)Rc) >> 1);
  return (Ra + Rb) >> 1;
}

__device__ __forceinline__ uint4 ll_chunk(const uint4 *row, int c, int nchunk, bool act)
{
  return (act && c >= 0 && c < nchunk) ? row[c] : make_uint4(0u, 0u, 0u, 0u);
}

// rows (y0, y1) of a plane whose row y0 is reconstructed already
template <int PSV>
__device__ __forceinline__ void ll_strips(uint16_t *plane, int y0, int y1, int Wp)
{
  const int lane = (int)threadIdx.x, nchunk = Wp >> 3, nmacro = (nchunk + 63 + 7) >> 3;
  for (int r0 = y0; r0 + 1 < y1; r0 += 63) {                      // (uniform)
    const int y = r0 + lane;
    const bool act = y < y1;
    uint4 *mine = reinterpret_cast<uint4 *>(plane + (size_t)(act ? y : r0) * Wp);
    uint4 q[8];
#pragma unroll
    for (int i = 0; i < 8; i++) q[i] = ll_chunk(mine, i - lane, nchunk, act);
    uint4 res = make_uint4(0u, 0u, 0u, 0u);
    unsigned ra = 0, rc = 0;
    for (int m = 0; m < nmacro; m++) {
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const int c = 8 * m + i - lane;
        uint4 up;                         // what the lane above made in the step before: the chunk above mine
        up.x = __shfl_up(res.x, 1u);
        up.y = __shfl_up(res.y, 1u);
        up.z = __shfl_up(res.z, 1u);
        up.w = __shfl_up(res.w, 1u);
        const uint4 d = q[i];
        q[i] = ll_chunk(mine, c + 8, nchunk, act);
        if (act && c >= 0 && c < nchunk) {
          if (lane == 0) res = d;         // the row above the strip, as it is
          else {
            unsigned dv[8], ub[8];
            ll_unpack(d, dv);
            ll_unpack(up, ub);
#pragma unroll
            for (int t = 0; t < 8; t++) {
              const unsigned Rb = ub[t], Rc = t ? ub[t - 1] : rc;
              const unsigned pred = (c == 0 && t == 0) ? Rb : ll_predict<PSV>(ra, Rb, Rc);
              ra = (dv[t] + pred) & 0xFFFFu;
              dv[t] = ra;
            }
            rc = ub[7];
            res = ll_pack(dv);
            mine[c] = res;
          }
        }
      }
    }
    __syncthreads();                      // the strip's last row is the row above the next strip
  }
}

__global__ void __launch_bounds__(64)
k_ll_wave(MjhLlGeom G, const MjhLlPlane *__restrict__ planes, int16_t *__restrict__ diff)
{
  const MjhLlPlane pl = planes[blockIdx.y];
  const int rows = pl.rows < 1 ? 1 : pl.rows;
  const long long first = (long long)blockIdx.x * rows;
  if (pl.psv < 2 || pl.psv > 7 || first >= G.H) return;          // (uniform)
  if (pl.off < 0 || pl.off + (long long)G.H * G.Wp > G.per_image) return;
  const int y0 = (int)first, y1 = first + rows < G.H ? (int)(first + rows) : G.H;
  uint16_t *plane = reinterpret_cast<uint16_t *>(diff) + (size_t)(blockIdx.y / (unsigned)G.ncomp) * (size_t)G.per_image + (size_t)pl.off;
  switch (pl.psv) {
  case 2: ll_strips<2>(plane, y0, y1, G.Wp); break;
  case 3: ll_strips<3>(plane, y0, y1, G.Wp); break;
  case 4: ll_strips<4>(plane, y0, y1, G.Wp); break;
  case 5: ll_strips<5>(plane, y0, y1, G.Wp); break;
  case 6: ll_strips<6>(plane, y0, y1, G.Wp); break;
  default: ll_strips<7>(plane, y0, y1, G.Wp); break;
  }
}

// The output scaler (jdlossls.c: sample << Al, stored in the sample's type) and the pixel layout: 4 pixels of PX samples of BYTES bytes
// per lane, PX * BYTES dwords.
template <int BYTES, int PX>
__global__ void __launch_bounds__(256)
k_ll_pixels(MjhLlGeom G, const MjhLlPlane *__restrict__ planes, const int16_t *__restrict__ diff, MjhLlOut O, uint8_t *__restrict__ pixels,
            const unsigned *__restrict__ status)
{
  constexpr int NDW = PX * BYTES, NC = PX == 1 ? 1 : 3;
  const int g = (int)(blockIdx.x * 256u + threadIdx.x), y = (int)blockIdx.y, img = (int)blockIdx.z;
  if (g >= ((G.W + 3) >> 2) || y >= G.H) return;
  unsigned out[NDW];
#pragma unroll
  for (int i = 0; i < NDW; i++) out[i] = 0u;
  if (status[img] == 0u) {
    unsigned sv[NC][4];
#pragma unroll
    for (int c = 0; c < NC; c++) {
      const MjhLlPlane pl = planes[img * G.ncomp + c];
      const uint16_t *row = reinterpret_cast<const uint16_t *>(diff) + (size_t)img * (size_t)G.per_image + (size_t)pl.off + (size_t)y * G.Wp;
      const uint2 v = *reinterpret_cast<const uint2 *>(row + 4 * g);
      sv[c][0] = (v.x & 0xFFFFu) << pl.pt; sv[c][1] = (v.x >> 16) << pl.pt;
      sv[c][2] = (v.y & 0xFFFFu) << pl.pt; sv[c][3] = (v.y >> 16) << pl.pt;
    }
#pragma unroll
    for (int px = 0; px < 4; px++)
#pragma unroll
      for (int k = 0; k < PX; k++) {
        unsigned val;
        if (PX == 1) val = sv[0][px];
        else val = k == O.off[0] ? sv[0][px] : k == O.off[1] ? sv[1 % NC][px] : k == O.off[2] ? sv[2 % NC][px] : (unsigned)O.fill;
        const int idx = px * PX + k;
        if (BYTES == 1) out[idx >> 2] |= (val & 0xFFu) << ((idx & 3) * 8);
        else out[idx >> 1] |= (val & 0xFFFFu) << ((idx & 1) * 16);
      }
  }
  const int yo = O.bottom_up ? G.H - 1 - y : y;
  uint8_t *dst = pixels + (size_t)img * (size_t)O.image_stride + (size_t)yo * (size_t)O.row_pitch + (size_t)g * (NDW * 4);
  if (NDW % 4 == 0) {
#pragma unroll
    for (int i = 0; i < NDW / 4; i++) reinterpret_cast<uint4 *>(dst)[i] = make_uint4(out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3]);
  } else if (NDW % 2 == 0) {
#pragma unroll
    for (int i = 0; i < NDW / 2; i++) reinterpret_cast<uint2 *>(dst)[i] = make_uint2(out[2 * i], out[2 * i + 1]);
  } else {
#pragma unroll
    for (int i = 0; i < NDW; i++) reinterpret_cast<unsigned *>(dst)[i] = out[i];
  }
}

void mjh_launch_ldec_sync(const MjhConst &C, const MjhDecBatch &B, int q, int first, hipStream_t s)
{
  hipLaunchKernelGGL(k_ldec_sync, dim3(B.nsub_padded / MJH_DEC_WG), dim3(MJH_DEC_WG), 0, s, C, B, q, first);
}
void mjh_launch_ldec_store(const MjhConst &C, const MjhDecBatch &B, hipStream_t s)
{
  hipLaunchKernelGGL(k_ldec_store, dim3(B.nsub_padded / MJH_DEC_WG), dim3(MJH_DEC_WG), 0, s, C, B);
}
void mjh_launch_ll_undiff(const MjhLlGeom &G, const MjhLlPlane *planes, int16_t *diff, unsigned *above, int n, hipStream_t s)
{
  hipLaunchKernelGGL(k_ll_col0, dim3(G.max_intervals, n * G.ncomp), dim3(64), 0, s, G, planes, diff, above);
  hipLaunchKernelGGL(k_ll_rows, dim3(G.H, n * G.ncomp), dim3(64), 0, s, G, planes, diff, above);
  hipLaunchKernelGGL(k_ll_wave, dim3(G.max_intervals, n * G.ncomp), dim3(64), 0, s, G, planes, diff);
}
void mjh_launch_ll_pixels(const MjhLlGeom &G, const MjhLlPlane *planes, const int16_t *diff, const MjhLlOut &O, uint8_t *pixels, const unsigned *status, int n, hipStream_t s)
{
  const dim3 grid((((G.W + 3) >> 2) + 255) / 256, G.H, n), wg(256);
  const bool wide = G.precision > 8;
  if (O.px == 1) {
    if (wide) hipLaunchKernelGGL((k_ll_pixels<2, 1>), grid, wg, 0, s, G, planes, diff, O, pixels, status);
    else hipLaunchKernelGGL((k_ll_pixels<1, 1>), grid, wg, 0, s, G, planes, diff, O, pixels, status);
  } else if (O.px == 3) {
    if (wide) hipLaunchKernelGGL((k_ll_pixels<2, 3>), grid, wg, 0, s, G, planes, diff, O, pixels, status);
    else hipLaunchKernelGGL((k_ll_pixels<1, 3>), grid, wg, 0, s, G, planes, diff, O, pixels, status);
  } else {
    if (wide) hipLaunchKernelGGL((k_ll_pixels<2, 4>), grid, wg, 0, s, G, planes, diff, O, pixels, status);
    else hipLaunchKernelGGL((k_ll_pixels<1, 4>), grid, wg, 0, s, G, planes, diff, O, pixels, status);
  }
}
