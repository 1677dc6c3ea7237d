// mjh_idct.hip -- K-I: from the quantized coefficient planes the Huffman decoder leaves (mjh_decode.hip) to interleaved 8-bit
// pixels (mjh_decode_host).  Integer-only, bit-exact with the reference's decompressor as djpeg drives it: JDCT_ISLOW, the C
// upsamplers (no SIMD), fancy upsampling on or off.
//
// K-I1 k_idct: one lane per real block.  Dequantization inside the transform (DEQUANTIZE jdct.h, multiplier = quantval
//   jddctmgr.c), the two passes of jpeg_idct_islow (jidctint.c:173-413) in 64-bit arithmetic as the reference's JLONG (a
//   damaged or hostile file reaches products beyond 32 bits, and the descaling shifts do not commute with a wrap), the
//   workspace truncated to int between the passes as there, and the post-IDCT range-limit table reproduced WITH its wrap
//   (prepare_range_limit_table jdmaster.c:415ff: index & 1023).  The zero-AC shortcuts of the reference give the numbers of the
//   general path and are not branches here.
//   Memory: plane k of coef_q is read by 64 consecutive blocks per wave (coalesced 128-byte rows); the 8 x 8 samples of a block
//   leave as eight 8-byte vector stores, one per sample row: the lanes of a wave hold horizontally adjacent blocks, so every
//   store instruction writes one contiguous 512-byte run of a sample row.  The rows wait in registers; a pass through LDS would
//   add a write and a read per sample and change nothing about the shape of the stores.
// K-I1f k_idct_ifast: the same grid, loads and stores with the arithmetic of jpeg_idct_ifast (jidctfst.c), for djpeg -dct fast
//   and TurboJPEG's FASTDCT; see the kernel.
// K-I1s k_idct_scaled<N>: the same at DCT_scaled_size N = 1, 2, 4 (jidctred.c), one component per launch, for djpeg -scale.
//   Fewer coefficient planes read, N x N samples per block written; see the kernel.  Components a scaled decode leaves at
//   size 8 (and every component of an unscaled call) go through k_idct, or k_idct_ifast when the call asks for the fast method
//   (jddctmgr.c start_pass consults dct_method at size 8 only).
// K-I2 k_upcolor: one lane per 4 output pixels of a row.  Per component the upsampler jinit_upsampler picks (jdsample.c:444-525),
//   evaluated per output sample from the samples it reads, then the colour conversion of jdcolor.c / jdcolext.c, then one 4-byte,
//   three 4-byte (12 contiguous bytes) or one 16-byte store (rows of the output hold whole groups of 4 pixels).
//   Edges: neighbours are clamped to [0, downsampled_width) x [0, downsampled_height), which is what the special
//   first / last column cases of the fancy upsamplers (jdsample.c:289-303, :386-404) and the duplicated context rows of the main
//   controller (jdmainct.c make_funny_pointers / set_bottom_pointers) amount to; samples beyond are never read.
// K-I2' k_upcolor_565: the same lanes for JCS_RGB565 (djpeg -rgb565): 4 packed 16-bit pixels, one 8-byte store, with or without
//   the reference's ordered dither; see the kernel.
// K-I2'' k_upcolor4: the same lanes for the four-component files (CMYK, YCCK): 4 pixels of C, M, Y, K, one 16-byte store; see the kernel.
#include <hip/hip_runtime.h>
#include "mjh_device.h"
#include "mjh_idct.h"

// zig-zag position of every natural-order position (the inverse of jpeg_natural_order)
__constant__ int kZigOfNat[64] = {
   0,  1,  5,  6, 14, 15, 27, 28,
   2,  4,  7, 13, 16, 26, 29, 42,
   3,  8, 12, 17, 25, 30, 41, 43,
   9, 11, 18, 24, 31, 40, 44, 53,
  10, 19, 23, 32, 39, 45, 52, 54,
  20, 22, 33, 38, 46, 51, 55, 60,
  21, 34, 37, 47, 50, 56, 59, 61,
  35, 36, 48, 49, 57, 58, 62, 63 };

// the 1-D inverse transform of jidctint.c (CONST_BITS 13): eight inputs -> the eight sums in front of the descaling shift
__device__ __forceinline__ void idct8(const int (&x)[8], long long (&o)[8])
{
  long long z2 = x[2], z3 = x[6];
  long long z1 = (z2 + z3) * 4433;                     // FIX_0_541196100
  long long tmp2 = z1 - z3 * 15137;                    // FIX_1_847759065
  long long tmp3 = z1 + z2 * 6270;                     // FIX_0_765366865
  long long tmp0 = ((long long)x[0] + x[4]) * 8192;
  long long tmp1 = ((long long)x[0] - x[4]) * 8192;
  const long long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = x[7]; tmp1 = x[5]; tmp2 = x[3]; tmp3 = x[1];
  z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
  long long z4 = tmp1 + tmp3;
  const long long z5 = (z3 + z4) * 9633;               // FIX_1_175875602
  tmp0 *= 2446;                                        // FIX_0_298631336
  tmp1 *= 16819;                                       // FIX_2_053119869
  tmp2 *= 25172;                                       // FIX_3_072711026
  tmp3 *= 12299;                                       // FIX_1_501321110
  z1 *= -7373;                                         // FIX_0_899976223
  z2 *= -20995;                                        // FIX_2_562915447
  z3 = z3 * -16069 + z5;                               // FIX_1_961570560
  z4 = z4 * -3196 + z5;                                // FIX_0_390180644
  tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
  o[0] = tmp10 + tmp3; o[7] = tmp10 - tmp3;
  o[1] = tmp11 + tmp2; o[6] = tmp11 - tmp2;
  o[2] = tmp12 + tmp1; o[5] = tmp12 - tmp1;
  o[3] = tmp13 + tmp0; o[4] = tmp13 - tmp0;
}

// the post-IDCT table of prepare_range_limit_table at index v & 1023: 128..255, 255 x 384, 0 x 384, 0..127
__device__ __forceinline__ unsigned idct_range_limit(int v)
{
  v &= 1023;
  return (unsigned)(v < 128 ? v + 128 : (v < 512 ? 255 : (v < 896 ? 0 : v - 896)));
}

__global__ void __launch_bounds__(256)
k_idct(MjhConst C, MjhIdctQ Q, const int16_t *__restrict__ coef_q, uint8_t *__restrict__ planes, const unsigned *__restrict__ status)
{
  const int img = blockIdx.z, ci = blockIdx.y;
  const MjhComp &cc = C.c[ci];
  const int b = (int)(blockIdx.x * 256u + threadIdx.x);
  if (b >= cc.nblk) return;
  if (status[img] != 0u) return;
  const int16_t *in = coef_q + (size_t)img * C.coefs_per_image + cc.coef_off + b;
  const int *q = Q.q[ci];
  int ws[64];
  // pass 1: columns, results scaled up by 2^PASS1_BITS (2)
#pragma unroll
  for (int c = 0; c < 8; c++) {
    int x[8];
#pragma unroll
    for (int r = 0; r < 8; r++) x[r] = (int)in[(size_t)kZigOfNat[r * 8 + c] * cc.kstride] * q[r * 8 + c];
    long long o[8];
    idct8(x, o);
#pragma unroll
    for (int r = 0; r < 8; r++) ws[r * 8 + c] = (int)((o[r] + 1024) >> 11);
  }
  // pass 2: rows; descale by 2^(CONST_BITS + PASS1_BITS + 3), then the range limit with the sample's centre added
  const int by = b / cc.wib, bx = b - by * cc.wib;
  uint8_t *out = planes + (size_t)img * C.planes_per_image + cc.plane_off + (size_t)(by * 8) * cc.pw + (size_t)bx * 8;
#pragma unroll
  for (int r = 0; r < 8; r++) {
    int x[8];
#pragma unroll
    for (int c = 0; c < 8; c++) x[c] = ws[r * 8 + c];
    long long o[8];
    idct8(x, o);
    unsigned s[8];
#pragma unroll
    for (int c = 0; c < 8; c++) s[c] = idct_range_limit((int)((o[c] + (1 << 17)) >> 18));
    uint2 v;
    v.x = s[0] | (s[1] << 8) | (s[2] << 16) | (s[3] << 24);
    v.y = s[4] | (s[5] << 8) | (s[6] << 16) | (s[7] << 24);
    *reinterpret_cast<uint2 *>(out + (size_t)r * cc.pw) = v;
  }
}

// ---- K-I1 with the fast integer method (djpeg -dct fast, JDCT_IFAST): jpeg_idct_ifast jidctfst.c:170-368 --------------------------
// As the reference built for 8-bit samples without SIMD has it: DCTELEM and the multipliers are int, CONST_BITS 8, PASS1_BITS 2.
// MULTIPLY is a 64-bit product (its constant is a JLONG) shifted right by 8 WITHOUT rounding and cast back to int; every sum
// and the dequantizing product are int.  Where those overflow (absurd quantization tables only: real files stay far inside)
// the reference's behaviour is undefined; here they wrap in two's complement -- the sums are unsigned arithmetic.
__device__ __forceinline__ unsigned ifast_mul(unsigned v, int c) { return (unsigned)(int)(((long long)(int)v * c) >> 8); }

// the 1-D transform of both passes: eight inputs -> the eight sums in front of the final shift (pass 1 has none)
__device__ __forceinline__ void idct8_ifast(const unsigned (&x)[8], unsigned (&o)[8])
{
  unsigned tmp10 = x[0] + x[4], tmp11 = x[0] - x[4];
  const unsigned tmp13 = x[2] + x[6];
  unsigned tmp12 = ifast_mul(x[2] - x[6], 362) - tmp13;          // FIX_1_414213562
  const unsigned tmp0 = tmp10 + tmp13, tmp3 = tmp10 - tmp13, tmp1 = tmp11 + tmp12, tmp2 = tmp11 - tmp12;
  const unsigned z13 = x[5] + x[3], z10 = x[5] - x[3], z11 = x[1] + x[7], z12 = x[1] - x[7];
  const unsigned tmp7 = z11 + z13;
  tmp11 = ifast_mul(z11 - z13, 362);
  const unsigned z5 = ifast_mul(z10 + z12, 473);                 // FIX_1_847759065
  tmp10 = ifast_mul(z12, 277) - z5;                              // FIX_1_082392200
  tmp12 = ifast_mul(z10, -669) + z5;                             // -FIX_2_613125930
  const unsigned tmp6 = tmp12 - tmp7, tmp5 = tmp11 - tmp6, tmp4 = tmp10 + tmp5;
  o[0] = tmp0 + tmp7; o[7] = tmp0 - tmp7;
  o[1] = tmp1 + tmp6; o[6] = tmp1 - tmp6;
  o[2] = tmp2 + tmp5; o[5] = tmp2 - tmp5;
  o[4] = tmp3 + tmp4; o[3] = tmp3 - tmp4;
}

// One lane per real block: the grid, the loads and the eight 8-byte row stores of k_idct.  Q holds the AA&N multipliers the
// host made (mjh_idct.h), not quantval.  The reference's zero-AC shortcuts are no branches here: a column whose AC terms are
// zero leaves MULTIPLY(0, c) = 0 everywhere, so every output of the general path is the dequantized DC, which is what the
// shortcut stores (jidctfst.c:205-228); a workspace row with zero AC terms gives IDESCALE(ws[0], 5) eight times on either
// path (:284-304).
__global__ void __launch_bounds__(256)
k_idct_ifast(MjhConst C, MjhIdctQ Q, const int16_t *__restrict__ coef_q, uint8_t *__restrict__ planes, const unsigned *__restrict__ status)
{
  const int img = blockIdx.z, ci = blockIdx.y;
  const MjhComp &cc = C.c[ci];
  const int b = (int)(blockIdx.x * 256u + threadIdx.x);
  if (b >= cc.nblk) return;
  if (status[img] != 0u) return;
  const int16_t *in = coef_q + (size_t)img * C.coefs_per_image + cc.coef_off + b;
  const int *q = Q.q[ci];
  unsigned ws[64];
  // pass 1: columns; the multipliers carry the 2^PASS1_BITS the workspace is scaled up by
#pragma unroll
  for (int c = 0; c < 8; c++) {
    unsigned x[8], o[8];
#pragma unroll
    for (int r = 0; r < 8; r++) x[r] = (unsigned)(int)in[(size_t)kZigOfNat[r * 8 + c] * cc.kstride] * (unsigned)q[r * 8 + c];
    idct8_ifast(x, o);
#pragma unroll
    for (int r = 0; r < 8; r++) ws[r * 8 + c] = o[r];
  }
  // pass 2: rows; a plain shift by PASS1_BITS + 3, then the range limit with the sample's centre added
  const int by = b / cc.wib, bx = b - by * cc.wib;
  uint8_t *out = planes + (size_t)img * C.planes_per_image + cc.plane_off + (size_t)(by * 8) * cc.pw + (size_t)bx * 8;
#pragma unroll
  for (int r = 0; r < 8; r++) {
    unsigned x[8], o[8];
#pragma unroll
    for (int c = 0; c < 8; c++) x[c] = ws[r * 8 + c];
    idct8_ifast(x, o);
    unsigned s[8];
#pragma unroll
    for (int c = 0; c < 8; c++) s[c] = idct_range_limit((int)o[c] >> 5);
    uint2 v;
    v.x = s[0] | (s[1] << 8) | (s[2] << 16) | (s[3] << 24);
    v.y = s[4] | (s[5] << 8) | (s[6] << 16) | (s[7] << 24);
    *reinterpret_cast<uint2 *>(out + (size_t)r * cc.pw) = v;
  }
}

// ---- K-I1 at a reduced size (djpeg -scale): the transforms of jidctred.c ------------------------------------------------------
// which of the eight coefficients of a column or row the transform to N samples reads: all but 4 (4), 0 and the odd ones (2),
// the DC alone (1); a further size of jidctint.c is one more line here and one more idct_1d
__host__ __device__ constexpr bool idct_reads(int N, int i) { return N == 4 ? i != 4 : (N == 2 ? (i == 0 || (i & 1)) : i == 0); }

// the 1-D transforms, chosen by the number of outputs: the sums in front of the descaling shift.  Those of jidctred.c carry
// one (4 outputs) or two (2 outputs) more fraction bits than jidctint.c's (its LEFT_SHIFT of the DC by CONST_BITS + 1 / + 2).
__device__ __forceinline__ void idct_1d(const int (&x)[8], long long (&o)[4])     // jpeg_idct_4x4 jidctred.c:160-199
{
  const long long tmp0 = (long long)x[0] * 16384;
  const long long tmp2 = (long long)x[2] * 15137 + (long long)x[6] * -6270;      // FIX_1_847759065, -FIX_0_765366865
  const long long tmp10 = tmp0 + tmp2, tmp12 = tmp0 - tmp2;
  const long long z1 = x[7], z2 = x[5], z3 = x[3], z4 = x[1];
  const long long odd0 = z1 * -1730 + z2 * 11893 + z3 * -17799 + z4 * 8697;      // -FIX_0_211164243 FIX_1_451774981 -FIX_2_172734803 FIX_1_061594337
  const long long odd2 = z1 * -4176 + z2 * -4926 + z3 * 7373 + z4 * 20995;       // -FIX_0_509795579 -FIX_0_601344887 FIX_0_899976223 FIX_2_562915447
  o[0] = tmp10 + odd2; o[3] = tmp10 - odd2;
  o[1] = tmp12 + odd0; o[2] = tmp12 - odd0;
}
__device__ __forceinline__ void idct_1d(const int (&x)[8], long long (&o)[2])     // jpeg_idct_2x2 jidctred.c:316-335
{
  const long long tmp10 = (long long)x[0] * 32768;
  // -FIX_0_720959822 FIX_0_850430095 -FIX_1_272758580 FIX_3_624509785
  const long long tmp0 = (long long)x[7] * -5906 + (long long)x[5] * 6967 + (long long)x[3] * -10426 + (long long)x[1] * 29692;
  o[0] = tmp10 + tmp0; o[1] = tmp10 - tmp0;
}

// one block to its N x N samples, OR-ed into the row words w at byte j * N of every row (j: the block's place in its lane's
// group).  `in`: the block's entry of zig-zag plane 0.  Only the planes idct_reads names are loaded.
// The zero-AC shortcuts of both passes of jidctred.c are the general formulas with zeros put in and are no
// branches here.
template <int N>
__device__ __forceinline__ void idct_block(const int16_t *__restrict__ in, int kstride, const int *__restrict__ q, unsigned (&w)[N], int j)
{
  constexpr int X = N == 4 ? 1 : 2;                    // the fraction bits the 1-D sums carry beyond jidctint.c's
  int ws[N][8];
#pragma unroll
  for (int c = 0; c < 8; c++) {
    if (!idct_reads(N, c)) {
#pragma unroll
      for (int r = 0; r < N; r++) ws[r][c] = 0;
      continue;
    }
    int x[8];
#pragma unroll
    for (int r = 0; r < 8; r++) x[r] = idct_reads(N, r) ? (int)in[(size_t)kZigOfNat[r * 8 + c] * kstride] * q[r * 8 + c] : 0;
    long long o[N];
    idct_1d(x, o);
#pragma unroll
    for (int r = 0; r < N; r++) ws[r][c] = (int)((o[r] + (1LL << (10 + X))) >> (11 + X));
  }
#pragma unroll
  for (int r = 0; r < N; r++) {
    long long o[N];
    idct_1d(ws[r], o);
#pragma unroll
    for (int c = 0; c < N; c++) w[r] |= idct_range_limit((int)((o[c] + (1LL << (17 + X))) >> (18 + X))) << (8 * (j * N + c));
  }
}
template <>
__device__ __forceinline__ void idct_block<1>(const int16_t *__restrict__ in, int, const int *__restrict__ q, unsigned (&w)[1], int j)
{
  w[0] |= idct_range_limit((int)(((long long)((int)in[0] * q[0]) + 4) >> 3)) << (8 * j);       // jpeg_idct_1x1: one eighth of the DC
}

// One lane per G = 4 / N horizontally adjacent blocks of component ci: a lane holds N rows of four samples and stores each as
// one word, and the lanes of a wave write one contiguous run per sample row.  pitch: samples between rows of the reduced
// plane, a multiple of 4 that holds ceil(wib / G) such words; the blocks a last group has beyond wib are not read and leave
// zeros in that pad.
template <int N>
__global__ void __launch_bounds__(256)
k_idct_scaled(MjhConst C, MjhIdctQ Q, int ci, int pitch, const int16_t *__restrict__ coef_q, uint8_t *__restrict__ planes, const unsigned *__restrict__ status)
{
  constexpr int G = 4 / N;
  const int img = blockIdx.z;
  const MjhComp &cc = C.c[ci];
  const int gpr = (cc.wib + G - 1) / G;
  const int t = (int)(blockIdx.x * 256u + threadIdx.x);
  if (t >= gpr * cc.hib) return;
  if (status[img] != 0u) return;
  const int by = t / gpr, gx = t - by * gpr;
  const int16_t *in = coef_q + (size_t)img * C.coefs_per_image + cc.coef_off + (size_t)by * cc.wib;
  unsigned w[N];
#pragma unroll
  for (int r = 0; r < N; r++) w[r] = 0u;
#pragma unroll
  for (int j = 0; j < G; j++) {
    const int bx = gx * G + j;
    if (bx >= cc.wib) continue;
    idct_block<N>(in + bx, cc.kstride, Q.q[ci], w, j);
  }
  uint8_t *out = planes + (size_t)img * C.planes_per_image + cc.plane_off + (size_t)(by * N) * pitch + (size_t)gx * 4;
#pragma unroll
  for (int r = 0; r < N; r++) *reinterpret_cast<unsigned *>(out + (size_t)r * pitch) = w[r];
}

// one sample of component uc at output position (x, y), 0 <= x < W, 0 <= y < H
__device__ __forceinline__ int up_sample(const MjhUpComp &uc, const uint8_t *__restrict__ pl, int x, int y)
{
  if (uc.mode == MJH_UP_REPLICATE) {
    int c = x / uc.hexp, r = y / uc.vexp;
    c = c < uc.dw ? c : uc.dw - 1; r = r < uc.dh ? r : uc.dh - 1;
    return pl[(size_t)r * uc.pw + c];
  }
  if (uc.mode == MJH_UP_H2V1_FANCY) {                  // jdsample.c:276-305
    const int c = x >> 1, odd = x & 1;
    int n = odd ? c + 1 : c - 1;
    n = n < 0 ? 0 : (n < uc.dw ? n : uc.dw - 1);
    const uint8_t *row = pl + (size_t)y * uc.pw;
    return (3 * (int)row[c] + (int)row[n] + 1 + odd) >> 2;
  }
  const int r = y >> 1, below = y & 1;
  int rn = below ? r + 1 : r - 1;
  rn = rn < 0 ? 0 : (rn < uc.dh ? rn : uc.dh - 1);
  const uint8_t *row0 = pl + (size_t)r * uc.pw, *row1 = pl + (size_t)rn * uc.pw;
  if (uc.mode == MJH_UP_H1V2_FANCY)                    // jdsample.c:316-350
    return (3 * (int)row0[x] + (int)row1[x] + 1 + below) >> 2;
  const int c = x >> 1, odd = x & 1;                   // h2v2_fancy_upsample jdsample.c:362-408
  int n = odd ? c + 1 : c - 1;
  n = n < 0 ? 0 : (n < uc.dw ? n : uc.dw - 1);
  const int here = 3 * (int)row0[c] + (int)row1[c], there = 3 * (int)row0[n] + (int)row1[n];
  return (3 * here + there + 8 - odd) >> 4;
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__global__ void __launch_bounds__(256)
k_upcolor(MjhPixOut P, const uint8_t *__restrict__ planes, uint8_t *__restrict__ pixels, const unsigned *__restrict__ status)
{
  const int img = blockIdx.z, y = blockIdx.y;
  const int x0 = (int)(blockIdx.x * 256u + threadIdx.x) * 4;
  if (x0 >= P.W) return;
  if (status[img] != 0u) return;
  const uint8_t *pl = planes + (size_t)img * P.planes_per_image;
  const int yo = P.bottom_up ? P.H - 1 - y : y;          // the output row image row y goes to
  unsigned px[4][3];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int x = x0 + i < P.W ? x0 + i : P.W - 1;      // (the pad of the last group: an in-range position, its bytes mean nothing)
    const int a = up_sample(P.c[0], pl + P.c[0].plane_off, x, y);
    int r = a, g = a, b = a;
    if (P.ncomp == 3) {
      const int c1 = up_sample(P.c[1], pl + P.c[1].plane_off, x, y), c2 = up_sample(P.c[2], pl + P.c[2].plane_off, x, y);
      if (P.conv == MJH_CC_YCC_RGB) {                  // ycc_rgb_convert with the tables of build_ycc_rgb_table (jdcolor.c:215-251), SCALEBITS 16
        const int cb = c1 - 128, cr = c2 - 128;
        r = clamp255(a + ((91881 * cr + 32768) >> 16));
        g = clamp255(a + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
        b = clamp255(a + ((116130 * cb + 32768) >> 16));
      } else if (P.conv == MJH_CC_RGB_GRAY) {           // rgb_gray_convert (build_rgb_y_table jdcolor.c:306-327)
        r = g = b = (19595 * a + 38470 * c1 + 7471 * c2 + 32768) >> 16;
      } else { g = c1; b = c2; }
    }
    px[i][0] = (unsigned)r; px[i][1] = (unsigned)g; px[i][2] = (unsigned)b;
  }
  uint8_t *out = pixels + (size_t)img * P.image_stride + (size_t)yo * P.row_pitch + (size_t)x0 * P.px_size;
  if (P.px_size == 1) {
    *reinterpret_cast<unsigned *>(out) = px[0][0] | (px[1][0] << 8) | (px[2][0] << 16) | (px[3][0] << 24);
  } else if (P.px_size == 4) {
    uint4 v;
    unsigned w[4];
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = 0xFFFFFFFFu ^ ((0xFFu ^ px[i][0]) << (8 * P.off_r)) ^ ((0xFFu ^ px[i][1]) << (8 * P.off_g)) ^ ((0xFFu ^ px[i][2]) << (8 * P.off_b));
    v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
    *reinterpret_cast<uint4 *>(out) = v;
  } else {
    // twelve bytes: byte j of pixel i is the colour whose offset is j
    unsigned w[3] = { 0u, 0u, 0u };
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const unsigned p24 = (px[i][0] << (8 * P.off_r)) | (px[i][1] << (8 * P.off_g)) | (px[i][2] << (8 * P.off_b));
      const unsigned long long sh = (unsigned long long)p24 << (8 * (3 * i & 3));     // pixel i starts at byte 3 i: word 3 i / 4, byte 3 i % 4
      w[(3 * i) >> 2] |= (unsigned)sh;
      if (((3 * i) >> 2) + 1 < 3) w[((3 * i) >> 2) + 1] |= (unsigned)(sh >> 32);
    }
    unsigned *o32 = reinterpret_cast<unsigned *>(out);
    o32[0] = w[0]; o32[1] = w[1]; o32[2] = w[2];
  }
}

// ---- K-I2 for JCS_RGB565 (djpeg -rgb565): jdcol565.c / jdmrg565.c, little-endian ------------------------------------------------
// d: byte x & 3 of dither_matrix[y & 3] (jdcolor.c:619), y the row of the (scaled) image -- what a client that reads one row
// per jpeg_read_scanlines call, as djpeg does, gets from the reference (it takes the matrix row from output_scanline at the time
// of the call); a row whose pointer is 4-byte aligned (PACK_NEED_ALIGNMENT = 0).
__constant__ unsigned kDither565[4] = { 0x0008020Au, 0x0C040E06u, 0x030B0109u, 0x0F070D05u };

// The grid, the planes and the MjhPixOut of k_upcolor (px_size 2; the offsets are not read); one lane's 4 pixels are 8 bytes
// and one store.  The dither goes in BEFORE the range limit (range_limit[y + Crrtab[cr] + d], jdcol565.c:136): red and blue
// get d, green d >> 1; a gray file gets d on its one sample, which is then packed three times (gray_rgb565D_convert).
// dither 0 (dither_mode = JDITHER_NONE, djpeg -dither none): d = 0, which is ycc_rgb565_convert / rgb_rgb565_convert /
// gray_rgb565_convert.  The sums stay inside the part of the reference's table that is a plain clamp (-256 .. 639).
__global__ void __launch_bounds__(256)
k_upcolor_565(MjhPixOut P, int dither, const uint8_t *__restrict__ planes, uint8_t *__restrict__ pixels, const unsigned *__restrict__ status)
{
  const int img = blockIdx.z, y = blockIdx.y;
  const int x0 = (int)(blockIdx.x * 256u + threadIdx.x) * 4;
  if (x0 >= P.W) return;
  if (status[img] != 0u) return;
  const uint8_t *pl = planes + (size_t)img * P.planes_per_image;
  const int yo = P.bottom_up ? P.H - 1 - y : y;
  const unsigned dm = dither ? kDither565[y & 3] : 0u;
  unsigned p16[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int x = x0 + i < P.W ? x0 + i : P.W - 1;      // (the pad of the last group, as in k_upcolor)
    const int d = (int)((dm >> (8 * i)) & 0xFFu);       // x0 is a multiple of 4: x & 3 = i
    const int a = up_sample(P.c[0], pl + P.c[0].plane_off, x, y);
    int r, g, b;
    if (P.ncomp == 3) {
      const int c1 = up_sample(P.c[1], pl + P.c[1].plane_off, x, y), c2 = up_sample(P.c[2], pl + P.c[2].plane_off, x, y);
      if (P.conv == MJH_CC_YCC_RGB) {                  // the tables of build_ycc_rgb_table, as k_upcolor
        const int cb = c1 - 128, cr = c2 - 128;
        r = a + ((91881 * cr + 32768) >> 16);
        g = a + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
        b = a + ((116130 * cb + 32768) >> 16);
      } else { r = a; g = c1; b = c2; }                // rgb_rgb565(D)_convert
      r = clamp255(r + d); g = clamp255(g + (d >> 1)); b = clamp255(b + d);
    } else r = g = b = clamp255(a + d);                // gray_rgb565(D)_convert
    p16[i] = (((unsigned)r << 8) & 0xF800u) | (((unsigned)g << 3) & 0x7E0u) | ((unsigned)b >> 3);      // PACK_SHORT_565_LE
  }
  uint2 v;
  v.x = p16[0] | (p16[1] << 16); v.y = p16[2] | (p16[3] << 16);
  *reinterpret_cast<uint2 *>(pixels + (size_t)img * P.image_stride + (size_t)yo * P.row_pitch + (size_t)x0 * 2) = v;
}

// ---- K-I2 for four components (Adobe-style CMYK and YCCK files): pixels of four bytes C, M, Y, K ---------------------------------
// The grid and the lanes of k_upcolor: one lane per 4 output pixels of a row, every sample through up_sample with its component's
// own mode (K may be sampled like Y or lower: jinit_upsampler treats it as any component, and there is no merged upsampling for
// four components), then one 16-byte store.  MJH_CC4_NULL: null_convert, the samples interleaved as they are.  MJH_CC4_YCCK:
// ycck_cmyk_convert (jdcolor.c:543-587): range_limit[255 - (y + table terms)] with the tables of build_ycc_rgb_table as k_upcolor
// has them; the index stays inside the part of the table that is a plain clamp, where range_limit[255 - v] = 255 - clamp(v).
__global__ void __launch_bounds__(256)
k_upcolor4(MjhPixOut4 P, const uint8_t *__restrict__ planes, uint8_t *__restrict__ pixels, const unsigned *__restrict__ status)
{
  const int img = blockIdx.z, y = blockIdx.y;
  const int x0 = (int)(blockIdx.x * 256u + threadIdx.x) * 4;
  if (x0 >= P.W) return;
  if (status[img] != 0u) return;
  const uint8_t *pl = planes + (size_t)img * P.planes_per_image;
  const int yo = P.bottom_up ? P.H - 1 - y : y;
  unsigned w[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int x = x0 + i < P.W ? x0 + i : P.W - 1;      // (the pad of the last group, as in k_upcolor)
    int c0 = up_sample(P.c[0], pl + P.c[0].plane_off, x, y), c1 = up_sample(P.c[1], pl + P.c[1].plane_off, x, y);
    int c2 = up_sample(P.c[2], pl + P.c[2].plane_off, x, y);
    const int c3 = up_sample(P.c[3], pl + P.c[3].plane_off, x, y);
    if (P.conv == MJH_CC4_YCCK) {
      const int a = c0, cb = c1 - 128, cr = c2 - 128;
      c0 = 255 - clamp255(a + ((91881 * cr + 32768) >> 16));
      c1 = 255 - clamp255(a + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
      c2 = 255 - clamp255(a + ((116130 * cb + 32768) >> 16));
    }
    w[i] = (unsigned)c0 | ((unsigned)c1 << 8) | ((unsigned)c2 << 16) | ((unsigned)c3 << 24);
  }
  uint4 v;
  v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
  *reinterpret_cast<uint4 *>(pixels + (size_t)img * P.image_stride + (size_t)yo * P.row_pitch + (size_t)x0 * 4) = v;
}

void mjh_launch_idct(const MjhConst &C, const MjhIdctQ &Q, int comps, const int16_t *coef_q, uint8_t *planes, const unsigned *status, int n, hipStream_t s)
{
  int nblk = 1;
  for (int c = 0; c < comps; c++) if (C.c[c].nblk > nblk) nblk = C.c[c].nblk;
  hipLaunchKernelGGL(k_idct, dim3((nblk + 255) / 256, comps, n), dim3(256), 0, s, C, Q, coef_q, planes, status);
}

void mjh_launch_idct_ifast(const MjhConst &C, const MjhIdctQ &Q, int comps, const int16_t *coef_q, uint8_t *planes, const unsigned *status, int n, hipStream_t s)
{
  int nblk = 1;
  for (int c = 0; c < comps; c++) if (C.c[c].nblk > nblk) nblk = C.c[c].nblk;
  hipLaunchKernelGGL(k_idct_ifast, dim3((nblk + 255) / 256, comps, n), dim3(256), 0, s, C, Q, coef_q, planes, status);
}

void mjh_launch_upcolor(const MjhPixOut &P, const uint8_t *planes, uint8_t *pixels, const unsigned *status, int n, hipStream_t s)
{
  const int groups = (P.W + 3) / 4;
  hipLaunchKernelGGL(k_upcolor, dim3((groups + 255) / 256, P.H, n), dim3(256), 0, s, P, planes, pixels, status);
}

void mjh_launch_upcolor_565(const MjhPixOut &P, int dither, const uint8_t *planes, uint8_t *pixels, const unsigned *status, int n, hipStream_t s)
{
  const int groups = (P.W + 3) / 4;
  hipLaunchKernelGGL(k_upcolor_565, dim3((groups + 255) / 256, P.H, n), dim3(256), 0, s, P, dither, planes, pixels, status);
}

void mjh_launch_upcolor4(const MjhPixOut4 &P, const uint8_t *planes, uint8_t *pixels, const unsigned *status, int n, hipStream_t s)
{
  const int groups = (P.W + 3) / 4;
  hipLaunchKernelGGL(k_upcolor4, dim3((groups + 255) / 256, P.H, n), dim3(256), 0, s, P, planes, pixels, status);
}

void mjh_launch_idct_scaled(const MjhConst &C, const MjhIdctQ &Q, int ci, int N, int pitch, const int16_t *coef_q, uint8_t *planes, const unsigned *status, int n, hipStream_t s)
{
  const MjhComp &cc = C.c[ci];
  const int G = 4 / N;
  const int lanes = (cc.wib + G - 1) / G * cc.hib;
  const dim3 grid((lanes + 255) / 256, 1, n);
  if (N == 4) hipLaunchKernelGGL((k_idct_scaled<4>), grid, dim3(256), 0, s, C, Q, ci, pitch, coef_q, planes, status);
  else if (N == 2) hipLaunchKernelGGL((k_idct_scaled<2>), grid, dim3(256), 0, s, C, Q, ci, pitch, coef_q, planes, status);
  else hipLaunchKernelGGL((k_idct_scaled<1>), grid, dim3(256), 0, s, C, Q, ci, pitch, coef_q, planes, status);
}
