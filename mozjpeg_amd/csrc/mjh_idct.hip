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
// K-I1n k_idct_sized<N>: the twelve other sizes of jidctint.c, N = 3, 5, 6, 7 and 9 to 16 (djpeg -scale N/8 with
//   mjh_decode_opts.all_scales), one component per launch.  N x N samples per block, whose rows need not start at a word: a wave
//   lays 64 blocks' worth of a sample row down in LDS and stores it as whole words; for N > 8 into planes of the call's own,
//   larger than the full-size ones (mjh_scale_layout.h); see the kernel.
// K-I2 k_upcolor: one lane per 4 output pixels of a row.  Per component the upsampler jinit_upsampler picks (jdsample.c:444-525),
//   evaluated per output sample from the samples it reads, then the colour conversion of jdcolor.c / jdcolext.c, then one 4-byte,
//   three 4-byte (12 contiguous bytes) or one 16-byte store (rows of the output hold whole groups of 4 pixels).
//   Edges: neighbours are clamped to [0, downsampled_width) x [0, downsampled_height), which is what the special
//   first / last column cases of the fancy upsamplers (jdsample.c:289-303, :386-404) and the duplicated context rows of the main
//   controller (jdmainct.c make_funny_pointers / set_bottom_pointers) amount to; samples beyond are never read.
// K-I2' k_upcolor_565: the same lanes for JCS_RGB565 (djpeg -rgb565): 4 packed 16-bit pixels, one 8-byte store, with or without
//   the reference's ordered dither; see the kernel.
// K-I2'' k_upcolor4: the same lanes for the four-component files (CMYK, YCCK): 4 pixels of C, M, Y, K, one 16-byte store; see the kernel.
// K-IR k_idct_region, k_idct_region_scaled<N>, k_upcolor_region, k_upcolor_565_region: the same for a region of the image
//   (mjh_decode_opts.crop_*: jpeg_crop_scanline + jpeg_skip_scanlines): only the region's blocks are transformed, into compact
//   planes, and only its pixels are made.  The bodies of K-I1, K-I1f, K-I2 and K-I2' are shared as text (mjh_idct8_body.inc,
//   mjh_idct8_ifast_body.inc, mjh_upcolor_body.inc, mjh_upcolor565_body.inc); see the kernels.
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
#include "mjh_idct8_body.inc"
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
#include "mjh_idct8_ifast_body.inc"
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

// ---- K-IR1: the inverse DCT of a region (mjh_decode_opts.crop_*: jpeg_crop_scanline + jpeg_skip_scanlines) ----------------------
// Only the blocks the region's pixels are made of are dequantized and transformed: of component ci the nbx x nby blocks from
// (bx0, by0) on (MjhRegComp: MCU columns first_MCU_col .. last_MCU_col of jdapistd.c:288-292, and the block rows that hold the
// region's sample rows and the one context row fancy vertical upsampling reads on either side).  They go to a compact plane at
// the component's plane_off whose row 0 is sample row by0 * N of the image and whose column 0 is sample bx0 * N: what the
// reference's coefficient controller leaves in its output buffer under a crop (output_col counts from first_MCU_col).
// One lane per block, region block t = by * nbx + bx: the lanes of a wave hold horizontally adjacent blocks of the REGION, so a
// store instruction writes runs of min(64, nbx) * 8 contiguous bytes -- one 512-byte run for a region 64 blocks wide or more,
// 64 / nbx shorter runs one block row apart for a narrow one -- and plane k of coef_q is read in runs of the same blocks.
// The bodies are k_idct's and k_idct_ifast's, given a component descriptor whose wib / pw are the region plane's.
template <bool FAST>
__global__ void __launch_bounds__(256)
k_idct_region(MjhConst C, MjhIdctQ Q, MjhIdctRegion R, const int16_t *__restrict__ coef_q, uint8_t *__restrict__ planes, const unsigned *__restrict__ status)
{
  const int img = blockIdx.z, ci = blockIdx.y;
  const MjhRegComp &rc = R.c[ci];
  const int b = (int)(blockIdx.x * 256u + threadIdx.x);
  if (b >= rc.nbx * rc.nby) return;
  if (status[img] != 0u) return;
  MjhComp cc = C.c[ci];
  const int ry = b / rc.nbx, rx = b - ry * rc.nbx;
  const int16_t *in = coef_q + (size_t)img * C.coefs_per_image + cc.coef_off + (size_t)(rc.by0 + ry) * cc.wib + (size_t)(rc.bx0 + rx);
  const int *q = Q.q[ci];
  cc.wib = rc.nbx; cc.pw = rc.pitch;                   // the body's b / wib, pw: the region plane's
  if (FAST) {
#include "mjh_idct8_ifast_body.inc"
  } else {
#include "mjh_idct8_body.inc"
  }
}

// The same at DCT_scaled_size N = 1, 2, 4: the lanes of k_idct_scaled (G = 4 / N horizontally adjacent blocks each, N words
// stored) over the region's blocks of component ci; rc.pitch: a multiple of 4 that holds ceil(nbx / G) words.
template <int N>
__global__ void __launch_bounds__(256)
k_idct_region_scaled(MjhConst C, MjhIdctQ Q, int ci, MjhRegComp rc, const int16_t *__restrict__ coef_q, uint8_t *__restrict__ planes, const unsigned *__restrict__ status)
{
  constexpr int G = 4 / N;
  const int img = blockIdx.z;
  const MjhComp &cc = C.c[ci];
  const int gpr = (rc.nbx + G - 1) / G;
  const int t = (int)(blockIdx.x * 256u + threadIdx.x);
  if (t >= gpr * rc.nby) return;
  if (status[img] != 0u) return;
  const int ry = t / gpr, gx = t - ry * gpr;
  const int16_t *in = coef_q + (size_t)img * C.coefs_per_image + cc.coef_off + (size_t)(rc.by0 + ry) * cc.wib + (size_t)rc.bx0;
  unsigned w[N];
#pragma unroll
  for (int r = 0; r < N; r++) w[r] = 0u;
#pragma unroll
  for (int j = 0; j < G; j++) {
    const int rx = gx * G + j;
    if (rx >= rc.nbx) continue;
    idct_block<N>(in + rx, cc.kstride, Q.q[ci], w, j);
  }
  uint8_t *out = planes + (size_t)img * C.planes_per_image + cc.plane_off + (size_t)(ry * N) * rc.pitch + (size_t)gx * 4;
#pragma unroll
  for (int r = 0; r < N; r++) *reinterpret_cast<unsigned *>(out + (size_t)r * rc.pitch) = w[r];
}

// ---- K-I1n: every other size of jidctint.c, N = 3, 5, 6, 7 and 9 to 16 (djpeg -scale N/8, mjh_decode_opts.all_scales) -----------
// FIX() of jidctint.c: a constant at CONST_BITS 13
__host__ __device__ constexpr long long fix13(double x) { return (long long)(x * 8192 + 0.5); }

// The 1-D transforms of jpeg_idct_NxN, chosen by the number of outputs: the sums in front of the descaling shift, WITHOUT the
// rounding term.  The reference adds that term (1 << 10 in pass 1, 1 << 17 in pass 2) to the DC term, which reaches every output
// with the coefficient 1 -- the arithmetic is exact in 64 bits, so the callers add it to the sums instead.  Where the reference's
// pass 1 shifts an even term alone and adds an odd term that was only scaled by 2^PASS1_BITS (6x6, 10x10, 14x14: "tmp11 =
// RIGHT_SHIFT(...)", "tmp1 = LEFT_SHIFT(z1 - z2 - z3, PASS1_BITS)"), the odd term is a multiple of the shift's divisor once
// brought to CONST_BITS, and floor((a + m 2^11) / 2^11) = floor(a / 2^11) + m: the sum shifted is the same number, which is
// how pass 2 of the reference has it.  So both passes of a size are one function here as well.
// x: sizes below 8 read x[0 .. N-1], the others all eight.
__device__ __forceinline__ void idct_1d(const int (&x)[8], long long (&o)[3])     // jpeg_idct_3x3
{
  const long long tmp0 = (long long)x[0] * 8192, tmp12 = x[2] * fix13(0.707106781);
  const long long tmp10 = tmp0 + tmp12, odd = x[1] * fix13(1.224744871);
  o[0] = tmp10 + odd; o[2] = tmp10 - odd;
  o[1] = tmp0 - tmp12 - tmp12;
}
__device__ __forceinline__ void idct_1d(const int (&x)[8], long long (&o)[5])     // jpeg_idct_5x5
{
  long long tmp12 = (long long)x[0] * 8192;
  long long tmp0 = x[2], tmp1 = x[4];
  long long z1 = (tmp0 + tmp1) * fix13(0.790569415), z2 = (tmp0 - tmp1) * fix13(0.353553391), z3 = tmp12 + z2;
  const long long tmp10 = z3 + z1, tmp11 = z3 - z1;
  tmp12 -= z2 * 4;
  z2 = x[1]; z3 = x[3];
  z1 = (z2 + z3) * fix13(0.831253876);
  tmp0 = z1 + z2 * fix13(0.513743148);
  tmp1 = z1 - z3 * fix13(2.176250899);
  o[0] = tmp10 + tmp0; o[4] = tmp10 - tmp0;
  o[1] = tmp11 + tmp1; o[3] = tmp11 - tmp1;
  o[2] = tmp12;
}
__device__ __forceinline__ void idct_1d(const int (&x)[8], long long (&o)[6])     // jpeg_idct_6x6
{
  long long tmp0 = (long long)x[0] * 8192;
  long long tmp10 = x[4] * fix13(0.707106781);
  long long tmp1 = tmp0 + tmp10;
  const long long tmp11 = tmp0 - tmp10 - tmp10;
  tmp0 = x[2] * fix13(1.224744871);
  tmp10 = tmp1 + tmp0;
  const long long tmp12 = tmp1 - tmp0;
  const long long z1 = x[1], z2 = x[3], z3 = x[5];
  tmp1 = (z1 + z3) * fix13(0.366025404);
  tmp0 = tmp1 + (z1 + z2) * 8192;
  const long long tmp2 = tmp1 + (z3 - z2) * 8192;
  tmp1 = (z1 - z2 - z3) * 8192;
  o[0] = tmp10 + tmp0; o[5] = tmp10 - tmp0;
  o[1] = tmp11 + tmp1; o[4] = tmp11 - tmp1;
  o[2] = tmp12 + tmp2; o[3] = tmp12 - tmp2;
}
__device__ __forceinline__ void idct_1d(const int (&x)[8], long long (&o)[7])     // jpeg_idct_7x7
{
  long long tmp13 = (long long)x[0] * 8192;
  long long z1 = x[2], z2 = x[4], z3 = x[6];
  long long tmp10 = (z2 - z3) * fix13(0.881747734), tmp12 = (z1 - z2) * fix13(0.314692123);
  const long long tmp11 = tmp10 + tmp12 + tmp13 - z2 * fix13(1.841218003);
  long long tmp0 = z1 + z3;
  z2 -= tmp0;
  tmp0 = tmp0 * fix13(1.274162392) + tmp13;
  tmp10 += tmp0 - z3 * fix13(0.077722536);
  tmp12 += tmp0 - z1 * fix13(2.470602249);
  tmp13 += z2 * fix13(1.414213562);
  z1 = x[1]; z2 = x[3]; z3 = x[5];
  long long tmp1 = (z1 + z2) * fix13(0.935414347), tmp2 = (z1 - z2) * fix13(0.170262339);
  tmp0 = tmp1 - tmp2;
  tmp1 += tmp2;
  tmp2 = (z2 + z3) * -fix13(1.378756276);
  tmp1 += tmp2;
  z2 = (z1 + z3) * fix13(0.613604268);
  tmp0 += z2;
  tmp2 += z2 + z3 * fix13(1.870828693);
  o[0] = tmp10 + tmp0; o[6] = tmp10 - tmp0;
  o[1] = tmp11 + tmp1; o[5] = tmp11 - tmp1;
  o[2] = tmp12 + tmp2; o[4] = tmp12 - tmp2;
  o[3] = tmp13;
}
__device__ __forceinline__ void idct_1d(const int (&x)[8], long long (&o)[9])     // jpeg_idct_9x9
{
  long long tmp0 = (long long)x[0] * 8192;
  long long z1 = x[2], z2 = x[4], z3 = x[6], z4;
  long long tmp3 = z3 * fix13(0.707106781);
  long long tmp1 = tmp0 + tmp3, tmp2 = tmp0 - tmp3 - tmp3;
  tmp0 = (z1 - z2) * fix13(0.707106781);
  const long long tmp11 = tmp2 + tmp0, tmp14 = tmp2 - tmp0 - tmp0;
  tmp0 = (z1 + z2) * fix13(1.328926049);
  tmp2 = z1 * fix13(1.083350441);
  tmp3 = z2 * fix13(0.245575608);
  const long long tmp10 = tmp1 + tmp0 - tmp3, tmp12 = tmp1 - tmp0 + tmp2, tmp13 = tmp1 - tmp2 + tmp3;
  z1 = x[1]; z2 = x[3]; z3 = x[5]; z4 = x[7];
  z2 = z2 * -fix13(1.224744871);
  tmp2 = (z1 + z3) * fix13(0.909038955);
  tmp3 = (z1 + z4) * fix13(0.483689525);
  tmp0 = tmp2 + tmp3 - z2;
  tmp1 = (z3 - z4) * fix13(1.392728481);
  tmp2 += z2 - tmp1;
  tmp3 += z2 + tmp1;
  tmp1 = (z1 - z3 - z4) * fix13(1.224744871);
  o[0] = tmp10 + tmp0; o[8] = tmp10 - tmp0;
  o[1] = tmp11 + tmp1; o[7] = tmp11 - tmp1;
  o[2] = tmp12 + tmp2; o[6] = tmp12 - tmp2;
  o[3] = tmp13 + tmp3; o[5] = tmp13 - tmp3;
  o[4] = tmp14;
}
__device__ __forceinline__ void idct_1d(const int (&x)[8], long long (&o)[10])    // jpeg_idct_10x10
{
  long long z3 = (long long)x[0] * 8192, z4 = x[4];
  long long z1 = z4 * fix13(1.144122806), z2 = z4 * fix13(0.437016024);
  long long tmp10 = z3 + z1, tmp11 = z3 - z2;
  const long long tmp22 = z3 - (z1 - z2) * 2;
  z2 = x[2]; z3 = x[6];
  z1 = (z2 + z3) * fix13(0.831253876);
  long long tmp12 = z1 + z2 * fix13(0.513743148), tmp13 = z1 - z3 * fix13(2.176250899);
  const long long tmp20 = tmp10 + tmp12, tmp24 = tmp10 - tmp12, tmp21 = tmp11 + tmp13, tmp23 = tmp11 - tmp13;
  z1 = x[1]; z2 = x[3]; z3 = x[5]; z4 = x[7];
  tmp11 = z2 + z4;
  tmp13 = z2 - z4;
  tmp12 = tmp13 * fix13(0.309016994);
  const long long z5 = z3 * 8192;
  z2 = tmp11 * fix13(0.951056516);
  z4 = z5 + tmp12;
  tmp10 = z1 * fix13(1.396802247) + z2 + z4;
  const long long tmp14 = z1 * fix13(0.221231742) - z2 + z4;
  z2 = tmp11 * fix13(0.587785252);
  z4 = z5 - tmp12 - tmp13 * 4096;
  tmp12 = (z1 - tmp13 - z3) * 8192;
  tmp11 = z1 * fix13(1.260073511) - z2 - z4;
  tmp13 = z1 * fix13(0.642039522) - z2 + z4;
  o[0] = tmp20 + tmp10; o[9] = tmp20 - tmp10;
  o[1] = tmp21 + tmp11; o[8] = tmp21 - tmp11;
  o[2] = tmp22 + tmp12; o[7] = tmp22 - tmp12;
  o[3] = tmp23 + tmp13; o[6] = tmp23 - tmp13;
  o[4] = tmp24 + tmp14; o[5] = tmp24 - tmp14;
}
__device__ __forceinline__ void idct_1d(const int (&x)[8], long long (&o)[11])    // jpeg_idct_11x11
{
  long long tmp10 = (long long)x[0] * 8192;
  long long z1 = x[2], z2 = x[4], z3 = x[6];
  long long tmp20 = (z2 - z3) * fix13(2.546640132), tmp23 = (z2 - z1) * fix13(0.430815045);
  long long z4 = z1 + z3;
  long long tmp24 = z4 * -fix13(1.155664402);
  z4 -= z2;
  long long tmp25 = tmp10 + z4 * fix13(1.356927976);
  const long long tmp21 = tmp20 + tmp23 + tmp25 - z2 * fix13(1.821790775);
  tmp20 += tmp25 + z3 * fix13(2.115825087);
  tmp23 += tmp25 - z1 * fix13(1.513598477);
  tmp24 += tmp25;
  const long long tmp22 = tmp24 - z3 * fix13(0.788749120);
  tmp24 += z2 * fix13(1.944413522) - z1 * fix13(1.390975730);
  tmp25 = tmp10 - z4 * fix13(1.414213562);
  z1 = x[1]; z2 = x[3]; z3 = x[5]; z4 = x[7];
  long long tmp11 = z1 + z2;
  long long tmp14 = (tmp11 + z3 + z4) * fix13(0.398430003);
  tmp11 = tmp11 * fix13(0.887983902);
  long long tmp12 = (z1 + z3) * fix13(0.670361295);
  long long tmp13 = tmp14 + (z1 + z4) * fix13(0.366151574);
  tmp10 = tmp11 + tmp12 + tmp13 - z1 * fix13(0.923107866);
  z1 = tmp14 - (z2 + z3) * fix13(1.163011579);
  tmp11 += z1 + z2 * fix13(2.073276588);
  tmp12 += z1 - z3 * fix13(1.192193623);
  z1 = (z2 + z4) * -fix13(1.798248910);
  tmp11 += z1;
  tmp13 += z1 + z4 * fix13(2.102458632);
  tmp14 += z2 * -fix13(1.467221301) + z3 * fix13(1.001388905) - z4 * fix13(1.684843907);
  o[0] = tmp20 + tmp10; o[10] = tmp20 - tmp10;
  o[1] = tmp21 + tmp11; o[9] = tmp21 - tmp11;
  o[2] = tmp22 + tmp12; o[8] = tmp22 - tmp12;
  o[3] = tmp23 + tmp13; o[7] = tmp23 - tmp13;
  o[4] = tmp24 + tmp14; o[6] = tmp24 - tmp14;
  o[5] = tmp25;
}
__device__ __forceinline__ void idct_1d(const int (&x)[8], long long (&o)[12])    // jpeg_idct_12x12
{
  long long z3 = (long long)x[0] * 8192;
  long long z4 = x[4] * fix13(1.224744871);
  long long tmp10 = z3 + z4, tmp11 = z3 - z4;
  long long z1 = x[2];
  z4 = z1 * fix13(1.366025404);
  z1 = z1 * 8192;
  long long z2 = (long long)x[6] * 8192;
  long long tmp12 = z1 - z2;
  const long long tmp21 = z3 + tmp12, tmp24 = z3 - tmp12;
  tmp12 = z4 + z2;
  const long long tmp20 = tmp10 + tmp12, tmp25 = tmp10 - tmp12;
  tmp12 = z4 - z1 - z2;
  const long long tmp22 = tmp11 + tmp12, tmp23 = tmp11 - tmp12;
  z1 = x[1]; z2 = x[3]; z3 = x[5]; z4 = x[7];
  tmp11 = z2 * fix13(1.306562965);
  long long tmp14 = z2 * -fix13(0.541196100);
  tmp10 = z1 + z3;
  long long tmp15 = (tmp10 + z4) * fix13(0.860918669);
  tmp12 = tmp15 + tmp10 * fix13(0.261052384);
  tmp10 = tmp12 + tmp11 + z1 * fix13(0.280143716);
  long long tmp13 = (z3 + z4) * -fix13(1.045510580);
  tmp12 += tmp13 + tmp14 - z3 * fix13(1.478575242);
  tmp13 += tmp15 - tmp11 + z4 * fix13(1.586706681);
  tmp15 += tmp14 - z1 * fix13(0.676326758) - z4 * fix13(1.982889723);
  z1 -= z4;
  z2 -= z3;
  z3 = (z1 + z2) * fix13(0.541196100);
  tmp11 = z3 + z1 * fix13(0.765366865);
  tmp14 = z3 - z2 * fix13(1.847759065);
  o[0] = tmp20 + tmp10; o[11] = tmp20 - tmp10;
  o[1] = tmp21 + tmp11; o[10] = tmp21 - tmp11;
  o[2] = tmp22 + tmp12; o[9] = tmp22 - tmp12;
  o[3] = tmp23 + tmp13; o[8] = tmp23 - tmp13;
  o[4] = tmp24 + tmp14; o[7] = tmp24 - tmp14;
  o[5] = tmp25 + tmp15; o[6] = tmp25 - tmp15;
}
__device__ __forceinline__ void idct_1d(const int (&x)[8], long long (&o)[13])    // jpeg_idct_13x13
{
  long long z1 = (long long)x[0] * 8192;
  long long z2 = x[2], z3 = x[4], z4 = x[6];
  long long tmp10 = z3 + z4, tmp11 = z3 - z4;
  long long tmp12 = tmp10 * fix13(1.155388986), tmp13 = tmp11 * fix13(0.096834934) + z1;
  const long long tmp20 = z2 * fix13(1.373119086) + tmp12 + tmp13, tmp22 = z2 * fix13(0.501487041) - tmp12 + tmp13;
  tmp12 = tmp10 * fix13(0.316450131);
  tmp13 = tmp11 * fix13(0.486914739) + z1;
  const long long tmp21 = z2 * fix13(1.058554052) - tmp12 + tmp13, tmp25 = z2 * -fix13(1.252223920) + tmp12 + tmp13;
  tmp12 = tmp10 * fix13(0.435816023);
  tmp13 = tmp11 * fix13(0.937303064) - z1;
  const long long tmp23 = z2 * -fix13(0.170464608) - tmp12 - tmp13, tmp24 = z2 * -fix13(0.803364869) + tmp12 - tmp13;
  const long long tmp26 = (tmp11 - z2) * fix13(1.414213562) + z1;
  z1 = x[1]; z2 = x[3]; z3 = x[5]; z4 = x[7];
  tmp11 = (z1 + z2) * fix13(1.322312651);
  tmp12 = (z1 + z3) * fix13(1.163874945);
  long long tmp15 = z1 + z4;
  tmp13 = tmp15 * fix13(0.937797057);
  tmp10 = tmp11 + tmp12 + tmp13 - z1 * fix13(2.020082300);
  long long tmp14 = (z2 + z3) * -fix13(0.338443458);
  tmp11 += tmp14 + z2 * fix13(0.837223564);
  tmp12 += tmp14 - z3 * fix13(1.572116027);
  tmp14 = (z2 + z4) * -fix13(1.163874945);
  tmp11 += tmp14;
  tmp13 += tmp14 + z4 * fix13(2.205608352);
  tmp14 = (z3 + z4) * -fix13(0.657217813);
  tmp12 += tmp14;
  tmp13 += tmp14;
  tmp15 = tmp15 * fix13(0.338443458);
  tmp14 = tmp15 + z1 * fix13(0.318774355) - z2 * fix13(0.466105296);
  z1 = (z3 - z2) * fix13(0.937797057);
  tmp14 += z1;
  tmp15 += z1 + z3 * fix13(0.384515595) - z4 * fix13(1.742345811);
  o[0] = tmp20 + tmp10; o[12] = tmp20 - tmp10;
  o[1] = tmp21 + tmp11; o[11] = tmp21 - tmp11;
  o[2] = tmp22 + tmp12; o[10] = tmp22 - tmp12;
  o[3] = tmp23 + tmp13; o[9] = tmp23 - tmp13;
  o[4] = tmp24 + tmp14; o[8] = tmp24 - tmp14;
  o[5] = tmp25 + tmp15; o[7] = tmp25 - tmp15;
  o[6] = tmp26;
}
__device__ __forceinline__ void idct_1d(const int (&x)[8], long long (&o)[14])    // jpeg_idct_14x14
{
  long long z1 = (long long)x[0] * 8192, z4 = x[4];
  long long z2 = z4 * fix13(1.274162392), z3 = z4 * fix13(0.314692123);
  z4 = z4 * fix13(0.881747734);
  long long tmp10 = z1 + z2, tmp11 = z1 + z3, tmp12 = z1 - z4;
  const long long tmp23 = z1 - (z2 + z3 - z4) * 2;
  z1 = x[2]; z2 = x[6];
  z3 = (z1 + z2) * fix13(1.105676686);
  long long tmp13 = z3 + z1 * fix13(0.273079590), tmp14 = z3 - z2 * fix13(1.719280954);
  long long tmp15 = z1 * fix13(0.613604268) - z2 * fix13(1.378756276);
  const long long tmp20 = tmp10 + tmp13, tmp26 = tmp10 - tmp13, tmp21 = tmp11 + tmp14, tmp25 = tmp11 - tmp14;
  const long long tmp22 = tmp12 + tmp15, tmp24 = tmp12 - tmp15;
  z1 = x[1]; z2 = x[3]; z3 = x[5]; z4 = x[7];
  tmp13 = z4 * 8192;
  tmp14 = z1 + z3;
  tmp11 = (z1 + z2) * fix13(1.334852607);
  tmp12 = tmp14 * fix13(1.197448846);
  tmp10 = tmp11 + tmp12 + tmp13 - z1 * fix13(1.126980169);
  tmp14 = tmp14 * fix13(0.752406978);
  long long tmp16 = tmp14 - z1 * fix13(1.061150426);
  z1 -= z2;
  tmp15 = z1 * fix13(0.467085129) - tmp13;
  tmp16 += tmp15;
  z1 += z4;
  z4 = (z2 + z3) * -fix13(0.158341681) - tmp13;
  tmp11 += z4 - z2 * fix13(0.424103948);
  tmp12 += z4 - z3 * fix13(2.373959773);
  z4 = (z3 - z2) * fix13(1.405321284);
  tmp14 += z4 + tmp13 - z3 * fix13(1.6906431334);
  tmp15 += z4 + z2 * fix13(0.674957567);
  tmp13 = (z1 - z3) * 8192;
  o[0] = tmp20 + tmp10; o[13] = tmp20 - tmp10;
  o[1] = tmp21 + tmp11; o[12] = tmp21 - tmp11;
  o[2] = tmp22 + tmp12; o[11] = tmp22 - tmp12;
  o[3] = tmp23 + tmp13; o[10] = tmp23 - tmp13;
  o[4] = tmp24 + tmp14; o[9] = tmp24 - tmp14;
  o[5] = tmp25 + tmp15; o[8] = tmp25 - tmp15;
  o[6] = tmp26 + tmp16; o[7] = tmp26 - tmp16;
}
__device__ __forceinline__ void idct_1d(const int (&x)[8], long long (&o)[15])    // jpeg_idct_15x15
{
  long long z1 = (long long)x[0] * 8192;
  long long z2 = x[2], z3 = x[4], z4 = x[6];
  long long tmp10 = z4 * fix13(0.437016024), tmp11 = z4 * fix13(1.144122806);
  const long long tmp12 = z1 - tmp10, tmp13 = z1 + tmp11;
  z1 -= (tmp11 - tmp10) * 2;
  z4 = z2 - z3;
  z3 += z2;
  tmp10 = z3 * fix13(1.337628990);
  tmp11 = z4 * fix13(0.045680613);
  z2 = z2 * fix13(1.439773946);
  const long long tmp20 = tmp13 + tmp10 + tmp11, tmp23 = tmp12 - tmp10 + tmp11 + z2;
  tmp10 = z3 * fix13(0.547059574);
  tmp11 = z4 * fix13(0.399234004);
  const long long tmp25 = tmp13 - tmp10 - tmp11, tmp26 = tmp12 + tmp10 - tmp11 - z2;
  tmp10 = z3 * fix13(0.790569415);
  tmp11 = z4 * fix13(0.353553391);
  const long long tmp21 = tmp12 + tmp10 + tmp11, tmp24 = tmp13 - tmp10 + tmp11;
  tmp11 += tmp11;
  const long long tmp22 = z1 + tmp11, tmp27 = z1 - tmp11 - tmp11;
  z1 = x[1]; z2 = x[3]; z4 = x[5];
  z3 = z4 * fix13(1.224744871);
  z4 = x[7];
  long long t13 = z2 - z4;
  long long tmp15 = (z1 + t13) * fix13(0.831253876);
  tmp11 = tmp15 + z1 * fix13(0.513743148);
  const long long tmp14 = tmp15 - t13 * fix13(2.176250899);
  t13 = z2 * -fix13(0.831253876);
  tmp15 = z2 * -fix13(1.344997024);
  z2 = z1 - z4;
  long long t12 = z3 + z2 * fix13(1.406466353);
  tmp10 = t12 + z4 * fix13(2.457431844) - tmp15;
  const long long tmp16 = t12 - z1 * fix13(1.112434820) + t13;
  t12 = z2 * fix13(1.224744871) - z3;
  z2 = (z1 + z4) * fix13(0.575212477);
  t13 += z2 + z1 * fix13(0.475753014) - z3;
  tmp15 += z2 - z4 * fix13(0.869244010) + z3;
  o[0] = tmp20 + tmp10; o[14] = tmp20 - tmp10;
  o[1] = tmp21 + tmp11; o[13] = tmp21 - tmp11;
  o[2] = tmp22 + t12; o[12] = tmp22 - t12;
  o[3] = tmp23 + t13; o[11] = tmp23 - t13;
  o[4] = tmp24 + tmp14; o[10] = tmp24 - tmp14;
  o[5] = tmp25 + tmp15; o[9] = tmp25 - tmp15;
  o[6] = tmp26 + tmp16; o[8] = tmp26 - tmp16;
  o[7] = tmp27;
}
__device__ __forceinline__ void idct_1d(const int (&x)[8], long long (&o)[16])    // jpeg_idct_16x16
{
  long long tmp0 = (long long)x[0] * 8192;
  long long z1 = x[4];
  long long tmp1 = z1 * fix13(1.306562965), tmp2 = z1 * fix13(0.541196100);
  long long tmp10 = tmp0 + tmp1, tmp11 = tmp0 - tmp1, tmp12 = tmp0 + tmp2, tmp13 = tmp0 - tmp2;
  z1 = x[2];
  long long z2 = x[6];
  long long z3 = z1 - z2;
  long long z4 = z3 * fix13(0.275899379);
  z3 = z3 * fix13(1.387039845);
  tmp0 = z3 + z2 * fix13(2.562915447);
  tmp1 = z4 + z1 * fix13(0.899976223);
  tmp2 = z3 - z1 * fix13(0.601344887);
  long long tmp3 = z4 - z2 * fix13(0.509795579);
  const long long tmp20 = tmp10 + tmp0, tmp27 = tmp10 - tmp0, tmp21 = tmp12 + tmp1, tmp26 = tmp12 - tmp1;
  const long long tmp22 = tmp13 + tmp2, tmp25 = tmp13 - tmp2, tmp23 = tmp11 + tmp3, tmp24 = tmp11 - tmp3;
  z1 = x[1]; z2 = x[3]; z3 = x[5]; z4 = x[7];
  tmp11 = z1 + z3;
  tmp1 = (z1 + z2) * fix13(1.353318001);
  tmp2 = tmp11 * fix13(1.247225013);
  tmp3 = (z1 + z4) * fix13(1.093201867);
  tmp10 = (z1 - z4) * fix13(0.897167586);
  tmp11 = tmp11 * fix13(0.666655658);
  tmp12 = (z1 - z2) * fix13(0.410524528);
  tmp0 = tmp1 + tmp2 + tmp3 - z1 * fix13(2.286341144);
  tmp13 = tmp10 + tmp11 + tmp12 - z1 * fix13(1.835730603);
  z1 = (z2 + z3) * fix13(0.138617169);
  tmp1 += z1 + z2 * fix13(0.071888074);
  tmp2 += z1 - z3 * fix13(1.125726048);
  z1 = (z3 - z2) * fix13(1.407403738);
  tmp11 += z1 - z3 * fix13(0.766367282);
  tmp12 += z1 + z2 * fix13(1.971951411);
  z2 += z4;
  z1 = z2 * -fix13(0.666655658);
  tmp1 += z1;
  tmp3 += z1 + z4 * fix13(1.065388962);
  z2 = z2 * -fix13(1.247225013);
  tmp10 += z2 + z4 * fix13(3.141271809);
  tmp12 += z2;
  z2 = (z3 + z4) * -fix13(1.353318001);
  tmp2 += z2;
  tmp3 += z2;
  z2 = (z4 - z3) * fix13(0.410524528);
  tmp10 += z2;
  tmp11 += z2;
  o[0] = tmp20 + tmp0; o[15] = tmp20 - tmp0;
  o[1] = tmp21 + tmp1; o[14] = tmp21 - tmp1;
  o[2] = tmp22 + tmp2; o[13] = tmp22 - tmp2;
  o[3] = tmp23 + tmp3; o[12] = tmp23 - tmp3;
  o[4] = tmp24 + tmp10; o[11] = tmp24 - tmp10;
  o[5] = tmp25 + tmp11; o[10] = tmp25 - tmp11;
  o[6] = tmp26 + tmp12; o[9] = tmp26 - tmp12;
  o[7] = tmp27 + tmp13; o[8] = tmp27 - tmp13;
}

// One lane per block of component ci; a wave holds 64 horizontally adjacent blocks of one block row ("chunk"), whose first
// sample byte, 64 * cx * N, is word-aligned for every N.  A block's row is N bytes at byte lane * N of the chunk's row -- not a
// word boundary for odd N -- so the wave lays the 64 x N bytes of one sample row down in LDS and its lanes carry them out as
// whole words: every store instruction writes one contiguous run of a sample row, and no byte store goes to memory.  Two LDS
// rows take turns, so one barrier per sample row is enough (a row is read before the barrier of the next, and written again
// only behind it).
// plane_off, planes_per_image: the layout of the call's sample planes -- the encoder's own where every component fits its
// full-size plane, a layout of the call's where a component is larger (N > 8); pitch: samples between rows, (wib * N + 3) & ~3.
// The lanes a last chunk has beyond wib read nothing and lay down zeros, of which at most three reach the pitch pad.
template <int N>
__global__ void __launch_bounds__(256)
k_idct_sized(MjhConst C, MjhIdctQ Q, int ci, int pitch, long long plane_off, long long planes_per_image,
             const int16_t *__restrict__ coef_q, uint8_t *__restrict__ planes, const unsigned *__restrict__ status)
{
  constexpr int NI = N < 8 ? N : 8;                    // the coefficients a 1-D transform reads (the workspace is NI wide)
  __shared__ unsigned seg[2][4][16 * N];
  const int img = blockIdx.z;
  if (status[img] != 0u) return;                       // (the same for every lane of the workgroup)
  const MjhComp &cc = C.c[ci];
  const int cpr = (cc.wib + 63) >> 6;                  // chunks per block row
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
  const int chunk = (int)blockIdx.x * 4 + wave;
  const int by = chunk / cpr, cx = chunk - by * cpr;
  const int bx = cx * 64 + lane;
  const bool row_live = by < cc.hib, live = row_live && bx < cc.wib;
  int ws[N][8];
  if (live) {
    const int16_t *in = coef_q + (size_t)img * C.coefs_per_image + cc.coef_off + (size_t)by * cc.wib + bx;
    const int *q = Q.q[ci];
    // pass 1: NI columns to N values each, scaled up by 2^PASS1_BITS
#pragma unroll
    for (int c = 0; c < NI; c++) {
      int x[8];
#pragma unroll
      for (int r = 0; r < 8; r++) x[r] = r < NI ? (int)in[(size_t)kZigOfNat[r * 8 + c] * cc.kstride] * q[r * 8 + c] : 0;
      long long o[N];
      idct_1d(x, o);
#pragma unroll
      for (int r = 0; r < N; r++) ws[r][c] = (int)((o[r] + 1024) >> 11);
    }
#pragma unroll
    for (int r = 0; r < N; r++)
#pragma unroll
      for (int c = NI; c < 8; c++) ws[r][c] = 0;
  }
  // the words of the chunk's sample row that hold samples of real blocks
  const int nb = cc.wib - cx * 64 < 64 ? cc.wib - cx * 64 : 64;
  const int nw = row_live ? (nb * N + 3) >> 2 : 0;
  unsigned *out = reinterpret_cast<unsigned *>(planes + (size_t)img * (size_t)planes_per_image + (size_t)plane_off + (size_t)(by * N) * pitch + (size_t)cx * 64 * N);
  // pass 2: N rows; descale by 2^(CONST_BITS + PASS1_BITS + 3), then the range limit with the sample's centre added
#pragma unroll
  for (int r = 0; r < N; r++) {
    unsigned s[N];
#pragma unroll
    for (int c = 0; c < N; c++) s[c] = 0u;
    if (live) {
      long long o[N];
      idct_1d(ws[r], o);
#pragma unroll
      for (int c = 0; c < N; c++) s[c] = idct_range_limit((int)((o[c] + (1 << 17)) >> 18));
    }
    unsigned *row = seg[r & 1][wave];
    if (N % 4 == 0) {
#pragma unroll
      for (int j = 0; j < N / 4; j++) row[lane * (N / 4) + j] = s[4 * j] | (s[4 * j + 1] << 8) | (s[4 * j + 2] << 16) | (s[4 * j + 3] << 24);
    } else if (N % 2 == 0) {
      unsigned short *row16 = reinterpret_cast<unsigned short *>(row) + lane * (N / 2);
#pragma unroll
      for (int j = 0; j < N / 2; j++) row16[j] = (unsigned short)(s[2 * j] | (s[2 * j + 1] << 8));
    } else {
      unsigned char *row8 = reinterpret_cast<unsigned char *>(row) + lane * N;
#pragma unroll
      for (int j = 0; j < N; j++) row8[j] = (unsigned char)s[j];
    }
    __syncthreads();
    for (int i = lane; i < nw; i += 64) out[((size_t)r * pitch >> 2) + i] = row[i];
  }
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
#include "mjh_upcolor_body.inc"
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
#include "mjh_upcolor565_body.inc"
}

// ---- K-IR2: upsampling and colour conversion of a region ---------------------------------------------------------------------------
// The lanes, the conversions and the stores of k_upcolor / k_upcolor_565 over the region image P.W x P.H (the aligned width, the
// rows asked for); row y of the region is row y0 + y of the whole image.
// Across, everything is the region's: P.c[].dw is the cropped downsampled_width (jdapistd.c:276-281) and column 0 of a region
// plane is the region's first sample, so the clamps of up_sample give the crop edges the image-edge formulas, as the reference's
// fancy upsamplers do when they are handed the cropped rows, and the 565 dither counts columns from the region's left edge.
// Down, everything is the whole image's: P.c[].dh is the image's downsampled_height and up_sample is asked for image row
// y0 + y, so only rows at the image's top or bottom get the edge formula, every other row its real neighbours (which K-IR1
// transformed: MjhRegComp.by0 / nby), and the dither row is the image's.  P.c[].plane_off points by0 * N rows ABOVE the region
// plane (the host subtracts them), so image row r of a component is at plane_off + r * pw although the plane starts at row
// by0 * N; rows outside [by0 * N, (by0 + nby) * N) are never asked for.
__global__ void __launch_bounds__(256)
k_upcolor_region(MjhPixOut P, int y0, const uint8_t *__restrict__ planes, uint8_t *__restrict__ pixels, const unsigned *__restrict__ status)
{
  const int img = blockIdx.z, ry = blockIdx.y, y = y0 + ry;
  const int x0 = (int)(blockIdx.x * 256u + threadIdx.x) * 4;
  if (x0 >= P.W) return;
  if (status[img] != 0u) return;
  const uint8_t *pl = planes + (size_t)img * P.planes_per_image;
  const int yo = P.bottom_up ? P.H - 1 - ry : ry;        // the flip is inside the region
#include "mjh_upcolor_body.inc"
}

__global__ void __launch_bounds__(256)
k_upcolor_565_region(MjhPixOut P, int y0, int dither, const uint8_t *__restrict__ planes, uint8_t *__restrict__ pixels, const unsigned *__restrict__ status)
{
  const int img = blockIdx.z, ry = blockIdx.y, y = y0 + ry;
  const int x0 = (int)(blockIdx.x * 256u + threadIdx.x) * 4;
  if (x0 >= P.W) return;
  if (status[img] != 0u) return;
  const uint8_t *pl = planes + (size_t)img * P.planes_per_image;
  const int yo = P.bottom_up ? P.H - 1 - ry : ry;
#include "mjh_upcolor565_body.inc"
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

void mjh_launch_idct_sized(const MjhConst &C, const MjhIdctQ &Q, int ci, int N, int pitch, long long plane_off, long long planes_per_image,
                           const int16_t *coef_q, uint8_t *planes, const unsigned *status, int n, hipStream_t s)
{
  const MjhComp &cc = C.c[ci];
  const int chunks = (cc.wib + 63) / 64 * cc.hib;
  const dim3 grid((chunks + 3) / 4, 1, n);
#define MJH_SIZED(K) case K: hipLaunchKernelGGL((k_idct_sized<K>), grid, dim3(256), 0, s, C, Q, ci, pitch, plane_off, planes_per_image, coef_q, planes, status); break
  switch (N) {
    MJH_SIZED(3); MJH_SIZED(5); MJH_SIZED(6); MJH_SIZED(7); MJH_SIZED(9); MJH_SIZED(10); MJH_SIZED(11);
    MJH_SIZED(12); MJH_SIZED(13); MJH_SIZED(14); MJH_SIZED(15); MJH_SIZED(16);
  }
#undef MJH_SIZED
}

void mjh_launch_idct_region(const MjhConst &C, const MjhIdctQ &Q, const MjhIdctRegion &R, int comps, bool ifast, const int16_t *coef_q, uint8_t *planes, const unsigned *status, int n, hipStream_t s)
{
  int nblk = 1;
  for (int c = 0; c < comps; c++) if (R.c[c].nbx * R.c[c].nby > nblk) nblk = R.c[c].nbx * R.c[c].nby;
  const dim3 grid((nblk + 255) / 256, comps, n);
  if (ifast) hipLaunchKernelGGL((k_idct_region<true>), grid, dim3(256), 0, s, C, Q, R, coef_q, planes, status);
  else hipLaunchKernelGGL((k_idct_region<false>), grid, dim3(256), 0, s, C, Q, R, coef_q, planes, status);
}

void mjh_launch_idct_region_scaled(const MjhConst &C, const MjhIdctQ &Q, int ci, int N, const MjhRegComp &rc, const int16_t *coef_q, uint8_t *planes, const unsigned *status, int n, hipStream_t s)
{
  const int G = 4 / N;
  const int lanes = (rc.nbx + G - 1) / G * rc.nby;
  const dim3 grid((lanes + 255) / 256, 1, n);
  if (N == 4) hipLaunchKernelGGL((k_idct_region_scaled<4>), grid, dim3(256), 0, s, C, Q, ci, rc, coef_q, planes, status);
  else if (N == 2) hipLaunchKernelGGL((k_idct_region_scaled<2>), grid, dim3(256), 0, s, C, Q, ci, rc, coef_q, planes, status);
  else hipLaunchKernelGGL((k_idct_region_scaled<1>), grid, dim3(256), 0, s, C, Q, ci, rc, coef_q, planes, status);
}

void mjh_launch_upcolor_region(const MjhPixOut &P, int y0, const uint8_t *planes, uint8_t *pixels, const unsigned *status, int n, hipStream_t s)
{
  const int groups = (P.W + 3) / 4;
  hipLaunchKernelGGL(k_upcolor_region, dim3((groups + 255) / 256, P.H, n), dim3(256), 0, s, P, y0, planes, pixels, status);
}

void mjh_launch_upcolor_565_region(const MjhPixOut &P, int y0, int dither, const uint8_t *planes, uint8_t *pixels, const unsigned *status, int n, hipStream_t s)
{
  const int groups = (P.W + 3) / 4;
  hipLaunchKernelGGL(k_upcolor_565_region, dim3((groups + 255) / 256, P.H, n), dim3(256), 0, s, P, y0, dither, planes, pixels, status);
}
