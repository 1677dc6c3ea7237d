// mjh_idct.h -- descriptors shared by the host side of mjh_decode_host (mjh_encoder.cpp) and the pixel kernels (mjh_idct.hip)
#ifndef MJH_IDCT_H
#define MJH_IDCT_H
#include <hip/hip_runtime.h>
#include "mjh_internal.h"

// the multipliers of the inverse transform: quantval of every component's table, natural order, as 32-bit words (the reference
// built without SIMD keeps them as int: MULTIPLIER, jmorecfg.h:367-372; wave-uniform reads become scalar loads)
// For k_idct_ifast the same struct holds the AA&N multipliers of jddctmgr.c:284-316 instead (mjh_decode_host makes both).
struct MjhIdctQ { int q[MJH_MAXC][64]; };

// how one component reaches full size (jinit_upsampler jdsample.c:444-525)
#define MJH_UP_REPLICATE 0       // fullsize_upsample, h2v1_upsample, h2v2_upsample, int_upsample: sample (x / hexp, y / vexp)
#define MJH_UP_H2V1_FANCY 1
#define MJH_UP_H1V2_FANCY 2
#define MJH_UP_H2V2_FANCY 3
struct MjhUpComp {
  int mode;
  int hexp, vexp;
  int dw, dh;                // downsampled_width / downsampled_height: the samples the reference ever reads
  int pw;                    // samples per row of the plane
  long long plane_off;
};

// the colour conversion behind it (jdcolor.c)
#define MJH_CC_GRAY 0            // component 0 alone: grayscale_convert (a YCbCr file's Y as well)
#define MJH_CC_GRAY_RGB 1        // gray_rgb_convert
#define MJH_CC_YCC_RGB 2         // ycc_rgb_convert
#define MJH_CC_RGB_RGB 3         // a JCS_RGB file: the components as they are
#define MJH_CC_RGB_GRAY 4        // rgb_gray_convert
struct MjhPixOut {
  int W, H;
  int conv;                  // MJH_CC_*
  int ncomp;                 // components the conversion reads (1 or 3)
  int px_size;               // bytes per output pixel: 1, 3 or 4 (2: k_upcolor_565)
  int off_r, off_g, off_b;   // byte of every colour inside a pixel; the fourth byte of a 4-byte pixel is 0xFF
  int bottom_up;             // image row y is stored at output row H - 1 - y (0: at row y)
  long long row_pitch, image_stride;      // of the output, bytes; rows hold whole groups of 4 pixels
  long long planes_per_image;
  MjhUpComp c[3];
};

// the plan of a four-component file (CMYK, YCCK), whose one output is four bytes C, M, Y, K per pixel (jdcolor.c:901-918).  A
// descriptor of its own: MjhPixOut and the kernels that read it stay as they are.
#define MJH_CC4_NULL 0           // a JCS_CMYK file: null_convert, the four samples as they are (Adobe's inverted ones stay inverted)
#define MJH_CC4_YCCK 1           // a JCS_YCCK file: ycck_cmyk_convert (jdcolor.c:543-587)
struct MjhPixOut4 {
  int W, H;
  int conv;                  // MJH_CC4_*
  int bottom_up;
  long long row_pitch, image_stride;      // of the output, bytes; rows hold whole groups of 4 pixels (16 bytes each)
  long long planes_per_image;
  MjhUpComp c[4];
};

// the blocks of one component a region call (mjh_decode_opts.crop_*) transforms, and the compact plane they go to: nbx x nby
// blocks from block (bx0, by0) of the component on; rows of the plane are `pitch` samples apart (a multiple of 4, at least
// nbx * DCT_scaled_size), its row 0 is sample row by0 * DCT_scaled_size of the image, its column 0 sample bx0 * DCT_scaled_size
struct MjhRegComp { int bx0, nbx, by0, nby, pitch; };
struct MjhIdctRegion { MjhRegComp c[3]; };

// K-I1: coefficient planes (what k_dec_store / k_dec_dc leave) -> 8-bit sample planes, real blocks only; comps: the first
// `comps` components.  status != 0: that image is skipped.
void mjh_launch_idct(const MjhConst &C, const MjhIdctQ &Q, int comps, const int16_t *coef_q, uint8_t *planes, const unsigned *status, int n, hipStream_t s);
// K-I1 with the fast integer method (jpeg_idct_ifast, djpeg -dct fast): the same launch, Q holding the AA&N multipliers
// DESCALE(quantval * aanscales, 12) with rounding.  Only components at DCT_scaled_size 8 have such a method.
void mjh_launch_idct_ifast(const MjhConst &C, const MjhIdctQ &Q, int comps, const int16_t *coef_q, uint8_t *planes, const unsigned *status, int n, hipStream_t s);
// K-I1 at a reduced size (djpeg -scale): component ci alone at DCT_scaled_size N of 1, 2 or 4 (jpeg_idct_1x1 / 2x2 / 4x4 of
// jidctred.c), its N x N samples per block into a plane at the component's plane_off whose rows are `pitch` samples apart (a
// multiple of 4, at least wib * N; never more than the full-size plane holds).  Components left at size 8: mjh_launch_idct.
void mjh_launch_idct_scaled(const MjhConst &C, const MjhIdctQ &Q, int ci, int N, int pitch, const int16_t *coef_q, uint8_t *planes, const unsigned *status, int n, hipStream_t s);
// K-I1 at every other size of jidctint.c (mjh_decode_opts.all_scales): component ci alone at DCT_scaled_size N of 3, 5, 6, 7 or
// 9 to 16, its N x N samples per block into a plane at plane_off of an image's planes_per_image samples, rows `pitch` samples
// apart ((wib * N + 3) & ~3).  The layout is the caller's: for N > 8 the plane is larger than the full-size one (mjh_scale_layout.h).
void mjh_launch_idct_sized(const MjhConst &C, const MjhIdctQ &Q, int ci, int N, int pitch, long long plane_off, long long planes_per_image,
                           const int16_t *coef_q, uint8_t *planes, const unsigned *status, int n, hipStream_t s);
// K-I2: sample planes -> interleaved pixels.  Everything it knows of the planes and the image comes from P, so a scaled decode
// is the same kernel given the reduced planes (dw, dh, pw), the group ratios of jdsample.c:454-459 and the scaled W x H.
void mjh_launch_upcolor(const MjhPixOut &P, const uint8_t *planes, uint8_t *pixels, const unsigned *status, int n, hipStream_t s);
// K-I2 for JCS_RGB565: P.px_size 2, P.conv one of MJH_CC_GRAY_RGB / MJH_CC_YCC_RGB / MJH_CC_RGB_RGB; 16-bit little-endian pixels,
// dither != 0: the ordered dither of jdcol565.c by image row and column, 0: plain (JDITHER_NONE)
void mjh_launch_upcolor_565(const MjhPixOut &P, int dither, const uint8_t *planes, uint8_t *pixels, const unsigned *status, int n, hipStream_t s);
// K-I2 for four components: the grid of mjh_launch_upcolor, 4 pixels = 16 bytes = one store per lane
void mjh_launch_upcolor4(const MjhPixOut4 &P, const uint8_t *planes, uint8_t *pixels, const unsigned *status, int n, hipStream_t s);
// K-IR1: the inverse DCT of a region.  The first `comps` components of C, all at DCT_scaled_size 8, each over the blocks R.c[]
// names, into compact planes at the components' plane_off (a region plane is never larger than the full-size one it replaces);
// ifast: the method, as mjh_launch_idct / mjh_launch_idct_ifast (Q: the multipliers of that method).
void mjh_launch_idct_region(const MjhConst &C, const MjhIdctQ &Q, const MjhIdctRegion &R, int comps, bool ifast, const int16_t *coef_q, uint8_t *planes, const unsigned *status, int n, hipStream_t s);
// ... component ci alone at DCT_scaled_size N of 1, 2 or 4 over the blocks rc names (rc.pitch: a multiple of 4 that holds
// nbx * N samples rounded up to whole words)
void mjh_launch_idct_region_scaled(const MjhConst &C, const MjhIdctQ &Q, int ci, int N, const MjhRegComp &rc, const int16_t *coef_q, uint8_t *planes, const unsigned *status, int n, hipStream_t s);
// K-IR2: region planes -> the region's pixels.  P.W x P.H: the region image; P.c[].dw, pw: the region plane's; P.c[].dh: the
// WHOLE image's; P.c[].plane_off: the plane's offset minus (its first sample row * pw), so that rows are addressed by their
// number in the whole image; y0: the region's first row in the (scaled) image.
void mjh_launch_upcolor_region(const MjhPixOut &P, int y0, const uint8_t *planes, uint8_t *pixels, const unsigned *status, int n, hipStream_t s);
void mjh_launch_upcolor_565_region(const MjhPixOut &P, int y0, int dither, const uint8_t *planes, uint8_t *pixels, const unsigned *status, int n, hipStream_t s);
#endif
