// mjh_scale_layout.h -- the arithmetic of a scaled decode call that needs no device: which IDCT size a fraction names, which
// size every component is transformed at, and where the sample planes of a call lie whose components outgrow the full-size
// planes.  Plain C++ without a dependency, so that it can be compiled into a stand-alone program and run under the host
// sanitizers (tools/check_scale_layout.cpp) as well as into mjh_decode_host.
#ifndef MJH_SCALE_LAYOUT_H
#define MJH_SCALE_LAYOUT_H
#include <stddef.h>

#define MJH_LAYOUT_MAXC 4

// the IDCT size k of djpeg -scale num/denom (output = input * k / 8), as jpeg_core_output_dimensions resolves the fraction
// (jdmaster.c:105-235): the smallest k in 1..16 with num * 8 <= denom * k, else 16.  num, denom >= 1.
static inline int mjh_scale_idct_size(int num, int denom)
{
  int s = 1;
  while (s < 16 && (long long)num * 8 > (long long)denom * s) s++;
  return s;
}

// the sizes the kernels of the struct without all_scales are built for (jidctred.c and the full size)
static inline bool mjh_scale_size_is_classic(int k) { return k == 1 || k == 2 || k == 4 || k == 8; }

// DCT_scaled_size of a component with sampling factors h x v in a frame of maxh x maxv at the call's size k: k, doubled while
// it is below 8 and the sampling ratios allow it (jpeg_calc_output_dimensions jdmaster.c:287-320) -- so up to 14 from k = 7
static inline int mjh_scaled_size(int k, int h, int v, int maxh, int maxv)
{
  int ss = k;
  while (ss < 8 && (maxh * k) % (h * ss * 2) == 0 && (maxv * k) % (v * ss * 2) == 0) ss *= 2;
  return ss;
}

// samples between rows of a plane of wib blocks at size ss: whole words of the kernels' stores
static inline int mjh_scaled_pitch(int wib, int ss) { return (wib * ss + 3) & ~3; }

// The sample planes of one call.  own == false: every component is at most at size 8 and lies at its full-size plane's place in
// the encoder's own planes (off and stride are not set: the addresses of a call stay what they were).  own == true: some
// component is larger than 8, and the call has a layout of its own -- component c at off[c] of an image's `stride` samples,
// pitch[c] x (hib[c] * ssize[c]) samples each, offsets and stride multiples of 16.
struct MjhPlaneLayout {
  bool own;
  int pitch[MJH_LAYOUT_MAXC];
  size_t off[MJH_LAYOUT_MAXC];
  size_t stride;
};

static inline void mjh_plane_layout(int ncomp, const int wib[], const int hib[], const int ssize[], MjhPlaneLayout *L)
{
  L->own = false;
  L->stride = 0;
  for (int c = 0; c < MJH_LAYOUT_MAXC; c++) { L->pitch[c] = 0; L->off[c] = 0; }
  for (int c = 0; c < ncomp; c++) {
    L->pitch[c] = mjh_scaled_pitch(wib[c], ssize[c]);
    if (ssize[c] > 8) L->own = true;
  }
  if (!L->own) return;
  size_t at = 0;
  for (int c = 0; c < ncomp; c++) {
    L->off[c] = at;
    at += (size_t)L->pitch[c] * ((size_t)hib[c] * (size_t)ssize[c]);
    at = (at + 15) & ~(size_t)15;
  }
  L->stride = at;
}

// bytes of the buffer that holds such planes for a batch of max_batch images; 0: the product does not fit a size_t
static inline size_t mjh_plane_layout_bytes(const MjhPlaneLayout *L, int max_batch)
{
  if (max_batch < 1 || L->stride > (size_t)-1 / (size_t)max_batch) return 0;
  return L->stride * (size_t)max_batch;
}
#endif
