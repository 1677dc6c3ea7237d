// mjh_lossless.h -- geometry of a lossless (SOF3) encode, shared by the host pipeline (mjh_encoder.cpp) and mjh_lossless.hip
#ifndef MJH_LOSSLESS_H
#define MJH_LOSSLESS_H
#include <hip/hip_runtime.h>
#include "mjh_internal.h"

#define LL_UNIT 1024         // pixels of a row per work unit (one workgroup)

struct LlConst {
  int W, H;
  int ncomp;               // 1 or 3
  int px_size;             // samples per input pixel
  int off[3];              // sample offset of every component inside a pixel
  int precision;           // 8, 12 or 16 (12 / 16: uint16 samples)
  int psv, pt;             // predictor (1..7), point transform
  int init_pred;           // 1 << (precision - pt - 1): the first sample of the scan and of every restart interval (jclossls.c:64)
  int rows_per_seg;        // restart interval in rows (0 = none)
  int nseg;                // restart segments
  int units_x, units;      // work units per row / per image
};

// hist: 17 counts per unit; phase 0: statistics; 1: bits per unit, offsets, stream cleared; 2: bit writer
void mjh_launch_ll(const LlConst &L, const void *pix, size_t row_pitch, size_t img_stride, MjhHuffTable *tabs, int spi, int slot,
                   unsigned *hist, unsigned *len, unsigned *off, unsigned *seg_E, unsigned *mpos, unsigned *totals, unsigned *stream, size_t stream_words,
                   int n, hipStream_t s, int phase);
#endif
