// mjh_lossless.h -- geometry of a lossless (SOF3) encode, shared by the host pipeline (mjh_encoder.cpp) and mjh_lossless.hip
#ifndef MJH_LOSSLESS_H
#define MJH_LOSSLESS_H
#include <hip/hip_runtime.h>
#include "mjh_internal.h"

#define LL_UNIT 1024         // pixels of a row per work unit (one workgroup)

// one scan of the script (jpeg_scan_info as validate_script jcmaster.c:390-416 accepts it in lossless mode)
struct LlScan {
  int ncomp;               // components of the scan: its MCU is one sample of each (jcdiffct.c:160-215)
  int comp[3];             // their indices in the frame, ascending
  int psv, pt;             // Ss, Al of THIS scan
  int init_pred;           // 1 << (precision - pt - 1)
  int slot;                // table slot of the scan's optimal table (every scan re-defines DC table 0, jcmarker.c:516)
};

struct LlConst {
  int W, H;
  int ncomp;               // 1 or 3
  int px_size;             // samples per input pixel
  int off[3];              // sample offset of every component inside a pixel
  int precision;           // 8, 12 or 16 (12 / 16: uint16 samples)
  int psv, pt;             // predictor (1..7), point transform of a one-scan image (a script of several: sc[])
  int init_pred;           // 1 << (precision - pt - 1): the first sample of the scan and of every restart interval (jclossls.c:64)
  int rows_per_seg;        // restart interval in rows (0 = none)
  int nseg;                // restart segments
  int units_x, units;      // work units per row / per image (the same in every scan: 1x1 sampling)
  int nscan;               // scans of the script, 1..3 (one scan: all components, sc[0] repeats psv / pt / init_pred)
  LlScan sc[3];
};

// hist: 17 counts per unit; phase 0: statistics; 1: bits per unit, offsets, stream cleared; 2: bit writer.
// hist, len, off, seg_E, mpos, totals and stream hold n * L.nscan "virtual images", scan-major: v = scan * n + image.
void mjh_launch_ll(const LlConst &L, const void *pix, size_t row_pitch, size_t img_stride, MjhHuffTable *tabs, int spi,
                   unsigned *hist, unsigned *len, unsigned *off, unsigned *seg_E, unsigned *mpos, unsigned *totals, unsigned *stream, size_t stream_words,
                   int n, hipStream_t s, int phase);
#endif
