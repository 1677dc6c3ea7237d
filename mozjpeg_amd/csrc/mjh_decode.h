// mjh_decode.h -- descriptors shared by the host side of mjh_transcode_host (mjh_encoder.cpp) and the Huffman decoder kernels
// (mjh_decode.hip, mjh_decode_prog.hip, mjh_decode_lossless.hip; their shared device code: mjh_decode_dev.h).  The host reads marker segments only (mjh_jpeg_probe); every Huffman symbol is decoded on the device.
#ifndef MJH_DECODE_H
#define MJH_DECODE_H
#include <hip/hip_runtime.h>
#include "mjh_internal.h"

#define MJH_DEC_WG 256           // lanes (= subsequences) per workgroup; a workgroup serves ONE (image, scan)

// jpeg_make_d_derived_tbl (jdhuff.c:169-308) of one table: 8-bit look-ahead (nbits << 8 | symbol, 0 = longer code),
// maxcode[1..16] (-1: no code of that length; [17] ends the search), valoff[l] = index of the first symbol of length l - its code
struct MjhDecTable {
  uint16_t look[256];
  int maxcode[18];
  int valoff[18];
  uint8_t huffval[256];
};

// one (image, scan) pair
struct MjhDecScan {
  int image;
  int ncomp;                 // components of the scan
  int comp[MJH_MAXC];        // their frame indices
  int dctab[MJH_MAXC], actab[MJH_MAXC];   // indices into the batch's MjhDecTable array
  int nb[MJH_MAXC];          // blocks of each component per MCU (h * v; 1 in a single-component scan)
  int bpm;                   // blocks per MCU
  int canon[10];             // block-in-MCU index b -> the smallest b' from which the same sequence of tables follows: states that differ only in
                             // such b decode alike for ever (three components on one table pair never tell b), so they count as one state
  int ri;                    // restart interval in MCUs (no interval: the scan's MCU count)
  int mcus, mcus_per_row;    // single-component scan: the component's real blocks, raster order (per_scan_setup jdinput.c:116-140)
  long long diff_off;        // element offset of the scan's first component inside one image's DC-difference array
};

// one restart segment: bytes [off, off + len) of the batch buffer (no marker inside), MCUs [mcu0, mcu0 + nmcu) of its scan
struct MjhDecSeg {
  unsigned long long off;
  unsigned len;
  int scan;
  int mcu0, nmcu;
  int sub0, nsub;            // its subsequences: entries [sub0, sub0 + nsub) of the batch's subsequence arrays
};

// decoder state between two code words: p = bit position inside the segment (never inside a stuffed zero byte), k = next
// coefficient position of the block in progress (0: its DC symbol comes next), b = block inside the MCU; n = blocks
// completed inside the subsequence the record belongs to (not part of the comparison)
struct MjhDecState { unsigned p, kb, n, pad; };
struct MjhDecCarry { unsigned p, kb; int next, active; };

// per-image status bits of a transcode batch
#define MJH_DEC_CORRUPT 1u     // the entropy-coded data does not decode to exactly the scan's blocks
#define MJH_DEC_BADCOEF 2u     // an AC value beyond MjhDecBatch::coef_limit (re-compression: what jchuff.c:596,624 can code)

struct MjhDecBatch {
  const uint8_t *bytes;            // the files, back to back
  const MjhDecScan *scans;
  const MjhDecSeg *segs;
  const unsigned *sub_seg;         // subsequence -> segment (0xFFFFFFFF: padding up to the workgroup size)
  const MjhDecTable *tables;
  MjhDecState *state;              // [subsequence] state at its END
  MjhDecCarry *carry;              // [subsequence] the lane that started there
  unsigned *ord;                   // [subsequence] blocks of the segment completed in front of it
  unsigned *changed;               // [round of the group]
  unsigned *status;                // [image]
  int16_t *diff;                   // [image][C.total_mcu_blocks] DC differences in scan order, dummy blocks included
  int nsub_padded, nseg, nscan, n;
  int S;                           // subsequence length in bytes
  int coef_limit;                  // an AC value beyond +-coef_limit sets MJH_DEC_BADCOEF: 1023 where the file is coded again (the encoder has no
                                   // symbol for more), 32767 = never on the way to pixels (the decompressor takes any amplitude a symbol exists for)
};

// What a scan of a progressive file adds to MjhDecScan: entry i of a parallel array belongs to scan i of the same batch (MjhDecScan
// keeps its layout: dec_load_scan copies it into LDS word by word).  Ss..Se: the coefficient positions the scan codes
// (0..0: a DC scan, then ncomp may be > 1; else one component and diff_off is unused); Ah = 0: a first scan, values << Al; else a
// refinement of bit Al
struct MjhDecProg { int Ss, Se, Ah, Al; };

// Arithmetic-coded files (SOF9, SOF10; mjh_decode_arith.hip): entry i of a parallel array belongs to scan i of the same batch and holds
// the conditioning in force at its SOS for tables 0..3; MjhDecScan::dctab / actab then hold the scan's conditioning table NUMBERS
// (Td / Ta) and canon, diff_off and the subsequence arrays are not looked at
struct MjhDecArith { int dc_L[4], dc_U[4], ac_K[4]; };

// Lossless files (SOF3, mjh_decode_lossless.hip).  The entropy-coded data of a scan is one difference symbol per sample, so a scan
// goes through the phases above with "block" = sample: MjhDecScan::nb is 1 for every component, mcus = W * H, mcus_per_row = W, and
// the scan-order difference array becomes one plane of 16-bit differences per component, rows MjhLlGeom::Wp elements apart (component
// j of a scan: diff_off + j * H * Wp).  The undifferencing kernels turn every plane into the reconstructed samples in place.
struct MjhLlPlane {          // one (image, component), indexed image * ncomp + component
  long long off;             // of its plane inside the image's difference array, in elements
  int psv, pt;               // predictor 1..7 and point transform of the scan the component is in
  int rows;                  // rows per restart interval (no interval: H)
  int pad;
};
struct MjhLlGeom {
  int W, H;
  int Wp;                    // elements between rows of a plane: W rounded up to 8 (16-byte rows)
  int ncomp, precision;
  int max_intervals;         // the most restart intervals any plane of the batch has
  long long per_image;       // elements of one image's difference array: ncomp * H * Wp
};
// where the samples go: `px` samples per pixel (1: gray; 3 or 4: component c at sample off[c], the fourth sample = fill), each of
// 1 byte (precision 8) or 2 (12, 16; little-endian); rows hold whole groups of 4 pixels
struct MjhLlOut {
  int px, off[3], fill, bottom_up;
  long long row_pitch, image_stride;     // bytes
};

// A lossless transform fused into the two places that store coefficients (mjh_encoder_set_transform): the kernels decode in the
// SOURCE frame's geometry (the MjhConst they get is the source's) and store into the DESTINATION frame's planes.  Every operation
// of transupp.c is: transpose or not; mirror the whole iMCUs in x and / or y (a partial iMCU at that edge stays in place); cut.
// Inside a block the same: zig-zag position k goes to zz_t[k] under a transposition, and a block that was mirrored in x / y has
// the coefficients of its odd columns / rows negated (bit k of odd_col / odd_row: destination position k lies in one).
struct MjhXformComp {        // indexed by SOURCE component
  int nblk;                  // blocks of the destination component (0: the component is dropped)
  int wib, hib, kstride;     // of the destination component
  int cw, ch;                // blocks across / down that mirror (whole iMCUs of the uncropped image)
  int xcb, ycb;              // crop offset in blocks
  long long coef_off;        // of the destination component inside one image's plane set
};
struct MjhXform {
  int transpose, mirror_x, mirror_y, pad;
  long long coefs_per_image; // of the destination
  unsigned long long odd_col, odd_row;
  MjhXformComp c[MJH_MAXC];
  uint8_t zz_t[64];
};

// phase 0 (first): every lane decodes its own subsequence from the guessed state; q >= 1: one synchronisation round (exits at once
// when round q - 1 of the group changed nothing); then block indices, the storing pass, the DC running sums and the scrub of damaged
// images.  PS == nullptr: B holds sequential scans; else the first scans of progressive files, PS[i] belonging to B.scans[i] (a batch
// of their own; k_dec_prefix serves both).  X == nullptr: no transform; else C = the SOURCE frame's geometry and X (device memory) =
// where things go.  PS and X together do not exist: the host refuses a transform of a progressive file.
void mjh_launch_dec_sync(const MjhConst &C, const MjhDecBatch &B, const MjhDecProg *PS, int q, int first, hipStream_t s);
void mjh_launch_dec_prefix(const MjhDecBatch &B, hipStream_t s);
void mjh_launch_dec_store(const MjhConst &C, const MjhDecBatch &B, const MjhDecProg *PS, const MjhXform *X, int16_t *coef_q, hipStream_t s);
void mjh_launch_dec_dc(const MjhConst &C, const MjhDecBatch &B, const MjhDecProg *PS, const MjhXform *X, int16_t *coef_q, hipStream_t s);
// refinement scans of progressive files (mjh_decode_prog.hip): B.segs[0 .. B.nseg) are the restart segments of ONE level's DC
// (dc_refine) or AC (ac_refine) refinement scans; sub_seg / state / carry / ord / diff are not looked at.
void mjh_launch_pdec_dc_refine(const MjhConst &C, const MjhDecBatch &B, const MjhDecProg *PS, int16_t *coef_q, hipStream_t s);
void mjh_launch_pdec_ac_refine(const MjhConst &C, const MjhDecBatch &B, const MjhDecProg *PS, int16_t *coef_q, hipStream_t s);
// the first pass / a synchronisation round and the storing pass of a batch of lossless scans (k_dec_prefix between them); the stores
// go to B.diff alone and no DC phase follows.  C: "blocks" = samples (h = v = 1, wib = W, hib = H, total_mcu_blocks = G.per_image)
void mjh_launch_ldec_sync(const MjhConst &C, const MjhDecBatch &B, int q, int first, hipStream_t s);
void mjh_launch_ldec_store(const MjhConst &C, const MjhDecBatch &B, hipStream_t s);
// undifferencing (jdlossls.c) of all planes of the batch in place, then the samples << pt into the pixel layout; an image whose
// status is set gets zeros
// (above: n * ncomp * H words of scratch, the column-0 chain of the predictor 1 planes)
void mjh_launch_ll_undiff(const MjhLlGeom &G, const MjhLlPlane *planes, int16_t *diff, unsigned *above, int n, hipStream_t s);
void mjh_launch_ll_pixels(const MjhLlGeom &G, const MjhLlPlane *planes, const int16_t *diff, const MjhLlOut &O, uint8_t *pixels, const unsigned *status, int n, hipStream_t s);
// arithmetic-coded scans: one wave per restart segment of B.segs[0 .. B.nseg), decoded and stored in one go (no other phase; the
// scrub follows as for the other kinds).  whole_blocks: the scans of sequential files (PS may be nullptr); else PS[i] belongs to
// B.scans[i] and the launch holds ONE scan ordinal of every progressive file.  AR[i]: the conditioning of B.scans[i]
void mjh_launch_adec_scans(const MjhConst &C, const MjhDecBatch &B, const MjhDecProg *PS, const MjhDecArith *AR, int whole_blocks, int16_t *coef_q, hipStream_t s);
void mjh_launch_dec_scrub(const MjhConst &C, const MjhDecBatch &B, int16_t *coef_q, void *meta, hipStream_t s);
// after the encode: image i's JFIF version / density bytes (7 bytes at file offset 11) and its status from the encoder's own checks
void mjh_launch_dec_finish(const uint8_t *jfif7, int patch, uint8_t *out, size_t out_stride, const void *meta, unsigned *status, int n, hipStream_t s);
#endif
