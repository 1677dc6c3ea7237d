/*
 * mozjpeg_hip.h -- C ABI of libmozjpeg_hip.so, the MI355X-native JPEG encode hot path.
 *
 * Two layers are exported (plain pointers and sizes only; no C++/torch types):
 *
 *  (1) The batch encoder (mjh_*): the native interface of the GPU pipeline.  One encoder =
 *      one parameter set + one GPU + device-resident working buffers for up to max_batch
 *      equally sized images.  It replaces, for a whole image at a time, the reference's
 *      pixel->bytes path:
 *        jpeg_start_compress      jcapistd.c:44   (parameter capture  -> mjh_encoder_create)
 *        jpeg_write_scanlines     jcapistd.c:90   (pixel hand-over    -> mjh_encode_*)
 *        jpeg_finish_compress     jcapimin.c:176  (passes 1..N + bytes-> mjh_encode_*, mjh_get_jpeg)
 *      and the parameter helpers a caller needs to fill mjh_params:
 *        jpeg_set_defaults        jcparam.c:386   -> mjh_params_defaults
 *        jpeg_set_quality         jcparam.c:360   -> mjh_params_set_quality
 *        jpeg_simple_progression  jcparam.c:859   -> (later rounds)
 *
 *  (2) The libjpeg drop-in symbols (declared in mozjpeg_hip_jpeglib.h, built into
 *      libmozjpeg_hip_jpeg62.so): jpeg_start_compress / jpeg_write_scanlines /
 *      jpeg_finish_compress with the reference's exact signatures (jpeglib.h:1065-1076),
 *      implemented on top of layer (1).
 *
 * Error convention: functions return 0 on success or a negative MJH_E* code;
 * mjh_last_error() returns a thread-local message.  Nothing here falls back to a CPU
 * implementation: an unsupported configuration is an error (MJH_EUNSUPPORTED).
 */
#ifndef MOZJPEG_HIP_H
#define MOZJPEG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MJH_MAX_COMPS 4
#define MJH_MAX_SCANS 64

#define MJH_OK            0
#define MJH_EINVAL       -1   /* bad argument */
#define MJH_EUNSUPPORTED -2   /* configuration outside the GPU hot path (no CPU fallback) */
#define MJH_EHIP         -3   /* HIP runtime error (message has the hipError string) */
#define MJH_ENOMEM       -4
#define MJH_ETOOSMALL    -5   /* output buffer too small */

/* profile values = the reference's JINT_COMPRESS_PROFILE GUIDs (jpeglib.h:353-356) */
#define MJH_PROFILE_MAX_COMPRESSION 0x5D083AAD
#define MJH_PROFILE_FASTEST         0x2AEA5CB4

/* one entry of a progressive scan script (jpeg_scan_info, jpeglib.h:196-201) */
typedef struct {
  int comps_in_scan;
  int component_index[MJH_MAX_COMPS];
  int Ss, Se, Ah, Al;
} mjh_scan;

/* Everything the hot path reads from a jpeg_compress_struct at jpeg_start_compress
 * (SURVEY 8b "Inputs read from cinfo"; field names follow jpeglib.h:399-488 and the
 * extension parameters of jpeglib.h:321-356). */
typedef struct {
  int image_width, image_height;
  int input_components;            /* 3 = interleaved RGB, 1 = grayscale */
  int num_components;              /* 3 = YCbCr output, 1 = grayscale output */
  int h_samp_factor[MJH_MAX_COMPS], v_samp_factor[MJH_MAX_COMPS];
  int quant_tbl_no[MJH_MAX_COMPS], dc_tbl_no[MJH_MAX_COMPS], ac_tbl_no[MJH_MAX_COMPS];
  int component_id[MJH_MAX_COMPS];
  uint16_t quantval[4][64];        /* natural order, = quant_tbl_ptrs[i]->quantval */
  int compress_profile;            /* MJH_PROFILE_* : marker layout (jcmarker.c:189,293) */
  int optimize_coding;
  int trellis_quant, trellis_quant_dc, overshoot_deringing;
  float lambda_log_scale1, lambda_log_scale2;
  unsigned restart_interval;
  int restart_in_rows;
  /* 0 = one sequential scan (baseline).  A script whose first scan has Ss != 0 and Se == 0 is a LOSSLESS file (SOF3), as
   * validate_script decides (jcmaster.c:300-310) and as jpeg_enable_lossless leaves the object (cinfo->Ss = PSV, Se = 0, Ah = 0,
   * Al = Pt, jcparam.c:1016-1040): one scan of every component in order, Ss = the predictor 1..7, Ah = 0, Al = the point
   * transform 0..precision-1 (else JERR_BAD_PROGRESSION) -- or a lossless script of several scans, whatever validate_script
   * accepts for 1 or 3 components (jcmaster.c:332-347, :390-416, :432-436): every component in exactly one scan, the components
   * of a scan in frame order, and PER SCAN Ss = its predictor 1..7, Se = Ah = 0, Al = its point transform < precision; the file
   * is SOF3, then per scan a DHT of table 0 made from that scan's statistics alone and its SOS (the DRI in front of the first
   * SOS only).  A script the reference refuses is MJH_EINVAL with its reason in the text (JERR_BAD_SCAN_SCRIPT,
   * JERR_BAD_PROG_SCRIPT, JERR_MISSING_DATA, with its entry number).  The encoder applies jcmaster.c's overrides itself (1x1 sampling, no
   * smoothing, optimal tables: jcmaster.c:1067-1094) and writes no DQT.  Input is grayscale (input_components 1) or an RGB-family
   * layout coded as JCS_RGB (color_transform MJH_COLOR_NONE), every component with dc_tbl_no 0 (the reference's SOS names table 0
   * for every component of a lossless scan, jcmarker.c:516), in the fastest profile (the max-compression profile writes a DQT and
   * an empty DHT, jcmarker.c:189-254, :293-401), without trellis quantization (JERR_BAD_BUFFER_MODE) or arithmetic coding.
   * data_precision 8, 12 or 16 (16: lossless only; 12 / 16: uint16 samples, row_pitch / image_stride in BYTES).  Restart intervals
   * must be whole rows of the image in every scan (JERR_BAD_RESTART, jclossls.c:289-294).  The planes / coefficient entry points return MJH_EINVAL for a lossless encoder. */
  int num_scans;
  mjh_scan scan_info[MJH_MAX_SCANS];
  int optimize_scans;
  int write_JFIF_header;
  /* layout of one input pixel, the extended RGB colour spaces of jpeglib.h:262-290 / jccolext.c
   * (TurboJPEG's TJPF_*): bytes per pixel (0 = input_components) and the byte offsets of R, G, B
   * (all 0 = R,G,B at 0,1,2).  input_components stays 3 for every RGB-family layout. */
  int input_pixel_size;
  int rgb_offset[3];
  /* 0 or 8: 8-bit samples (one byte each); 12: 12-bit samples stored as uint16 (jpeg12_write_scanlines,
   * J12SAMPLE).  row_pitch / image_stride stay in BYTES.  Trellis quantization has no 12-bit reference
   * behaviour (jccoefct.c:132-138) and is rejected. */
  int data_precision;
  /* JINT_TRELLIS_NUM_LOOPS (jpeglib.h:345, default 1, 0 is read as 1): (statistics, trellis) pass pairs per component,
   * each trellis pass restarting from the unquantized coefficients with the tables of the previous result
   * (jcmaster.c:451-466, :1128-1138) */
  int trellis_num_loops;
  /* cinfo->smoothing_factor (jpeglib.h:459, cjpeg -smooth N), 0..100: input smoothing inside the full-size and the
   * 2x2 downsamplers (jcsample.c:306-455); the other sampling ratios have no smoothing variant in the reference */
  int smoothing_factor;
  /* colour transform between input pixels and JPEG components: MJH_COLOR_YCC (0) = RGB -> YCbCr / gray (rgb_ycc_convert,
   * rgb_gray_convert, grayscale_convert of jccolor.c), MJH_COLOR_NONE = the three input samples become the three
   * components unconverted (null_convert jccolor.c:479, JCS_RGB output = `cjpeg -rgb`; an Adobe APP14 marker with
   * transform 0 replaces the JFIF APP0, component ids are whatever component_id[] says, 'R' 'G' 'B' for cjpeg),
   * MJH_COLOR_YCC_IN = input pixels that are YCbCr already (what an application sets with in_color_space = JCS_YCbCr) */
  int color_transform;
  /* JINT_DC_SCAN_OPT_MODE (jpeglib.h:349, cjpeg -dc-scan-opt N; library default 0, jcparam.c:495): 0 = one DC scan for
   * all components, 1 = one DC scan per component, 2 = luma alone, then chroma interleaved or separate -- with the scan
   * search whichever is smaller (jcmaster.c:836-838, :904-913).  mjh_params_simple_progression /
   * mjh_params_search_progression read it when they build the script (jcparam.c:791-794, :934-947); the encoder
   * reads it for the scan search's final choice of the chroma DC scans. */
  int dc_scan_opt_mode;
  /* JFLOAT_TRELLIS_DELTA_DC_WEIGHT (jpeglib.h:337, cjpeg -trellis-dc-ver-weight W; default 0): weight of the
   * vertical-gradient error against the block above (same iMCU row) in the DC trellis (jcdctmgr.c:1069-1084) */
  float trellis_delta_dc_weight;
  /* JBOOLEAN_USE_SCANS_IN_TRELLIS + JINT_TRELLIS_FREQ_SPLIT (jpeglib.h:326,344; split 0 is read as the default 8):
   * two (statistics, trellis) pass pairs per component, AC bands 1..split and split+1..63 (jcmaster.c:451-460) */
  int use_scans_in_trellis, trellis_freq_split;
  /* JBOOLEAN_TRELLIS_EOB_OPT (jpeglib.h:325): end-of-band runs over all-zero blocks chosen by a second dynamic
   * programme along each block row (jcdctmgr.c:1224-1297) */
  int trellis_eob_opt;
  /* JBOOLEAN_TRELLIS_Q_OPT (jpeglib.h:327): quantization tables re-estimated from the trellis result
   * (sums jcdctmgr.c:1299-1306, update jcmaster.c:1014-1030) */
  int trellis_q_opt;
  /* cinfo->arith_code (jpeglib.h:420, cjpeg -arithmetic): arithmetic entropy coding (jcarith.c) instead of Huffman -- SOF9 /
   * SOF10 frames, DAC markers, no Huffman tables; with trellis_quant the coder's own rate model (quantize_trellis_arith
   * jcdctmgr.c:1334-1667).  An adaptive coder is one dependent chain per scan: this mode is there for completeness, not for
   * throughput.  With trellis_q_opt the reference's pass arithmetic decides whether component 0's table is ever re-estimated
   * (jcmaster.c:687-698, :1016-1030, :1135-1138): reproduced for any number of loops. */
  int arith_code;
  /* cinfo->arith_dc_L / arith_dc_U / arith_ac_K (jpeglib.h:447-449) of conditioning tables 0 and 1: the DC category thresholds
   * (jcarith.c:442-445, :757-760) and the AC position Kx that switches the magnitude bins (:533, :802), written into the DAC
   * marker (emit_dac jcmarker.c:404-448) and read by the coder's trellis (jget_arith_rates jcarith.c:949-951).
   * mjh_params_defaults sets the library defaults 0 / 1 / 5 (jcparam.c:417-419); a table whose three values are all 0 (a
   * zeroed struct of an older caller; Kx = 0 is not a valid conditioning) is read as those defaults.  0 <= L <= U <= 15, 1 <= K <= 63. */
  int arith_dc_L[2], arith_dc_U[2], arith_ac_K[2];
  /* cinfo->Ah / cinfo->Al as the compress object holds them when the image STARTS.  The trellis passes of a progressive image
   * gather their statistics through jcphuff.c with whatever these fields hold -- select_scan_parameters sets Ss / Se for those
   * passes and nothing else (jcmaster.c:451-466): 0 / 0 in a new object, the last coded scan's values when the
   * object has compressed an image before (refinement statistics after a script that ends with a refinement scan, first-pass
   * statistics at the best chroma Al after a scan search).  Read only with num_scans > 0 and trellis_quant. */
  int trellis_stats_Ah, trellis_stats_Al;
  /* cinfo->dc_huff_tbl_ptrs[t] / ac_huff_tbl_ptrs[t] as the object holds them when the image starts, for the two uses the
   * reference has for them: (1) optimize_coding off: the tables the scans are coded with and the DHT markers carry
   * (start_pass_huff -> jpeg_make_c_derived_tbl jchuff.c:190-196, :231-318); (2) a progressive image with the DC trellis: the
   * rates of the DC candidates, because no pass in front of the trellis makes a DC table (compress_trellis_pass
   * jccoefct.c:388-389).  Bit 2 t + is_ac of huff_tables_given says slot t's DC / AC table is given in
   * huff_bits[2 t + is_ac][0..16] (counts per code length, [0] unused) and huff_vals[2 t + is_ac][] (symbols in code order);
   * a slot not given holds the Annex K.3 table for t = 0, 1 (what jpeg_set_defaults installs) and nothing for t = 2, 3.
   * A table must be a legal code (the checks of jpeg_make_c_derived_tbl: JERR_BAD_HUFF_TABLE), DC symbols 0..15; a symbol the
   * image needs and the table lacks is coded with no bits, as jchuff.c does. */
  int huff_tables_given;
  uint8_t huff_bits[8][17];
  uint8_t huff_vals[8][256];
  /* cinfo->dct_method (jpeglib.h:456): 0 = JDCT_ISLOW (jfdctint.c), 1 = JDCT_IFAST (jfdctfst.c: AA&N with 8-bit constants,
   * its scale factors folded into the divisors, jcdctmgr.c:291-345) -- what the legacy TurboJPEG calls select below quality 96
   * (turbojpeg.c:522-527) and `cjpeg -dct fast`.  8- and 12-bit samples. */
  int dct_method;
} mjh_params;

#define MJH_COLOR_YCC  0
#define MJH_COLOR_NONE 1
#define MJH_COLOR_YCC_IN 2   /* the input samples ARE Y, Cb, Cr (in_color_space = JCS_YCbCr, jpeg_color_space = JCS_YCbCr: null_convert
                              * jccolor.c:479 via jinit_color_converter :687-692): unconverted like MJH_COLOR_NONE, but the file is an
                              * ordinary YCbCr one -- JFIF APP0, no Adobe marker, YCbCr's progressive scripts; with num_components = 1 the Y
                              * samples become a grayscale file (grayscale_convert :448-466) */
/* Four-component files are decoded, not written: these two values come from mjh_params_from_jpeg on a CMYK / YCCK file alone and
 * name the colour kind an encoder made from such parameters owns for its mjh_decode_host calls (num_components 4,
 * input_components 4).  Every call that would write a file on such an encoder is MJH_EUNSUPPORTED. */
#define MJH_COLOR_CMYK 3     /* JCS_CMYK: the four components as they are (null_convert jdcolor.c) */
#define MJH_COLOR_YCCK 4     /* JCS_YCCK: Y, Cb, Cr to inverted R, G, B = C, M, Y; K as it is (ycck_cmyk_convert jdcolor.c:543-587) */

typedef struct mjh_encoder mjh_encoder;

/* ---- parameter helpers (host only) ---------------------------------------------------- */
/* jpeg_set_defaults (jcparam.c:386-519) for an RGB->YCbCr (or ->gray) encode of the given size
 * and profile, plus the sampling factors of component 0 (others 1x1). */
int mjh_params_defaults(mjh_params *p, int width, int height, int input_components,
                        int gray_output, int compress_profile, int hsamp, int vsamp);
/* jpeg_set_quality (jcparam.c:360-380) with the base table selected by base_quant_tbl_idx
 * (-1 = the profile's default: 3 for max compression, 0 for fastest; jcparam.c:509-510; 0..8 = cjpeg -quant-table N). */
int mjh_params_set_quality(mjh_params *p, int quality, int force_baseline, int base_quant_tbl_idx);

/* The Annex K.3 Huffman tables jpeg_set_defaults installs (std_huff_tables jstdhuff.c:31-131): bits[0..16] and the
 * symbol list of DC / AC table 0 (luminance) or 1 (chrominance).  Constants owned by the library. */
int mjh_std_huffman_table(int is_ac, int tblno, const uint8_t **bits, const uint8_t **vals, int *nvals);

/* jpeg_simple_progression (jcparam.c:859-1004): the profile's fixed script (9 scans for YCbCr in
 * the max-compression profile, 10 in the fastest profile); clears optimize_scans. */
int mjh_params_simple_progression(mjh_params *p);
/* jpeg_search_progression (jcparam.c:733-852): the 64 (YCbCr) / 23 (gray) candidate scans of the
 * scan search; sets optimize_scans (what jpeg_set_defaults selects in the max-compression profile). */
int mjh_params_search_progression(mjh_params *p);

/* ---- encoder lifetime ----------------------------------------------------------------- */
/* Creates the device-resident state for up to max_batch images of p's geometry on HIP device
 * `device`.  Returns MJH_EUNSUPPORTED for configurations the GPU path does not cover. */
int mjh_encoder_create(const mjh_params *p, int max_batch, int device, mjh_encoder **out);
/* number of visible HIP devices (0 if there is none: every mjh_encoder_create then fails with MJH_EHIP) */
int mjh_device_count(void);
/* Host-side placement of a device (one compress object per thread, libjpeg.txt:2198-2200): the NUMA node the
 * device's PCIe root belongs to (-1: unknown, one-node host, or MJH_NUMA=0), and "run the calling thread on that node's
 * CPUs" (returns the node, or -1 when nothing was changed).  The encoder pins its own staging / result buffers on that
 * node; a client that fills mjh_host_staging buffers or owns pinned frames should do so from a bound thread.
 * mjh_device_placement writes a one-line description (for logs / bench lines) and returns its length. */
int mjh_device_numa_node(int device);
int mjh_bind_thread_to_device(int device);
int mjh_device_placement(int device, char *buf, size_t n);
void mjh_encoder_destroy(mjh_encoder *e);
/* the parameters the encoder was created with (owned by the encoder) */
const mjh_params *mjh_encoder_params(const mjh_encoder *e);

/* ---- one process, several GPUs --------------------------------------------- */
/* A pool owns one encoder per device (devices == NULL: every visible device) and drives each from its own host thread.
 * mjh_pool_encode_host deals the n images of a batch round-robin (image i -> device i mod N, nothing is exchanged
 * between devices), pipelines every device's share through mjh_encode_host / mjh_collect in steps of
 * max_batch_per_device, and returns the finished files in the caller's image order: (*jpegs)[i] is (*sizes)[i] bytes,
 * in host memory owned by the pool, valid until the next call.  Pixels may be pageable or pinned. */
typedef struct mjh_pool mjh_pool;
int mjh_pool_create(const mjh_params *p, int max_batch_per_device, const int *devices, int ndevices, mjh_pool **out);
void mjh_pool_destroy(mjh_pool *pool);
int mjh_pool_device_count(const mjh_pool *pool);
int mjh_pool_encode_host(mjh_pool *pool, const void *pixels, size_t row_pitch, size_t image_stride, int n,
                         const uint8_t *const **jpegs, const size_t **sizes);
const char *mjh_pool_last_error(const mjh_pool *pool);

/* ---- encode ---------------------------------------------------------------------------- */
/* Encode n images that are ALREADY in device memory (interleaved samples, row_pitch bytes per
 * row, image_stride bytes between images).  `stream` is a hipStream_t passed as void*
 * (NULL = the encoder's own stream, which is NOT ordered behind the null stream; (void *)1 =
 * the encoder's own stream, made to wait for everything queued on the null stream so far -- for
 * pixels produced on the legacy default stream).  With MJH_SPLIT=2 in the environment when the
 * encoder is created (sequential mode) a batch larger than half of max_batch runs as two image
 * ranges concurrently on streams of the encoder, forked from and joined into `stream`: about 5 %
 * more throughput on large batches.  Asynchronous: results are valid after
 * mjh_encoder_sync() or any later synchronising call. */
int mjh_encode_device(mjh_encoder *e, const void *d_pixels, size_t row_pitch, size_t image_stride,
                      int n, void *stream);
/* Batches in flight on the encoder's own stream (stream == NULL above): 2 (the default; MJH_INFLIGHT in the environment) -- consecutive
 * mjh_encode_device calls alternate between two complete sets of working buffers and streams inside the encoder, so that the
 * front end of one batch (colour conversion, FDCT) runs next to the tail of the other (final statistics, bit lengths, prefix sums,
 * bit writing, byte stuffing), while the VALU-bound AC trellis of either keeps the chip to itself; the results of
 * call k stay valid until call k + 2, and every accessor (mjh_get_jpeg, mjh_get_output_device, taps, ...) refers to the most recent
 * call.  1 -- one batch at a time on one buffer set (half the device memory).  A caller's stream, debug taps and the memory checker
 * always run one batch at a time.  The files are the same either way. */
int mjh_set_inflight(mjh_encoder *e, int batches);
/* Same with host pixels -- the whole-image form of jpeg_write_scanlines (jcapistd.c:90) + jpeg_finish_compress
 * (jcapimin.c:176) for a batch.  ASYNCHRONOUS and double-buffered: the call queues the host->device copy, the kernel
 * schedule and the hand-over of the finished files to pinned host memory, and returns; the copy of batch k+1 overlaps
 * the kernels of batch k and the hand-over of batch k-1.  Pixels in pinned memory (mjh_host_alloc,
 * mjh_host_register, or the encoder's own buffer from mjh_host_staging) are read by the DMA engine where they lie and
 * must stay untouched until mjh_wait_input or mjh_collect returns; pixels in ordinary (pageable) memory are first
 * copied to a pinned staging buffer by a few worker threads (MJH_HOST_THREADS, default min(8, cores/2)) and may be
 * reused as soon as the call returns.  Results: mjh_collect (zero-copy) or mjh_get_jpeg[_size]. */
int mjh_encode_host(mjh_encoder *e, const void *pixels, size_t row_pitch, size_t image_stride, int n);
/* One finished file of a batch inside the pinned result arena. */
typedef struct { uint64_t offset, size; } mjh_result;
/* Waits for a batch queued by mjh_encode_host -- age 0: the most recent call, age 1: the call before it (so that a
 * loop can queue batch k+1 before it picks up batch k) -- and returns its files where the device put them: file i is
 * results[i].size bytes at (const uint8_t *)base + results[i].offset, in pinned host memory owned by the encoder.
 * The memory of a batch is reused by the SECOND mjh_encode_host call after the one that queued it. */
int mjh_collect(mjh_encoder *e, int age, const void **base, const mjh_result **results, int *count);
/* Blocks until the pixels handed to the most recent mjh_encode_host call have been read (pinned sources only matter). */
int mjh_wait_input(mjh_encoder *e);
/* The encoder's own pinned staging buffer for the NEXT mjh_encode_host call (max_batch images, tightly packed rows):
 * a caller that produces pixels row by row (the libjpeg drop-in's jpeg_write_scanlines) writes them here and passes
 * the pointer to mjh_encode_host, which then copies nothing on the host. */
int mjh_host_staging(mjh_encoder *e, void **buffer, size_t *bytes);
/* The first `bytes` of that staging buffer (packed images, whole rows) are final: their host->device copy is queued now and
 * runs while the caller produces the rest -- what jpeg_write_scanlines does with a client's rows (jcapistd.c:90-135 hands
 * them on strip by strip as well).  The mjh_encode_host call for the buffer copies only the remainder. */
int mjh_stage_commit(mjh_encoder *e, size_t bytes);
/* One batch out of the images n OTHER encoders (same parameters, same device) have staged that way, one image each:
 * image i of the batch = what members[i] holds.  For callers that get their images one at a time from several threads
 * (the libjpeg shim coalesces concurrent jpeg_finish_compress calls): the device then runs ONE schedule for the lot
 * instead of n single-image ones.  Results through mjh_collect / mjh_get_jpeg of `e`; nobody else may use the member
 * encoders during the call. */
int mjh_encode_gather(mjh_encoder *e, mjh_encoder *const *members, int n);
/* Pinned host memory for zero-copy hand-over (hipHostMalloc / hipHostRegister underneath; no HIP types in the ABI). */
void *mjh_host_alloc(size_t bytes);
void mjh_host_free(void *p);
int mjh_host_register(void *p, size_t bytes);
int mjh_host_unregister(void *p);
/* Component planes instead of pixels: jpeg_write_raw_data (jcapistd.c:145) for whole images, the entry
 * tj3CompressFromYUVPlanes8 (turbojpeg.c:1222) uses.  Colour conversion and downsampling are skipped; the
 * encoder must have been created with the sampling factors the planes were made for (input_components and
 * the pixel layout fields are ignored by these calls).  Plane c of image i starts at planes[c] + i *
 * image_stride[c] (image_stride may be NULL for n == 1), its rows are row_pitch[c] BYTES apart and
 * plane_width[c] x plane_height[c] samples of it are valid.  The encoder reads width_in_blocks*8 x
 * height_in_blocks*8 samples per component (mjh_component_geometry); where the plane is smaller its last
 * sample / row is replicated, which is exactly what tj3CompressFromYUVPlanes8 does before it calls
 * jpeg_write_raw_data (turbojpeg.c:1295-1316), so TurboJPEG-layout planes (tj3YUVPlaneWidth/Height) can be
 * passed as they are. */
int mjh_encode_planes_device(mjh_encoder *e, const void *const d_planes[MJH_MAX_COMPS], const size_t row_pitch[MJH_MAX_COMPS],
                             const size_t image_stride[MJH_MAX_COMPS], const int plane_width[MJH_MAX_COMPS],
                             const int plane_height[MJH_MAX_COMPS], int n, void *stream);
int mjh_encode_planes_host(mjh_encoder *e, const void *const planes[MJH_MAX_COMPS], const size_t row_pitch[MJH_MAX_COMPS],
                           const size_t image_stride[MJH_MAX_COMPS], const int plane_width[MJH_MAX_COMPS],
                           const int plane_height[MJH_MAX_COMPS], int n);
/* Quantized DCT coefficients instead of pixels: jpeg_write_coefficients (jctrans.c:44) for whole images -- the
 * lossless re-encode jpegtran performs ("jpegrescan": optimal tables, progressive scan search).  Only the
 * entropy-coding passes run; quantval[] of the parameters is written to the DQT marker unchanged.  The encoder
 * must have been created with trellis_quant = 0 (there is no unquantized data; jpeg_copy_critical_parameters
 * switches it off as well, jctrans.c:102) -- otherwise MJH_EINVAL.  coefs[c] of image i starts at coefs[c] +
 * i * image_stride[c] bytes (image_stride may be NULL for n == 1) and holds height_in_blocks rows of
 * blocks_per_row[c] (>= width_in_blocks) blocks of 64 int16 in natural order (JBLOCKARRAY layout, 4-byte
 * aligned); dummy blocks are generated, not read (compress_output jctrans.c:322-373). */
int mjh_encode_coefficients_device(mjh_encoder *e, const void *const d_coefs[MJH_MAX_COMPS], const size_t blocks_per_row[MJH_MAX_COMPS],
                                   const size_t image_stride[MJH_MAX_COMPS], int n, void *stream);
int mjh_encode_coefficients_host(mjh_encoder *e, const void *const coefs[MJH_MAX_COMPS], const size_t blocks_per_row[MJH_MAX_COMPS],
                                 const size_t image_stride[MJH_MAX_COMPS], int n);
int mjh_encoder_sync(mjh_encoder *e);

/* ---- re-compressing existing files ("jpegrescan": jpegtran -copy none [-optimize | -progressive | ...]) -------------------
 * JPEG bytes in, JPEG bytes out.  The host reads marker segments only; every Huffman symbol is decoded by kernels
 * (mjh_decode.hip), whose output feeds the entropy-coding passes of mjh_encode_coefficients_*.
 * Accepted: Huffman-coded sequential DCT files (SOF0, SOF1), 8-bit, 1 or 3 components, one interleaved scan or several
 * scans (every component in exactly one), any restart intervals.  MJH_EUNSUPPORTED: progressive (unless asked for, see
 * mjh_encoder_set_sources below), arithmetic (unless MJH_SRC_ARITHMETIC, below), lossless (decoded to samples when asked for, MJH_SRC_LOSSLESS below; never re-compressed),
 * 12-bit, 2 components, DNL.  COM / APPn markers are not copied (-copy none) unless mjh_encoder_set_copy_markers asks for
 * them (-copy comments / all / icc, below).
 * Four components (Adobe-style CMYK and YCCK files) are read by the marker walk and DECODED (mjh_decode_host: pixels, planes,
 * coefficients), never written: mjh_params_from_jpeg gives parameters an encoder can be created from (color_transform
 * MJH_COLOR_CMYK / MJH_COLOR_YCCK), and mjh_transcode_host, mjh_encoder_set_transform and every mjh_encode_* call on such an
 * encoder is MJH_EUNSUPPORTED.  The colour space is guessed as default_decompress_parms does (jdapimin.c:130-205): an Adobe
 * APP14 marker with transform 0 or no Adobe marker is CMYK, transform 2 is YCCK; any other transform, which the reference only
 * warns about (JWRN_ADOBE_XFORM), is MJH_EUNSUPPORTED naming the code.  Still refused for four components: lossless files,
 * and an interleaved scan whose MCU exceeds 10 blocks (MJH_EINVAL, JERR_BAD_MCU_SIZE). */
#define MJH_MAX_FILE_SCANS 4
#define MJH_CS_GRAYSCALE 1   /* J_COLOR_SPACE values (jpeglib.h:232-234) */
#define MJH_CS_RGB       2
#define MJH_CS_YCbCr     3
#define MJH_CS_CMYK      4   /* a four-component file; as out_color_space, the one output of four-component files */
#define MJH_CS_YCCK      5   /* a four-component file with Adobe transform 2 (never an output) */
#define MJH_CS_RGB565    16  /* JCS_RGB565: an output of mjh_decode_host only */
typedef struct {
  int comps_in_scan;
  int component_index[MJH_MAX_COMPS];               /* frame index of every component of the scan */
  int dc_tbl_no[MJH_MAX_COMPS], ac_tbl_no[MJH_MAX_COMPS];   /* per component of the scan (Td / Ta of the SOS) */
  unsigned restart_interval;                        /* in force at this SOS (0 = none) */
  size_t data_offset, data_size;                    /* the entropy-coded segment, RSTn markers included, up to the next other marker */
  unsigned restart_markers;                         /* RSTn markers inside it */
  /* the Huffman tables in force at this SOS: slot 2 t + is_ac as in mjh_params; a bit set in huff_defined = that table was defined */
  int huff_defined;
  uint8_t huff_bits[8][17];
  uint8_t huff_vals[8][256];
} mjh_jpeg_scan;
typedef struct {
  int sof_type;                                     /* 0 = SOF0 (baseline), 1 = SOF1 (extended sequential), 2 = SOF2, 3 = SOF3, 9 = SOF9, 10 = SOF10 (2 and above: mjh_jpeg_probe_ex only) */
  int data_precision;
  int image_width, image_height;
  int num_components;
  int component_id[MJH_MAX_COMPS], h_samp_factor[MJH_MAX_COMPS], v_samp_factor[MJH_MAX_COMPS], quant_tbl_no[MJH_MAX_COMPS];
  int quant_defined;                                /* bit t: DQT table t was seen in front of the first SOS */
  uint16_t quantval[4][64];                         /* natural order */
  int jpeg_color_space;                             /* MJH_CS_*, as default_decompress_parms guesses it (jdapimin.c:130-205) */
  int saw_JFIF_marker, JFIF_major_version, JFIF_minor_version, density_unit, X_density, Y_density;
  int saw_Adobe_marker, Adobe_transform;
  int num_scans;
  mjh_jpeg_scan scans[MJH_MAX_FILE_SCANS];
  int lossless_psv, lossless_pt;                    /* appended: a lossless file's first scan, its predictor (Ss) and point transform (Al); else 0 */
} mjh_jpeg_info;
/* Walks the marker segments of one file (jdmarker.c).  Searches the entropy-coded data for 0xFF to find where a scan
 * ends; decodes nothing.  MJH_EINVAL with the reference's reason for malformed headers, MJH_EUNSUPPORTED for file
 * types outside the list above. */
int mjh_jpeg_probe(const void *jpeg, size_t size, mjh_jpeg_info *info);
/* ---- progressive source files (SOF2, Huffman-coded), opt-in ----
 * With nothing set every entry point refuses a progressive file as the list above says.  mjh_jpeg_probe_ex with
 * MJH_SRC_PROGRESSIVE in `accept`, and the calls of an encoder that mjh_encoder_set_sources(e, MJH_SRC_PROGRESSIVE) was called on
 * (mjh_transcode_host, mjh_decode_host with and without raw_coefs), accept 8-bit SOF2 files of 1, 3 or (mjh_decode_host only) 4
 * components; SOF9 / SOF10 (unless MJH_SRC_ARITHMETIC, below), 12-bit, lossless, two components and DNL stay refused in the same words.
 * A progressive file has more scans than mjh_jpeg_info holds: info->sof_type is 2, info->num_scans is 0 and the scans go to
 * scans[0 .. *num_scans), each with its spectral selection (Ss, Se), its successive approximation (Ah, Al) and the Huffman tables
 * and restart interval in force at its SOS (DHT and DRI between scans are normal in these files).  More than
 * min(cap, MJH_MAX_SRC_SCANS) scans: MJH_EUNSUPPORTED with the count.  Every scan is validated as start_pass_phuff_decoder does
 * (jdphuff.c:91-121; a violation is MJH_EINVAL, JERR_BAD_PROGRESSION), and the progression as jdphuff.c:126-144 tracks it in
 * coef_bits: where the reference only warns (JWRN_BOGUS_PROGRESSION: an AC scan before the component's DC scan, a first scan of
 * a coefficient already coded, a refinement whose Ah is not the Al before it), the file is refused with MJH_EUNSUPPORTED.
 * accept = 0: mjh_jpeg_probe (scans, cap, num_scans may be NULL / 0).  A sequential file gives the same info with either flag. */
#define MJH_SRC_PROGRESSIVE 1u
#define MJH_MAX_SRC_SCANS 64     /* the cap on the scans of one progressive file */
/* ---- lossless source files (SOF3, Huffman-coded), opt-in ----
 * With MJH_SRC_LOSSLESS in `accept` (alone or OR-ed with MJH_SRC_PROGRESSIVE) mjh_jpeg_probe_ex accepts lossless files of
 * data_precision 8, 12 or 16 (anything else: MJH_EINVAL, JERR_BAD_PRECISION), 1 or 3 components, every sampling factor 1, one
 * interleaved scan or several scans with every component in exactly one, predictor Ss 1..7 and point transform Al 0..precision-1
 * per scan (else MJH_EINVAL, JERR_BAD_PROGRESSION), tables in any of the four DC slots, and any restart interval that is a whole
 * number of sample rows (else MJH_EINVAL, JERR_BAD_RESTART as jddiffct.c raises it).  It reports them the way it reports a
 * progressive file: info->sof_type is 3, data_precision the file's, num_scans 0, the scans in scans[] with Ss = the predictor,
 * Al = the point transform and Se = Ah = 0; info->lossless_psv / lossless_pt repeat those of the first scan.  Still
 * MJH_EUNSUPPORTED, each naming its reason: arithmetic-coded lossless (SOF11), subsampled components, 2 or 4 components, DNL.
 * mjh_params_from_jpeg on such an info gives the lossless parameters of the file -- mjh_params for an encoder that writes files of
 * its size, precision, components, predictor and point transform with no colour conversion -- and an encoder made from them owns
 * the geometry of mjh_decode_host calls on such files once mjh_encoder_set_sources(e, MJH_SRC_LOSSLESS) was called on it.  The
 * files of one call must agree with it in size, component count and precision; they may differ in predictor, point transform,
 * scan script, tables and restart interval.  mjh_decode_host on a lossless file (jdlhuff.c, jdlossls.c, jddiffct.c: the samples the
 * reference's djpeg writes, which for a file of this library's encoder are the samples that went in, >> Pt << Pt):
 *   out_color_space: 0 or the file's own (MJH_CS_GRAYSCALE for one component, MJH_CS_RGB for three).  There is no colour
 *     conversion: MJH_CS_GRAYSCALE on a three-component file, MJH_CS_RGB on a gray file and MJH_CS_RGB565 are MJH_EUNSUPPORTED
 *     ("Unsupported color conversion request" in the reference), and so are raw_planes and raw_coefs.
 *   pixel_size / rgb_offset: as for DCT files but counted in SAMPLES -- 3 or 4 samples per RGB pixel, the sample of R, G and B
 *     inside it; the fourth sample is the sample maximum 2^precision - 1 (the reference's JCS_EXT_* layouts, jdcolext.c).
 *   bottom_up: honoured.  scale_*, fancy_upsampling, dct_method, no_dither: ignored, as the reference ignores them for these files.
 * Samples are 1 byte (precision 8) or 2 bytes, little-endian (12, 16): mjh_decode_stats reports a pixel_size in BYTES of 1, 2, 3,
 * 4, 6 or 8, and mjh_get_pixels / mjh_get_pixels_device address the image with it; rows hold whole groups of four pixels and are
 * 16-byte aligned as ever.  Damaged entropy-coded data is fatal for that file alone, as on the other decode paths, and its pixels
 * are zeros.  mjh_transcode_host refuses a lossless file whatever is set (jpegtran does: JERR_NOTIMPL, jctrans.c:83). */
#define MJH_SRC_LOSSLESS 2u
/* ---- arithmetic-coded source files (SOF9, SOF10), opt-in ----
 * With nothing set, and with MJH_SRC_PROGRESSIVE alone, every entry point refuses an arithmetic-coded file and a DAC marker in
 * the words it always used.  With MJH_SRC_ARITHMETIC in `accept` (mjh_jpeg_probe_ex, mjh_jpeg_markers, mjh_jpeg_arith_cond) and on
 * an encoder that mjh_encoder_set_sources(e, MJH_SRC_ARITHMETIC [| MJH_SRC_PROGRESSIVE]) was called on, these are accepted and
 * decoded on the device (jdarith.c; mjh_decode_arith.hip):
 *   SOF9  sequential DCT, 8-bit, 1, 3 or (mjh_decode_host only) 4 components, one interleaved scan or several scans with every
 *         component in exactly one, any restart interval.  info->sof_type is 9, the scans are in info->scans[] as for SOF0.
 *   SOF10 progressive DCT, when MJH_SRC_PROGRESSIVE is set as well (with MJH_SRC_ARITHMETIC alone: MJH_EUNSUPPORTED naming the
 *         missing flag).  info->sof_type is 10, the scans go to scans[] as for SOF2 with the same validation, progression
 *         tracking and cap (jdarith.c:638-690 does what jdphuff.c does).
 * In an arithmetic scan huff_defined is 0 and dc_tbl_no / ac_tbl_no hold the conditioning table numbers (Td / Ta).  DAC markers
 * are read as get_dac reads them (jdmarker.c:388-428): any number of (Tc|Tb, value) pairs; a DC entry is L = value & 15,
 * U = value >> 4 with L > U MJH_EINVAL (JERR_DAC_VALUE), an AC entry Kx = value; an index outside 0..15 / 16..31 is MJH_EINVAL
 * (JERR_DAC_INDEX).  Defaults L 0, U 1, K 5; a table keeps its conditioning from scan to scan until a DAC redefines it.  Tables
 * 0..3 are decoded: Td / Ta above 3 in an SOS is MJH_EUNSUPPORTED naming the number (the reference takes 0..15).  With the flag a
 * DAC in a Huffman-coded file is read and ignored.  Still MJH_EUNSUPPORTED with their reason: an SOF9 scan that is not Ss = 0,
 * Se = 63, Ah = Al = 0 (the reference warns JWRN_NOT_SEQUENTIAL), SOF11, 12-bit, two components, DNL.
 * Served: mjh_decode_host (pixels with every option, raw_planes, raw_coefs), mjh_transcode_host with every switch, the probes.
 * Refused with an arithmetic file in the call: a lossless transform (mjh_encoder_set_transform) and, on the way to pixels or
 * planes, an SOF10 file whose blocks the reference would smooth (as for SOF2).  A segment that ends early is not an error
 * (arith_decode feeds zeros behind a marker, jdarith.c:126-145) and decodes as in the reference; what the reference warns about
 * with JWRN_ARITH_BAD_CODE (a spectral or magnitude overflow) damages that file alone, like a bad Huffman code.  The drop-in
 * libraries (libjpeg, the interposing library, TurboJPEG) do not set the flag and keep refusing these files. */
#define MJH_SRC_ARITHMETIC 4u
struct mjh_jpeg_arith_cond {                        /* (a struct tag: the call below bears the same name) */
  int dc_L[4], dc_U[4], ac_K[4];                    /* conditioning of tables 0..3 in force at one SOS */
};
/* The arithmetic conditioning in force at every SOS of a file, in file order: entry i belongs to scan i (info->scans[i] of an
 * SOF9 file, scans[i] of an SOF10 file).  accept: the MJH_SRC_* mask of mjh_jpeg_probe_ex; a file the probe refuses is refused
 * here in the same words; a Huffman-coded file lists what its DAC markers, if any, left.  At most `cap` entries are written
 * (list may be NULL with cap 0); more scans than that: MJH_EINVAL with the number in *count. */
int mjh_jpeg_arith_cond(const void *jpeg, size_t size, unsigned accept, struct mjh_jpeg_arith_cond *list, int cap, int *count);
typedef struct {
  int comps_in_scan;                                /* the fields of mjh_jpeg_scan, in its order */
  int component_index[MJH_MAX_COMPS];
  int dc_tbl_no[MJH_MAX_COMPS], ac_tbl_no[MJH_MAX_COMPS];
  unsigned restart_interval;
  size_t data_offset, data_size;
  unsigned restart_markers;
  int huff_defined;
  uint8_t huff_bits[8][17];
  uint8_t huff_vals[8][256];
  int Ss, Se, Ah, Al;                               /* of the SOS: coefficients Ss..Se (0, 0 = a DC scan), Ah = 0 a first scan, else a refinement to bit Al */
} mjh_jpeg_scan_ex;
int mjh_jpeg_probe_ex(const void *jpeg, size_t size, unsigned accept, mjh_jpeg_info *info, mjh_jpeg_scan_ex *scans, int cap, int *num_scans);
/* The kinds of source file the encoder's mjh_transcode_host / mjh_decode_host calls take beyond the sequential ones: 0 (the state
 * of a new encoder) or any of MJH_SRC_PROGRESSIVE, MJH_SRC_LOSSLESS, MJH_SRC_ARITHMETIC OR-ed together (any other bit: MJH_EINVAL; so is
 * MJH_SRC_ARITHMETIC on an encoder made from lossless parameters, which decodes lossless files alone -- SOF11 is not decoded).  Files of one call may differ in scan script, and progressive and sequential files of
 * one geometry may share a call.  Refused with a progressive file in the call (MJH_EUNSUPPORTED): a lossless transform
 * (mjh_encoder_set_transform), and -- on the way to pixels or planes only -- a file at whose end the reference would smooth blocks
 * (jdcoefct.c smoothing_ok: some AC coefficient of positions 1..9 never sent or not refined to the last bit). */
int mjh_encoder_set_sources(mjh_encoder *e, unsigned accept);
/* The refinement scans of the last call's progressive files: how many levels of scans there were (first scans are level 0 and
 * count; a scan's level is 1 + the highest level among the earlier scans of its file that share a component and overlap its
 * coefficient range; 0 = no progressive file in the call) and, with mjh_set_profiling(e, 1), the milliseconds the levels above 0
 * took together.  The four phases of mjh_transcode_stats cover the first scans.  Any pointer may be NULL. */
int mjh_decode_prog_stats(mjh_encoder *e, int *levels, float *ms);
/* The arithmetic-coded files of the last call: how many chains -- (image, scan, restart segment), one wave each -- were decoded,
 * in how many launches (one for all SOF9 scans, one per scan ordinal of the SOF10 files) and, with mjh_set_profiling(e, 1), the
 * milliseconds they took together.  mjh_transcode_stats and mjh_decode_prog_stats keep their meaning for the Huffman-coded files
 * of the call.  Any pointer may be NULL. */
int mjh_decode_arith_stats(mjh_encoder *e, int *chains, int *launches, float *ms);
/* What jpeg_copy_critical_parameters (jctrans.c:75-171) leaves in the destination object: the profile's defaults
 * (the max-compression profile: optimal tables, progressive with scan search), trellis_quant = 0, and the source's size,
 * colour space, precision, component ids, sampling factors, quantization-table numbers and tables -- not its Huffman tables,
 * scan script or restart interval.  Apply jpegtran's switches to *p afterwards (optimize_coding,
 * mjh_params_simple_progression, restart_interval, num_scans = 0 for a sequential file, ...).
 * A four-component file (jpeg_color_space MJH_CS_CMYK / MJH_CS_YCCK) gives parameters for DECODING alone: num_components and
 * input_components 4, color_transform MJH_COLOR_CMYK / MJH_COLOR_YCCK, the file's ids, factors and quantization tables, a
 * sequential script in either profile.  mjh_encoder_create accepts them as they are (and four components made any other way
 * are MJH_EUNSUPPORTED); the encoder serves mjh_decode_host, and every call that would write a file is MJH_EUNSUPPORTED. */
int mjh_params_from_jpeg(const mjh_jpeg_info *info, int compress_profile, mjh_params *p);
/* Re-codes n files with the encoder's parameters, which mjh_params_from_jpeg made (trellis_quant must be 0).  Every file has
 * to agree with the encoder in everything mjh_params_from_jpeg copies (else MJH_EINVAL naming the file and the field) and
 * may differ in scans, Huffman tables, restart intervals and JFIF version / density, which go into that file's own APP0
 * (jctrans.c:162-170).  Queued like mjh_encode_host; results through mjh_collect / mjh_get_jpeg.  The bytes need not stay
 * valid after the call returns.  Damaged entropy-coded data fails the batch with MJH_EINVAL when its results are waited
 * for (the reference warns and writes a file); mjh_transcode_status then tells the damaged files from the good ones. */
int mjh_transcode_host(mjh_encoder *e, const void *const jpegs[], const size_t sizes[], int n);
/* Code (MJH_OK / MJH_EINVAL / MJH_EUNSUPPORTED) of file i of the last mjh_transcode_host batch and, in *text (may be NULL;
 * owned by the encoder, valid until the next batch), its reason.  Synchronises with the batch. */
int mjh_transcode_status(mjh_encoder *e, int i, const char **text);
/* Files of the last mjh_transcode_host / mjh_decode_host call that mjh_transcode_status knows about: n once the call has looked at
 * its files, 0 when it was refused as a whole (bad arguments or options, an encoder that cannot take it) -- such a call leaves
 * no per-file status, and none of an earlier batch. */
int mjh_transcode_batch_size(mjh_encoder *e);
/* Figures of the last mjh_transcode_host call: subsequence length in bytes (0 = one lane per restart segment), the
 * synchronisation rounds launched, host synchronisations inside the call, and -- with mjh_set_profiling(e, 1) -- the
 * milliseconds of the decoder's phases: [0] first pass + synchronisation rounds, [1] block indices, [2] storing pass,
 * [3] DC sums + scrub.  Any pointer may be NULL. */
int mjh_transcode_stats(mjh_encoder *e, int *subseq, int *rounds, int *host_syncs, float ms[4]);
/* ---- COM / APPn markers kept (jpegtran -copy), ICC profiles written (cjpeg -icc, jpegtran -icc) ----
 * The copy modes are JCOPY_OPTION's (transupp.h): MJH_COPY_NONE is the state of a new encoder and everything above without change. */
#define MJH_COPY_NONE           0
#define MJH_COPY_COMMENTS       1   /* COM only (jpegtran's own default) */
#define MJH_COPY_ALL            2   /* COM + APP0..15 */
#define MJH_COPY_ALL_EXCEPT_ICC 3   /* all but APP2 */
#define MJH_COPY_ICC            4   /* APP2 only */
typedef struct {
  int marker;                /* 0xFE (COM) or 0xE0..0xEF (APPn) */
  size_t data_offset;        /* of the segment's data in the file: the segment itself begins 4 bytes in front, FF xx len len */
  unsigned data_length;      /* without the two length bytes */
} mjh_jpeg_marker;
/* The reference's marker_list of a file under one copy mode (jcopy_markers_setup, transupp.c:2312-2336): every COM / APPn segment
 * the mode saves, in file order -- those between the scans and behind the last one too (jpeg_read_coefficients reads the whole
 * file before anything is written), and JFIF / Adobe segments, which only the writing side may leave out.  accept: the MJH_SRC_*
 * mask of mjh_jpeg_probe_ex; a file the probe refuses is refused here in the same words.  At most `cap` entries are written to
 * list (may be NULL with cap 0); more markers than that: MJH_EINVAL with the number in *count. */
int mjh_jpeg_markers(const void *jpeg, size_t size, unsigned accept, int copy_mode, mjh_jpeg_marker *list, int cap, int *count);
/* The copy mode of the following mjh_transcode_host calls on e (unknown: MJH_EINVAL).  The saved markers go out right behind the
 * SOI / JFIF APP0 / Adobe APP14 the encoder writes, in file order (jcopy_markers_execute, transupp.c:2345-2388): a JFIF APP0 is
 * left out when the encoder writes its own, an Adobe APP14 likewise; a JFXX APP0 is copied.  When the FIRST saved marker is an
 * APP1 that begins "Exif\0\0" (transupp.c:2115-2143) the encoder's JFIF APP0 is not written -- the file begins SOI, APP1 -- and,
 * where the destination's size differs from the source's (crop, trim, a transposing transform), ExifImageWidth / ExifImageHeight
 * of its ExifSubIFD are rewritten (adjust_exif_parameters; in the library's copy, never in the caller's buffer).
 * The markers are inserted where the finished files are handed to the host (k_pack_results_spliced); the files in device memory
 * never hold them.  On an encoder made for four-component files the call is accepted; the calls that write stay refused. */
int mjh_encoder_set_copy_markers(mjh_encoder *e, int copy_mode);
/* An ICC profile for every file the encoder produces from now on (jpeg_write_icc_profile, jcicc.c:49-80: APP2 segments of at
 * most 65519 profile bytes, each "ICC_PROFILE\0", sequence number, count): every mjh_encode_* call of every coder family, where
 * it stands right behind the SOI / APP0 / APP14 (cjpeg.c:957-992), and mjh_transcode_host, where it follows the copied markers
 * and MJH_COPY_ALL acts as MJH_COPY_ALL_EXCEPT_ICC, MJH_COPY_ICC as MJH_COPY_NONE (jpegtran.c:601-604).  NULL, 0 clears it.
 * MJH_EINVAL: a non-NULL pointer with length 0, or more than 255 segments.  The bytes are copied.  Synchronises with the device. */
int mjh_encoder_set_icc_profile(mjh_encoder *e, const void *icc, size_t len);

/* ---- lossless transforms while re-compressing (jpegtran -rotate / -flip / -transpose / -transverse / -crop / -grayscale) ----
 * The semantics are transupp.c's as jpegtran.c drives them: the bytes of `jpegtran -copy none <transform> <coding switches>`.
 * The decoder kernels store every coefficient straight into its place in the DESTINATION frame (block moved, position inside
 * the block transposed, sign of odd columns / rows changed): no second set of coefficient planes and no extra pass.
 * Edges as the reference: without trim the partial iMCU column / row at a mirrored edge stays where it is (copied or only
 * transposed), with trim it is cut off, perfect refuses such a size.  crop applies in output coordinates; its offset moves
 * down to an iMCU boundary and the size grows by the remainder.  grayscale keeps component 0 of a YCbCr file (1x1 factors,
 * its quantization table number); a one-component file gets 1x1 factors as well.
 * MJH_EUNSUPPORTED: crop extension (a crop larger than the image), the f / r suffixes of a crop specification, grayscale on
 * a file that is neither YCbCr nor gray or whose component 0 is not sampled at the maximum (JERR_CONVERSION_NOTIMPL);
 * -drop and -wipe have no operation number here.  MJH_EINVAL: a crop outside the image (JERR_BAD_CROP_SPEC), perfect on a
 * size that is not ("transformation is not perfect").  Markers are not copied (-copy none), so no Exif size is adjusted. */
#define MJH_XFORM_NONE       0   /* JXFORM_CODE (transupp.h) */
#define MJH_XFORM_FLIP_H     1
#define MJH_XFORM_FLIP_V     2
#define MJH_XFORM_TRANSPOSE  3
#define MJH_XFORM_TRANSVERSE 4
#define MJH_XFORM_ROT_90     5
#define MJH_XFORM_ROT_180    6
#define MJH_XFORM_ROT_270    7
#define MJH_CROP_UNSET   0       /* JCROP_CODE */
#define MJH_CROP_POS     1
#define MJH_CROP_NEG     2
#define MJH_CROP_FORCE   3       /* parsed, refused */
#define MJH_CROP_REFLECT 4       /* parsed, refused */
typedef struct {
  int transform;                 /* MJH_XFORM_* */
  int trim, perfect, grayscale;  /* -trim, -perfect, -grayscale */
  int crop;                      /* the crop fields below are in force (mjh_transform_parse_crop sets it) */
  unsigned crop_width, crop_height, crop_xoffset, crop_yoffset;
  int crop_width_set, crop_height_set, crop_xoffset_set, crop_yoffset_set;   /* MJH_CROP_*; NEG: the offset counts from the right / bottom edge */
} mjh_transform;
/* jtransform_parse_crop_spec: WxH+X+Y with any subset of the four numbers and `-` offsets into the crop fields of *t (the other
 * fields stay).  MJH_EINVAL "bogus -crop argument" for anything else. */
int mjh_transform_parse_crop(mjh_transform *t, const char *spec);
/* mjh_params_from_jpeg + jtransform_request_workspace + jtransform_adjust_parameters: the destination's size, sampling factors
 * (swapped by the four transposing operations), quantization tables (transposed by them) and components.  t == NULL or a
 * transform that asks for nothing: exactly mjh_params_from_jpeg. */
int mjh_params_from_jpeg_transform(const mjh_jpeg_info *info, const mjh_transform *t, int compress_profile, mjh_params *p);
/* The transform of the following mjh_transcode_host calls on e (NULL: none, today's path).  The encoder's parameters are the
 * DESTINATION's (mjh_params_from_jpeg_transform).  The source geometry cannot be derived from them (225 and 227 both trim
 * to 224): the first good file of a call defines it, every other file of the call must have the same size and sampling
 * factors, and every file's own destination parameters must equal the encoder's, else MJH_EINVAL naming file and field. */
int mjh_encoder_set_transform(mjh_encoder *e, const mjh_transform *t);

/* ---- decoding existing files to pixels (djpeg [-scale M/N] [-nosmooth] [-grayscale | -rgb]) -------------------------------------
 * JPEG bytes in host memory in, interleaved 8-bit pixels in device memory out (and in host memory on request): the marker walk
 * and the Huffman decoder kernels of mjh_transcode_host, then dequantization + inverse DCT and upsampling + colour conversion
 * (mjh_idct.hip).  The pixels are the bytes the reference's djpeg writes with the slow integer IDCT (-dct int, its default) or,
 * with dct_method 1, the fast one (-dct fast): every sample, every edge, and the wrap of its range-limit table on files with
 * absurd coefficients.
 * The encoder is one made from mjh_params_from_jpeg: it owns the geometry, the quantization tables and the coefficient planes;
 * the files accepted and the agreement every file of a batch must show are those of mjh_transcode_host.
 * out_color_space: 0 = djpeg's default for the file (gray for a one-component file, RGB otherwise), MJH_CS_GRAYSCALE
 * (a YCbCr file: its Y alone, no chroma is transformed; an RGB file: rgb_gray_convert) or MJH_CS_RGB (a gray file: replicated).
 * pixel_size / rgb_offset: the layouts mjh_params.input_pixel_size / rgb_offset name for input -- 3 or 4 bytes per RGB pixel
 * (0 = 3), the byte of R, G and B inside it (all 0 = 0, 1, 2); the fourth byte of a 4-byte pixel is 0xFF.  Gray pixels are
 * one byte.  fancy_upsampling: 1 = djpeg's default, 0 = -nosmooth.
 * MJH_CS_RGB565 (djpeg -rgb565, jdcol565.c): 16-bit pixels ((r << 8) & 0xF800) | ((g << 3) & 0x7E0) | (b >> 3), little-endian, of
 * any file RGB output is made of.
 * Four-component files (CMYK, YCCK): out_color_space 0 resolves to MJH_CS_CMYK, which may also be named; pixel_size is 0 or 4
 * and rgb_offset is ignored.  The pixels are four bytes C, M, Y, K: a CMYK file's samples as they are (Adobe's inverted samples
 * stay inverted, null_convert), a YCCK file's through ycck_cmyk_convert.  Gray, RGB and RGB565 output of such a file, and
 * MJH_CS_CMYK of a file of one or three components, are MJH_EUNSUPPORTED ("Unsupported color conversion request",
 * JERR_CONVERSION_NOTIMPL).  raw_planes gives four planes, raw_coefs four arrays.  CMYK and YCCK files do not share a call.
 * RGB565: pixel_size is 0 or 2, rgb_offset all 0 (mjh_decode_opts_defaults sets 0, 1, 2).  no_dither 0: the reference's ordered dither
 * (dither_mode other than JDITHER_NONE, djpeg's default), added in front of the range limit -- byte x & 3 of
 * dither_matrix[y & 3] (jdcolor.c:619) to red and blue, half of it to green, (x, y) the pixel's place in the (scaled) image:
 * what the reference gives a client that reads one row per jpeg_read_scanlines call into 4-byte aligned rows, as djpeg does
 * (it takes the matrix row from output_scanline at the time of the call).  no_dither 1: plain (-dither none).
 * scale_num / scale_denom: djpeg -scale M/N, decoding at a reduced size inside the inverse DCT (jidctred.c).  The fraction is
 * resolved as jpeg_core_output_dimensions does (jdmaster.c:105ff): to k / 8 with the smallest k in 1..16 for which
 * scale_num * 8 <= scale_denom * k, 16 if there is none -- 1/5 decodes at 2/8.  Every k is built: 1, 2 and 4 (jidctred.c), 8
 * (the full-size path, which 1/1 and 0/0, a zeroed struct, name) and, with all_scales, 3, 5, 6, 7 and 9 to 16 (jpeg_idct_3x3 to
 * jpeg_idct_16x16 of jidctint.c: djpeg -scale 3/8 ... 16/8, enlarging included).
 * all_scales: 0 = a scale that resolves to a k other than 1, 2, 4 or 8 is refused with MJH_EUNSUPPORTED, as it was before those
 * sizes were built (the refusal and its text are part of the tested contract, so the new sizes are an opt-in); 1 = every k in
 * 1..16 decodes.  Components are transformed at k, doubled while it is below 8 and the sampling ratios allow it (jdmaster.c:
 * 287-320), so a 4:2:0 file at k = 5, 6, 7 has its chroma at 10, 12, 14; a call with a component above 8 keeps its sample
 * planes in a buffer of its own (made by the first such call), every other call where they always were.  The output is ceil(W k / 8) x ceil(H k / 8): mjh_decode_stats
 * reports that size, mjh_get_pixels and mjh_get_pixels_device address that image.  The encoder is still the one made from
 * mjh_params_from_jpeg at the file's own size, and serves calls at different scales one after the other.
 * dct_method: the numbers of mjh_params.dct_method -- 0 = JDCT_ISLOW (jidctint.c), 1 = JDCT_IFAST (jidctfst.c: djpeg -dct fast,
 * TurboJPEG's FASTDCT).  As in the reference (jddctmgr.c start_pass) the method holds for components transformed at size 8;
 * the reduced sizes of a scaled call have one transform each.  The fast method's sums are 32-bit as the reference's; on a file
 * whose quantization tables make them overflow (undefined behaviour there) they wrap here.
 * bottom_up: row y of the image is stored at row H - 1 - y of the output, H the scaled height (TurboJPEG's BOTTOMUP).
 * raw_planes: the call stops after the inverse DCT and produces no pixels: the components' sample planes at the call's scale
 * (jpeg_read_raw_data, TurboJPEG's planar YUV output), through mjh_get_plane / mjh_get_planes_device.  EVERY component is then
 * transformed at the scale's own size k (the pixel path may leave subsampled chroma at a larger one, jdmaster.c:287-320), as
 * TurboJPEG forces it (turbojpeg.c:2151-2167): the planes keep the file's subsampling at every scale.  (With dct_method 1
 * the reference then runs the reduced transform of a component the pixel path would have left at size 8 -- chroma of a 4:2:0
 * file at 1/2 -- on the fast method's multiplier table; so does this call, for the reference's bytes.)  out_color_space,
 * pixel_size, rgb_offset, fancy_upsampling and bottom_up are ignored.
 * raw_coefs: the call stops after the Huffman decoder (its DC sums and the scrub of damaged files included) and produces neither
 * pixels nor planes: the files' quantized DCT coefficients (jpeg_read_coefficients, jdtrans.c), through mjh_get_coefs /
 * mjh_get_coefs_device -- per component [height_in_blocks][blocks_per_row][64] int16, block-major, natural order: the arrays
 * mjh_encode_coefficients_host / _device read.  The values are the 16 bits the reference's JCOEF holds; no +-1023 limit is
 * applied (that is the entropy coder's: a file with a larger value decodes here and is refused when it is coded again).  Every
 * other field of the struct is ignored, raw_planes too.  The files accepted are those of mjh_transcode_host.
 * crop_x, crop_y, crop_w, crop_h: a region of the image instead of the whole (jpeg_crop_scanline + jpeg_skip_scanlines, djpeg
 * -crop WxH+X+Y), in pixels of the SCALED output image, one region for all files of the call.  All four 0: the whole image, bit for
 * bit what the struct without them gives.  crop_w 0 / crop_h 0 beside a nonzero field: to the right / bottom edge.  The region
 * must lie inside the scaled image, else MJH_EINVAL ("exceeds the scaled image dimensions").  crop_x is moved LEFT to a multiple
 * of the iMCU column width -- k * max_h_samp_factor, k alone for a one-component file, k the IDCT size of the scale (16 for a
 * 4:2:0 file at 1/1, 2 at 1/8) -- and the width grows by as much, as jpeg_crop_scanline does (jdapistd.c:237-252): the right
 * edge stays where it was asked.  mjh_decode_region reports the region that was decoded; mjh_decode_stats, mjh_get_pixels and
 * mjh_get_pixels_device address THAT image (the aligned width x crop_h), bottom_up flips inside it.  Only the region's blocks are
 * inverse-transformed and only its pixels are made (K-IR).  The pixels are the reference's for the same calls: rows
 * are those of its output for the same column crop, with the real image above and below as the context of fancy vertical
 * upsampling; columns at the LEFT and RIGHT edge of the region may differ from the same columns of a whole decode, because the
 * fancy h2v1 / h2v2 upsamplers of the reference treat the crop edges as image edges (libjpeg.txt, "jpeg_crop_scanline"); RGB565
 * dither counts columns from the region's left edge and rows from the image's top, as there.
 * Restart segments: a sequential Huffman file with restart markers has only the segments decoded that hold MCUs of the block
 * rows the region reads (mjh_decode_region_stats tells how many).  A segment that is left out is NOT checked: a file damaged
 * only there decodes clean, where the reference would at most warn.  Files without restart markers, progressive and
 * arithmetic-coded files are entropy-decoded whole and get the region's pixel stage alone.
 * A region is MJH_EUNSUPPORTED together with raw_planes or raw_coefs, on a four-component file, on a lossless file (as the
 * reference: JERR_NOTIMPL), at an IDCT size other than 1, 2, 4 and 8 (the sizes of all_scales), and with a transform set on
 * the encoder (as every decode call).
 * dct_method, bottom_up, raw_planes, no_dither, raw_coefs, all_scales and crop_x .. crop_h were appended; 0 in all of them is the behaviour of the struct without them.
 * MJH_EINVAL: an unknown colour space, pixel size, offsets or dct_method; a pixel size other than 0 or 2 or an offset with RGB565; a scale_num or scale_denom below 1 (other than 0/0);
 * a region with a negative number or one that exceeds the scaled image dimensions.
 * MJH_EUNSUPPORTED: a lossless transform set on the encoder; without all_scales, a scale that resolves to an IDCT size of 3, 5,
 * 6, 7 or 9 to 16; the region refusals above;
 * the float IDCT and colour quantization have no option here. */
typedef struct {
  int out_color_space;
  int pixel_size;
  int rgb_offset[3];
  int fancy_upsampling;
  int scale_num, scale_denom;
  int dct_method;
  int bottom_up;
  int raw_planes;
  int no_dither;
  int raw_coefs;
  int all_scales;
  int crop_x, crop_y, crop_w, crop_h;
} mjh_decode_opts;
void mjh_decode_opts_defaults(mjh_decode_opts *o);
/* Decodes n files (opts == NULL: the defaults).  Queued on the encoder's stream; the bytes need not stay valid after the call.
 * Damaged entropy-coded data fails the batch with MJH_EINVAL when its pixels are waited for (mjh_get_pixels);
 * mjh_transcode_status then tells the damaged files from the good ones, and a damaged file has no pixels.  Decoding does not
 * apply the entropy coder's coefficient-range check: a value no Huffman code could carry again is still a sample to djpeg. */
int mjh_decode_host(mjh_encoder *e, const void *const jpegs[], const size_t sizes[], int n, const mjh_decode_opts *opts);
/* Waits for the last mjh_decode_host batch and tells whether it is clean: MJH_OK, or MJH_EINVAL naming the first damaged file
 * (whose slot of the device buffer then holds no pixels of this batch).  For callers who stay on the device: the one call
 * between mjh_decode_host and reading mjh_get_pixels_device's buffer. */
int mjh_decode_wait(mjh_encoder *e);
/* Copies image i of the last mjh_decode_host batch to host memory, row_pitch bytes between rows (synchronises). */
int mjh_get_pixels(mjh_encoder *e, int i, void *dst, size_t row_pitch);
/* The device buffer of the last mjh_decode_host batch: pixel (x, y) of image i starts at base + i * image_stride + y * row_pitch
 * + x * pixel_size.  Rows are padded (whole groups of four pixels, 16-byte aligned).  Does not wait: the work is queued on the
 * encoder's stream; mjh_decode_wait waits for it AND reports damaged files, mjh_encoder_sync only waits.  The buffer is reused
 * by the next decode call. */
int mjh_get_pixels_device(mjh_encoder *e, void **d_base, size_t *row_pitch, size_t *image_stride);
/* After a raw_planes call: copies the top-left width x height samples of component comp of image i to host memory, row_pitch
 * bytes between rows (synchronises).  The plane holds the component's real blocks at the call's IDCT size k: (blocks across * k)
 * x (blocks down * k) samples, never fewer than ceil(W h k / (8 hmax)) x ceil(H v k / (8 vmax)); more than that is MJH_EINVAL.
 * After a call that made pixels or coefficients: MJH_EINVAL (and mjh_get_pixels after a raw_planes or raw_coefs call likewise). */
int mjh_get_plane(mjh_encoder *e, int i, int comp, void *dst, size_t row_pitch, int width, int height);
/* The device view of the same planes: sample (x, y) of component comp of image i is at base + i * image_stride + y * row_pitch
 * + x, for x < width and y < height.  Does not wait (see mjh_get_pixels_device).  Any pointer may be NULL. */
int mjh_get_planes_device(mjh_encoder *e, int comp, void **d_base, size_t *row_pitch, size_t *image_stride, int *width, int *height);
/* After a raw_coefs call: the device arrays of component comp.  Coefficient k (natural order) of block (row, col) of image i is
 * the int16 at base + i * image_stride + ((row * blocks_per_row + col) * 64 + k) * 2, for row < height_in_blocks and
 * col < blocks_per_row; the columns from width_in_blocks on are padding (the width the reference rounds its arrays up to) and
 * hold zeros, as every block of a damaged file does.  image_stride = height_in_blocks * blocks_per_row * 128: the batch is one
 * contiguous [n][height_in_blocks][blocks_per_row][64] array, which mjh_encode_coefficients_device takes as it is.  Does not wait
 * (see mjh_get_pixels_device): mjh_decode_wait waits and reports damaged files.  The buffer is made by the first raw_coefs call
 * and reused by the next.  Any pointer may be NULL.  After a call that made pixels or planes: MJH_EINVAL. */
int mjh_get_coefs_device(mjh_encoder *e, int comp, void **d_base, size_t *image_stride, int *blocks_per_row, int *height_in_blocks, int *width_in_blocks);
/* Copies the height_in_blocks x width_in_blocks real blocks of component comp of image i to host memory, dst_blocks_per_row
 * blocks (of 64 int16) between rows, at least width_in_blocks (synchronises).  MJH_EINVAL after a call that made pixels or planes,
 * and for a batch with a damaged file (mjh_transcode_status tells which). */
int mjh_get_coefs(mjh_encoder *e, int i, int comp, void *dst, size_t dst_blocks_per_row);
/* With mjh_set_profiling(e, 1): the milliseconds of the last raw_coefs call's export kernel (0 without profiling), the phase
 * behind the four of the Huffman decoder that mjh_transcode_stats reports for the same call.  It is a call of its own because
 * mjh_transcode_stats and mjh_decode_stats write into arrays of 4 and 2 floats that their callers own: a fifth value there
 * would overrun every caller built against the header as it was.  The Python binding appends it to transcode_stats()["ms"] as
 * "export".  ms may be NULL.  After a call that made pixels or planes: MJH_EINVAL. */
int mjh_get_coefs_ms(mjh_encoder *e, float *ms);
/* Size (the scaled one) and pixel size of the last decoded batch (0 after a raw_planes or raw_coefs call) and, with mjh_set_profiling(e, 1), the milliseconds of its two pixel kernels:
 * [0] dequantization + inverse DCT, [1] upsampling + colour conversion (the Huffman decoder's phases: mjh_transcode_stats).
 * After a batch of lossless files: pixel_size is in bytes (1, 2, 3, 4, 6 or 8), [0] is the undifferencing, [1] the samples into the
 * pixel layout, and of mjh_transcode_stats' four phases the last (DC sums) is 0.  Any pointer may be NULL. */
int mjh_decode_stats(mjh_encoder *e, int *width, int *height, int *pixel_size, float ms[2]);
/* The region of the (scaled) image the last decoded batch holds: x as it was aligned, y as asked, w the width grown by what x
 * moved, h as asked -- w x h is what mjh_decode_stats reports.  A call without a region: 0, 0 and the whole size.  Any pointer
 * may be NULL. */
int mjh_decode_region(mjh_encoder *e, int *x, int *y, int *w, int *h);
/* Restart segments (a scan without restart markers is one) of the last decoded batch's files, and how many of them were
 * entropy-decoded: fewer only for a region call on sequential Huffman files with restart markers.  Any pointer may be NULL. */
int mjh_decode_region_stats(mjh_encoder *e, long long *segments_decoded, long long *segments);

/* The sequential Huffman coder writes a scan without restart intervals in one walk over its blocks (MJH_ENC_ONEPASS=0 in
 * the environment of mjh_encoder_create: the length pass and the second walk of the restart path for every scan).  enabled:
 * that setting.  long_blocks: blocks whose bits outgrew their staging column (256 bits) and were walked twice; big_groups:
 * groups of 256 blocks whose bits outgrew their window (64 Kbit) and were coded by the direct path -- both counted since
 * the encoder was made.  Any pointer may be NULL.  Synchronises with the device. */
int mjh_enc_onepass_stats(mjh_encoder *e, int *enabled, unsigned long long *long_blocks, unsigned long long *big_groups);
/* How many consecutive groups of 256 blocks a workgroup of that walk codes (MJH_ENCP_GROUPS in the environment of
 * mjh_encoder_create, 1 to 64; the files do not depend on it): the encoder's setting, and that of its second buffer set
 * (-1 while none has been made).  Either pointer may be NULL. */
int mjh_enc_pack_groups(mjh_encoder *e, int *groups, int *twin_groups);
/* Whether the latest batch counted its final AC symbol statistics inside the AC trellis kernels instead of in a pass of
 * their own (1 / 0; MJH_FUSE_FINAL_AC=0 in the environment of mjh_encoder_create keeps the pass; the files do not depend
 * on it), and the same of the second buffer set's latest batch (-1 while none has been made).  Either pointer may be NULL. */
int mjh_final_ac_fused(mjh_encoder *e, int *fused, int *twin_fused);
/* Which DC trellis kernels the latest call launched: 0 none, 1 one lane per chain (MJH_DC_LANES), 2 the sliding-window kernel,
 * 3 the general kernel, 4 the speculative pair of one- and two-frame calls. */
int mjh_get_dc_path(mjh_encoder *e, int *path);

/* Size in bytes of JPEG i of the last batch (synchronises): with a copy mode or an ICC profile set, of the file with its markers. */
int mjh_get_jpeg_size(mjh_encoder *e, int i, size_t *size);
/* Copy JPEG i of the last batch to host memory (synchronises). */
int mjh_get_jpeg(mjh_encoder *e, int i, void *dst, size_t cap, size_t *size);
/* Device-side view of the outputs of the last batch: file i starts at base + i*stride and is
 * sizes[i] bytes long (sizes is a device pointer to uint32).  These are the files BEFORE the hand-over: while a copy mode
 * (mjh_encoder_set_copy_markers) or an ICC profile (mjh_encoder_set_icc_profile) is set the call is MJH_EUNSUPPORTED, since
 * the markers go in at the hand-over and the device buffer never holds the files the other accessors return. */
int mjh_get_output_device(mjh_encoder *e, void **d_base, size_t *stride, void **d_sizes);

/* The Huffman table entry `scan` of the scan script was coded with in image `image` of the last batch: bits[0..16] (counts per
 * code length) and the symbols in code order.  Progressive encoders only; tblno selects the DC table of a DC scan (the number its
 * components carry in dc_tbl_no) and is ignored for AC scans.  A scan search codes all its candidates, also those the file
 * leaves out: the libjpeg drop-in keeps the object's table slots as the reference's last coded scans leave them
 * (jpeg_gen_optimal_table writes into cinfo->dc_huff_tbl_ptrs / ac_huff_tbl_ptrs, jchuff.c:1092-1105).  Synchronises. */
int mjh_get_scan_table(mjh_encoder *e, int image, int scan, int tblno, uint8_t bits[17], uint8_t vals[256]);

/* ---- introspection for parity tests and profiling ------------------------------------- */
enum {
  MJH_TAP_PLANE = 1,     /* uint8  [ph][pw] downsampled samples of one component            */
  MJH_TAP_COEF_UQ = 2,   /* int16  [64 zig-zag][nblk] raw DCT (x8) coefficients             */
  MJH_TAP_COEF_Q = 3,    /* int16  [64 zig-zag][nblk] quantized (after trellis if enabled)  */
  MJH_TAP_COEF_Q0 = 4,   /* int16  quantized before trellis (kept only when debug taps on)  */
  MJH_TAP_HUFF_BITS = 5, /* uint8  [4 slots: DC0,AC0,DC1,AC1][17] final tables               */
  MJH_TAP_HUFF_VALS = 6, /* uint8  [4][256]                                                  */
  MJH_TAP_PROG_SCAN_US = 7, /* uint32 [2][64] progressive: microseconds the statistics [0] / encode [1]
                              workgroup of each scan-script entry ran (0 = not run)              */
  MJH_TAP_LL_COUNTS = 8, /* uint32 [17] lossless: symbol histogram (difference categories 0..16) of the table (a script of several
                            scans: of the LAST scan's table, the one the object holds as DC table 0 afterwards; so MJH_TAP_HUFF_BITS / VALS) */
  MJH_TAP_FINAL_COUNTS = 9 /* diagnostic, for the test suite (no caller needs it to encode): uint32 [4 slots: DC0,AC0,DC1,AC1][256]
                              symbol histograms the image's final tables were made from; only what the LAST scan of a script counted */
};
int mjh_set_debug_taps(mjh_encoder *e, int on);
int mjh_read_tap(mjh_encoder *e, int what, int image, int component, void *dst, size_t cap, size_t *size);
/* geometry of component c: blocks across/down (real blocks) and plane size */
int mjh_component_geometry(const mjh_encoder *e, int c, int *width_in_blocks, int *height_in_blocks,
                           int *plane_width, int *plane_height);

/* Per-kernel HIP-event timing.  level 0 = off; 1 = every kernel of the schedule (the events serialise
 * back-to-back launches, so whole-step throughput drops by some percent); 2 = only the dominant kernel
 * (the AC trellis when trellis quantization is on, else the DCT/quantize kernel): two events per encode
 * call.  Times accumulate over the mjh_encode_* calls (at most 256) since the level was set or since the
 * last read; mjh_get_kernel_times synchronises, returns the AVERAGE milliseconds per call and starts a new
 * accumulation (names/ms arrays are owned by the encoder; *count entries). */
int mjh_set_profiling(mjh_encoder *e, int level);
/* Which interval level 2 brackets: a name returned by mjh_get_kernel_times (normally the largest entry of a level-1
 * pass over the same workload, so that "dominant" is measured, not assumed); NULL or "" = the built-in choice.  Takes
 * effect with the next mjh_set_profiling call.  When a batch runs as concurrent image ranges (mjh_encode_device), a
 * kernel's time per call is the sum of its launches over the ranges. */
int mjh_set_profiling_focus(mjh_encoder *e, const char *name);
int mjh_get_kernel_times(mjh_encoder *e, const char *const **names, const float **ms, int *count);

/* Memory checking (debugging aid, environment MJH_GUARD read once per process):
 * 0 = off (device buffers are plain hipMalloc blocks of exactly the size needed), 1 = canaries around every device
 * buffer, 2 / 3 = every device buffer (and a private copy of the caller's device input) ends / starts at an unmapped
 * page, so that a kernel that strays past it faults on the spot.  In the modes 1-3 the canaries are compared whenever
 * a batch is waited for (the call fails with MJH_EHIP and names the buffer); mjh_debug_guard_check does it on demand. */
int mjh_debug_guard_mode(void);
int mjh_debug_guard_check(void);
/* the checker's own test (tools/guard_probe.py): touches one byte at `offset` relative to the end of a 1000-byte buffer */
int mjh_debug_guard_selftest(long offset, int write);

const char *mjh_last_error(void);
const char *mjh_version(void);
/* sizeof(mjh_params) of THIS library.  mjh_params has grown at its end between versions (0.3: arith_code); a caller built
 * against an older header would pass a shorter struct.  Bindings compare their own sizeof with this before the first
 * mjh_encoder_create (the Python binding and both shims do) and fill the struct through mjh_params_defaults, which zeroes it. */
size_t mjh_params_size(void);

#ifdef __cplusplus
}
#endif
#endif /* MOZJPEG_HIP_H */
