/*
 * jpeg_dapi.c -- the libjpeg DECOMPRESS API of the stand-alone libjpeg.so.62 (next to jpeg_api.c, the compress half): an
 * unchanged client such as djpeg reads JPEG files through it, and the pixels are the GPU decoder's (mjh_decode_host: the
 * Huffman decoder kernels of mjh_decode.hip, K-I of mjh_idct.hip).
 *
 * What is restated here is host-side bookkeeping: the object's life cycle, the source managers, the marker reader with its
 * trace messages, saved markers and client marker processors (jdmarker.c), the defaults and output dimensions of
 * jdapimin.c / jdmaster.c.  Everything after the first SOS header is the device's: jpeg_start_decompress reads the rest of the
 * datastream through the client's source manager, hands ONE file to an encoder made from mjh_params_from_jpeg (leased from
 * the cache of the compress half), waits, and keeps the pixels in host memory; jpeg_read_scanlines copies rows out.
 * jpeg_read_coefficients (jdtrans.c) does the same with mjh_decode_opts.raw_coefs and hands out the quantized coefficients in
 * virtual arrays of the object's memory manager: an unchanged jpegtran runs on this library alone.  The arrays have the
 * reference's padded dimensions and hold the reference's real blocks; their PADDING blocks are zero, where the reference keeps
 * whatever an interleaved scan coded for its dummy blocks (jpeg_write_coefficients and transupp.c read real blocks only).
 *
 * Four-component files (Adobe-style CMYK and YCCK) are served like any other: out_color_space JCS_CMYK, which jpeg_read_header leaves
 * for them, gives four output components (null_convert / ycck_cmyk_convert on the device); every other output of them, and JCS_CMYK
 * of any other file, is JERR_CONVERSION_NOTIMPL as in the reference.
 *
 * Not built (JERR_NOT_COMPILED with one line on stderr): suspension (a source that returns FALSE: JERR_CANT_SUSPEND), buffered-image
 * mode, colour quantization, the float IDCT, IDCT sizes other than 1, 2, 4, 8, cropping / skipping scanlines,
 * and every source mjh_jpeg_probe refuses.  Damaged entropy-coded data is FATAL at jpeg_start_decompress (the reference warns and
 * delivers a partial image): JERR_INPUT_EOF when the source ran dry (it said JWRN_JPEG_EOF), else JWRN_HUFF_BAD_CODE's text
 * as an error.
 *
 * Compiled against the libjpeg headers of the tree it replaces (struct jpeg_decompress_struct is ABI).
 */
#define JPEG_INTERNALS
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "jinclude.h"
#include "jpeglib.h"   /* JPEG_INTERNALS: jpegint.h + jerror.h */

#include "mozjpeg_hip.h"
#include "jpeg_shim.h"

/* MOZJPEG_HIP_TIMING=1: seconds spent per phase of a decompression, summed over threads, printed when the library is unloaded
 * (the compress half prints its own line, jpeg_shim.c) */
static int d_timing = 0;
static double d_t[5];           /* source reading, marker walk + encoder lease, mjh_decode_host + wait, copy-out, row copies */
static unsigned long d_images;
static pthread_mutex_t d_tlock = PTHREAD_MUTEX_INITIALIZER;
static double d_now(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; }
static void d_acc(int what, double dt, int image) { pthread_mutex_lock(&d_tlock); d_t[what] += dt; d_images += image; pthread_mutex_unlock(&d_tlock); }
static void __attribute__((constructor)) d_timing_init(void) { const char *v = getenv("MOZJPEG_HIP_TIMING"); d_timing = v && atoi(v) > 0; }
static void __attribute__((destructor)) d_report(void)
{
  if (d_timing > 0 && d_images)
    fprintf(stderr, "mozjpeg_hip decompress timing: %lu images; per image: source %.3f ms, probe+lease %.3f ms, decode+wait %.3f ms, copy-out %.3f ms, rows %.3f ms\n",
            d_images, 1e3 * d_t[0] / d_images, 1e3 * d_t[1] / d_images, 1e3 * d_t[2] / d_images, 1e3 * d_t[3] / d_images, 1e3 * d_t[4] / d_images);
}

#define M_SOF0 0xC0
#define M_SOF1 0xC1
#define M_SOF2 0xC2
#define M_SOF3 0xC3
#define M_DHT 0xC4
#define M_JPG 0xC8
#define M_SOF9 0xC9
#define M_SOF10 0xCA
#define M_SOF11 0xCB
#define M_DAC 0xCC
#define M_RST0 0xD0
#define M_RST7 0xD7
#define M_SOI 0xD8
#define M_EOI 0xD9
#define M_SOS 0xDA
#define M_DQT 0xDB
#define M_DNL 0xDC
#define M_DRI 0xDD
#define M_APP0 0xE0
#define M_APP14 0xEE
#define M_APP15 0xEF
#define M_COM 0xFE
#define M_TEM 0x01

#define APP0_DATA_LEN 14     /* what the library looks at of an APP0 / APP14 segment (jdmarker.c:599-601) */
#define APP14_DATA_LEN 12
#define APPN_DATA_LEN 14

/* the marker reader: the public part the headers define, then who handles COM (slot 16) and APPn (slots 0..15) */
typedef struct {
  struct jpeg_marker_reader pub;
  jpeg_marker_parser_method client[17];   /* jpeg_set_marker_processor; NULL: the library (save or skip by limit[]) */
  unsigned int limit[17];                 /* jpeg_save_markers: bytes to keep, 0 = none */
} d_marker;

/* the master: the public part, then the image in work */
typedef struct {
  struct jpeg_decomp_master pub;
  unsigned char *file;         /* the datastream rebuilt for mjh_decode_host: SOI, tables kept from earlier datastreams, the segments */
  size_t file_len, file_cap;   /* the decoder reads (APP0 / APP14 as far as they were examined), entropy-coded data, EOI */
  int recording;               /* bytes taken from the source go into `file` */
  int q_seen, dc_seen, ac_seen;   /* table slots this datastream has defined so far */
  int eof_seen;                /* the source manager said JWRN_JPEG_EOF (it then supplies a fake EOI) */
  unsigned char *pixels;       /* the decoded image, output_height rows of row_bytes */
  size_t row_bytes;
  unsigned char *planes[MAX_COMPONENTS];   /* raw_data_out: the components' real blocks */
  size_t plane_w[MAX_COMPONENTS], plane_h[MAX_COMPONENTS];
  mjh_encoder *enc;            /* leased only inside jpeg_start_decompress / jpeg_read_coefficients */
  jvirt_barray_ptr *coef_arrays;   /* jpeg_read_coefficients: one array per component (JPOOL_IMAGE: gone with jpeg_abort) */
  int latching;                /* jpeg_read_coefficients: every scan's components get their quant_table as the scan starts */
  /* MOZJPEG_HIP_REGIONS=1: jpeg_start_decompress prepares the call and leaves it to the first jpeg_read_scanlines /
   * jpeg_finish_decompress (decode_pending), so that a jpeg_crop_scanline in between can narrow its columns */
  int pending, px;
  mjh_decode_opts opts;
  unsigned crop_x, crop_w;     /* jpeg_crop_scanline: the aligned columns (crop_w 0: none) */
} d_master;

#define DM(cinfo) ((d_master *)(cinfo)->master)
#define DK(cinfo) ((d_marker *)(cinfo)->marker)

static void refuse(j_decompress_ptr cinfo, const char *why)
{
  fprintf(stderr, "mozjpeg_hip: %s\n", why);
  ERREXIT(cinfo, JERR_NOT_COMPILED);
}

/* jpeg_abort / jpeg_destroy on a decompress object: the image in work goes, an encoder lease is handed back */
void mjh_dapi_drop(void *obj)
{
  j_decompress_ptr cinfo = (j_decompress_ptr)obj;
  d_master *m = DM(cinfo);
  int ci;
  if (m == NULL) return;
  free(m->file); m->file = NULL; m->file_len = m->file_cap = 0; m->recording = 0;
  free(m->pixels); m->pixels = NULL;
  for (ci = 0; ci < MAX_COMPONENTS; ci++) { free(m->planes[ci]); m->planes[ci] = NULL; }
  if (m->enc) { mjh_shim_cache_release(m->enc); m->enc = NULL; }
  m->coef_arrays = NULL; m->latching = 0;
  m->pending = 0; m->crop_x = m->crop_w = 0;
}

/* =====================================================================================================================
 * input: everything comes through the client's jpeg_source_mgr
 * ===================================================================================================================== */
static void file_put(j_decompress_ptr cinfo, const unsigned char *p, size_t n)
{
  d_master *m = DM(cinfo);
  if (m->file_len + n > m->file_cap) {
    size_t cap = m->file_cap ? m->file_cap * 2 : 65536;
    unsigned char *nb;
    while (cap < m->file_len + n) cap *= 2;
    nb = (unsigned char *)realloc(m->file, cap);
    if (nb == NULL) ERREXIT1(cinfo, JERR_OUT_OF_MEMORY, 8);
    m->file = nb; m->file_cap = cap;
  }
  memcpy(m->file + m->file_len, p, n);
  m->file_len += n;
}
static void file_put1(j_decompress_ptr cinfo, int v) { unsigned char b = (unsigned char)v; file_put(cinfo, &b, 1); }

static void src_fill(j_decompress_ptr cinfo)
{
  struct jpeg_error_mgr *err = cinfo->err;
  const long warned = err->num_warnings;
  if (!(*cinfo->src->fill_input_buffer) (cinfo)) ERREXIT(cinfo, JERR_CANT_SUSPEND);   /* suspension is not built */
  if (err->num_warnings != warned && err->msg_code == JWRN_JPEG_EOF) DM(cinfo)->eof_seen = 1;
}

static int src_byte(j_decompress_ptr cinfo)
{
  struct jpeg_source_mgr *s = cinfo->src;
  int c;
  if (s->bytes_in_buffer == 0) src_fill(cinfo);
  s->bytes_in_buffer--;
  c = *s->next_input_byte++;
  if (DM(cinfo)->recording) file_put1(cinfo, c);
  return c;
}
static long src_2bytes(j_decompress_ptr cinfo) { const int hi = src_byte(cinfo); return ((long)hi << 8) + src_byte(cinfo); }

/* ---- the stock source managers -- jdatasrc.c ------------------------------------------------------------------------ */
#define INPUT_BUF_SIZE 4096
typedef struct {
  struct jpeg_source_mgr pub;
  FILE *infile;
  JOCTET *buffer;
  boolean start_of_file;
} stdio_src;

static void stdio_init_source(j_decompress_ptr cinfo) { ((stdio_src *)cinfo->src)->start_of_file = TRUE; }
static boolean stdio_fill(j_decompress_ptr cinfo)
{ /* fill_input_buffer jdatasrc.c:98-124: an empty file is an error, an early end a warning and a fake EOI */
  stdio_src *s = (stdio_src *)cinfo->src;
  size_t n = fread(s->buffer, 1, INPUT_BUF_SIZE, s->infile);
  if (n == 0) {
    if (s->start_of_file) ERREXIT(cinfo, JERR_INPUT_EMPTY);
    WARNMS(cinfo, JWRN_JPEG_EOF);
    s->buffer[0] = (JOCTET)0xFF; s->buffer[1] = (JOCTET)JPEG_EOI;
    n = 2;
  }
  s->pub.next_input_byte = s->buffer;
  s->pub.bytes_in_buffer = n;
  s->start_of_file = FALSE;
  return TRUE;
}
static void any_skip(j_decompress_ptr cinfo, long num_bytes)
{ /* skip_input_data jdatasrc.c:169-190 */
  struct jpeg_source_mgr *s = cinfo->src;
  if (num_bytes <= 0) return;
  while (num_bytes > (long)s->bytes_in_buffer) {
    num_bytes -= (long)s->bytes_in_buffer;
    (void)(*s->fill_input_buffer) (cinfo);
  }
  s->next_input_byte += (size_t)num_bytes;
  s->bytes_in_buffer -= (size_t)num_bytes;
}
static void any_term(j_decompress_ptr cinfo) { (void)cinfo; }

void jpeg_stdio_src(j_decompress_ptr cinfo, FILE *infile)
{ /* jdatasrc.c:214-246 */
  stdio_src *s;
  if (cinfo->src == NULL) {
    cinfo->src = (struct jpeg_source_mgr *)(*cinfo->mem->alloc_small) ((j_common_ptr)cinfo, JPOOL_PERMANENT, sizeof(stdio_src));
    s = (stdio_src *)cinfo->src;
    s->buffer = (JOCTET *)(*cinfo->mem->alloc_small) ((j_common_ptr)cinfo, JPOOL_PERMANENT, INPUT_BUF_SIZE * sizeof(JOCTET));
  } else if (cinfo->src->init_source != stdio_init_source)
    ERREXIT(cinfo, JERR_BUFFER_SIZE);       /* a source of another kind cannot be reused */
  s = (stdio_src *)cinfo->src;
  s->pub.init_source = stdio_init_source;
  s->pub.fill_input_buffer = stdio_fill;
  s->pub.skip_input_data = any_skip;
  s->pub.resync_to_restart = jpeg_resync_to_restart;
  s->pub.term_source = any_term;
  s->infile = infile;
  s->pub.bytes_in_buffer = 0;
  s->pub.next_input_byte = NULL;
}

static void mem_init_source(j_decompress_ptr cinfo) { (void)cinfo; }
static boolean mem_fill(j_decompress_ptr cinfo)
{ /* fill_mem_input_buffer jdatasrc.c:127-147: the buffer was the whole file */
  static const JOCTET fake[4] = { (JOCTET)0xFF, (JOCTET)JPEG_EOI, 0, 0 };
  WARNMS(cinfo, JWRN_JPEG_EOF);
  cinfo->src->next_input_byte = fake;
  cinfo->src->bytes_in_buffer = 2;
  return TRUE;
}

void jpeg_mem_src(j_decompress_ptr cinfo, const unsigned char *inbuffer, unsigned long insize)
{ /* jdatasrc.c:255-289 */
  struct jpeg_source_mgr *s;
  if (inbuffer == NULL || insize == 0) ERREXIT(cinfo, JERR_INPUT_EMPTY);
  if (cinfo->src == NULL)
    cinfo->src = (struct jpeg_source_mgr *)(*cinfo->mem->alloc_small) ((j_common_ptr)cinfo, JPOOL_PERMANENT, sizeof(struct jpeg_source_mgr));
  else if (cinfo->src->init_source != mem_init_source)
    ERREXIT(cinfo, JERR_BUFFER_SIZE);
  s = cinfo->src;
  s->init_source = mem_init_source;
  s->fill_input_buffer = mem_fill;
  s->skip_input_data = any_skip;
  s->resync_to_restart = jpeg_resync_to_restart;
  s->term_source = any_term;
  s->bytes_in_buffer = (size_t)insize;
  s->next_input_byte = (const JOCTET *)inbuffer;
}

/* =====================================================================================================================
 * marker reader -- jdmarker.c.  The source is positioned as there: a client's marker processor is called just behind the
 * marker code, in front of the length word.
 * ===================================================================================================================== */
static void next_marker(j_decompress_ptr cinfo)
{ /* next_marker jdmarker.c:889-933 */
  int c;
  for (;;) {
    c = src_byte(cinfo);
    while (c != 0xFF) { cinfo->marker->discarded_bytes++; c = src_byte(cinfo); }
    do c = src_byte(cinfo); while (c == 0xFF);
    if (c != 0) break;
    cinfo->marker->discarded_bytes += 2;      /* a stuffed zero: data, not a marker */
  }
  if (cinfo->marker->discarded_bytes != 0) {
    WARNMS2(cinfo, JWRN_EXTRANEOUS_DATA, cinfo->marker->discarded_bytes, c);
    cinfo->marker->discarded_bytes = 0;
  }
  cinfo->unread_marker = c;
}

static void get_soi(j_decompress_ptr cinfo)
{ /* get_soi jdmarker.c:201-238 */
  int i;
  TRACEMS(cinfo, 1, JTRC_SOI);
  if (cinfo->marker->saw_SOI) ERREXIT(cinfo, JERR_SOI_DUPLICATE);
  for (i = 0; i < NUM_ARITH_TBLS; i++) { cinfo->arith_dc_L[i] = 0; cinfo->arith_dc_U[i] = 1; cinfo->arith_ac_K[i] = 5; }
  cinfo->restart_interval = 0;
  cinfo->jpeg_color_space = JCS_UNKNOWN;
  cinfo->CCIR601_sampling = FALSE;
  cinfo->saw_JFIF_marker = FALSE;
  cinfo->JFIF_major_version = 1; cinfo->JFIF_minor_version = 1;
  cinfo->density_unit = 0; cinfo->X_density = 1; cinfo->Y_density = 1;
  cinfo->saw_Adobe_marker = FALSE; cinfo->Adobe_transform = 0;
  cinfo->marker->saw_SOI = TRUE;
}

static void get_sof(j_decompress_ptr cinfo, boolean is_prog, boolean is_lossless, boolean is_arith)
{ /* get_sof jdmarker.c:241-304 */
  long length;
  int ci, c;
  jpeg_component_info *comp;
  if (cinfo->marker->saw_SOF) ERREXIT(cinfo, JERR_SOF_DUPLICATE);
  cinfo->progressive_mode = is_prog;
  cinfo->master->lossless = is_lossless;
  cinfo->arith_code = is_arith;
  length = src_2bytes(cinfo);
  cinfo->data_precision = src_byte(cinfo);
  cinfo->image_height = (JDIMENSION)src_2bytes(cinfo);
  cinfo->image_width = (JDIMENSION)src_2bytes(cinfo);
  cinfo->num_components = src_byte(cinfo);
  length -= 8;
  TRACEMS4(cinfo, 1, JTRC_SOF, cinfo->unread_marker, (int)cinfo->image_width, (int)cinfo->image_height, cinfo->num_components);
  if (cinfo->image_height <= 0 || cinfo->image_width <= 0 || cinfo->num_components <= 0) ERREXIT(cinfo, JERR_EMPTY_IMAGE);
  if (length != (long)cinfo->num_components * 3) ERREXIT(cinfo, JERR_BAD_LENGTH);
  if (cinfo->comp_info == NULL)
    cinfo->comp_info = (jpeg_component_info *)(*cinfo->mem->alloc_small) ((j_common_ptr)cinfo, JPOOL_IMAGE, cinfo->num_components * sizeof(jpeg_component_info));
  for (ci = 0, comp = cinfo->comp_info; ci < cinfo->num_components; ci++, comp++) {
    memset(comp, 0, sizeof(*comp));
    comp->component_index = ci;
    comp->component_id = src_byte(cinfo);
    c = src_byte(cinfo);
    comp->h_samp_factor = (c >> 4) & 15;
    comp->v_samp_factor = c & 15;
    comp->quant_tbl_no = src_byte(cinfo);
    TRACEMS4(cinfo, 1, JTRC_SOF_COMPONENT, comp->component_id, comp->h_samp_factor, comp->v_samp_factor, comp->quant_tbl_no);
  }
  cinfo->marker->saw_SOF = TRUE;
}

static void get_sos(j_decompress_ptr cinfo)
{ /* get_sos jdmarker.c:307-385 */
  long length;
  int i, ci, n, c, cc, pi;
  jpeg_component_info *comp = NULL;
  if (!cinfo->marker->saw_SOF) ERREXIT(cinfo, JERR_SOS_NO_SOF);
  length = src_2bytes(cinfo);
  n = src_byte(cinfo);
  TRACEMS1(cinfo, 1, JTRC_SOS, n);
  if (length != (long)(n * 2 + 6) || n < 1 || n > MAX_COMPS_IN_SCAN) ERREXIT(cinfo, JERR_BAD_LENGTH);
  cinfo->comps_in_scan = n;
  for (i = 0; i < MAX_COMPS_IN_SCAN; i++) cinfo->cur_comp_info[i] = NULL;
  for (i = 0; i < n; i++) {
    cc = src_byte(cinfo);
    c = src_byte(cinfo);
    for (ci = 0, comp = cinfo->comp_info; ci < cinfo->num_components && ci < MAX_COMPS_IN_SCAN; ci++, comp++)
      if (cc == comp->component_id && !cinfo->cur_comp_info[ci]) break;
    if (ci >= cinfo->num_components || ci >= MAX_COMPS_IN_SCAN) ERREXIT1(cinfo, JERR_BAD_COMPONENT_ID, cc);
    cinfo->cur_comp_info[i] = comp;
    comp->dc_tbl_no = (c >> 4) & 15;
    comp->ac_tbl_no = c & 15;
    TRACEMS3(cinfo, 1, JTRC_SOS_COMPONENT, cc, comp->dc_tbl_no, comp->ac_tbl_no);
    for (pi = 0; pi < i; pi++)
      if (cinfo->cur_comp_info[pi] == comp) ERREXIT1(cinfo, JERR_BAD_COMPONENT_ID, cc);
  }
  cinfo->Ss = src_byte(cinfo);
  cinfo->Se = src_byte(cinfo);
  c = src_byte(cinfo);
  cinfo->Ah = (c >> 4) & 15;
  cinfo->Al = c & 15;
  TRACEMS4(cinfo, 1, JTRC_SOS_PARAMS, cinfo->Ss, cinfo->Se, cinfo->Ah, cinfo->Al);
  cinfo->marker->next_restart_num = 0;
  cinfo->input_scan_number++;
}

static void get_dac(j_decompress_ptr cinfo)
{ /* get_dac jdmarker.c:390-427 */
  long length = src_2bytes(cinfo) - 2;
  while (length > 0) {
    const int index = src_byte(cinfo), val = src_byte(cinfo);
    length -= 2;
    TRACEMS2(cinfo, 1, JTRC_DAC, index, val);
    if (index < 0 || index >= 2 * NUM_ARITH_TBLS) ERREXIT1(cinfo, JERR_DAC_INDEX, index);
    if (index >= NUM_ARITH_TBLS) cinfo->arith_ac_K[index - NUM_ARITH_TBLS] = (UINT8)val;
    else {
      cinfo->arith_dc_L[index] = (UINT8)(val & 0x0F);
      cinfo->arith_dc_U[index] = (UINT8)(val >> 4);
      if (cinfo->arith_dc_L[index] > cinfo->arith_dc_U[index]) ERREXIT1(cinfo, JERR_DAC_VALUE, val);
    }
  }
  if (length != 0) ERREXIT(cinfo, JERR_BAD_LENGTH);
}

static void get_dht(j_decompress_ptr cinfo)
{ /* get_dht jdmarker.c:436-507 */
  long length = src_2bytes(cinfo) - 2;
  UINT8 bits[17], huffval[256];
  int i, index, count;
  JHUFF_TBL **slot;
  while (length > 16) {
    index = src_byte(cinfo);
    TRACEMS1(cinfo, 1, JTRC_DHT, index);
    bits[0] = 0;
    count = 0;
    for (i = 1; i <= 16; i++) { bits[i] = (UINT8)src_byte(cinfo); count += bits[i]; }
    length -= 1 + 16;
    TRACEMS8(cinfo, 2, JTRC_HUFFBITS, bits[1], bits[2], bits[3], bits[4], bits[5], bits[6], bits[7], bits[8]);
    TRACEMS8(cinfo, 2, JTRC_HUFFBITS, bits[9], bits[10], bits[11], bits[12], bits[13], bits[14], bits[15], bits[16]);
    if (count > 256 || (long)count > length) ERREXIT(cinfo, JERR_BAD_HUFF_TABLE);
    memset(huffval, 0, sizeof(huffval));
    for (i = 0; i < count; i++) huffval[i] = (UINT8)src_byte(cinfo);
    length -= count;
    if (index & 0x10) {
      index -= 0x10;
      if (index < 0 || index >= NUM_HUFF_TBLS) ERREXIT1(cinfo, JERR_DHT_INDEX, index);
      slot = &cinfo->ac_huff_tbl_ptrs[index];
      DM(cinfo)->ac_seen |= 1 << index;
    } else {
      if (index < 0 || index >= NUM_HUFF_TBLS) ERREXIT1(cinfo, JERR_DHT_INDEX, index);
      slot = &cinfo->dc_huff_tbl_ptrs[index];
      DM(cinfo)->dc_seen |= 1 << index;
    }
    if (*slot == NULL) *slot = jpeg_alloc_huff_table((j_common_ptr)cinfo);
    memcpy((*slot)->bits, bits, sizeof((*slot)->bits));
    memcpy((*slot)->huffval, huffval, sizeof((*slot)->huffval));
  }
  if (length != 0) ERREXIT(cinfo, JERR_BAD_LENGTH);
}

static void get_dqt(j_decompress_ptr cinfo)
{ /* get_dqt jdmarker.c:510-565 */
  long length = src_2bytes(cinfo) - 2;
  int n, i, prec;
  JQUANT_TBL *q;
  while (length > 0) {
    n = src_byte(cinfo);
    prec = n >> 4;
    n &= 0x0F;
    TRACEMS2(cinfo, 1, JTRC_DQT, n, prec);
    if (n >= NUM_QUANT_TBLS) ERREXIT1(cinfo, JERR_DQT_INDEX, n);
    if (cinfo->quant_tbl_ptrs[n] == NULL) cinfo->quant_tbl_ptrs[n] = jpeg_alloc_quant_table((j_common_ptr)cinfo);
    q = cinfo->quant_tbl_ptrs[n];
    for (i = 0; i < DCTSIZE2; i++) q->quantval[jpeg_natural_order[i]] = (UINT16)(prec ? src_2bytes(cinfo) : src_byte(cinfo));
    DM(cinfo)->q_seen |= 1 << n;
    if (cinfo->err->trace_level >= 2)
      for (i = 0; i < DCTSIZE2; i += 8)
        TRACEMS8(cinfo, 2, JTRC_QUANTVALS, q->quantval[i], q->quantval[i + 1], q->quantval[i + 2], q->quantval[i + 3],
                 q->quantval[i + 4], q->quantval[i + 5], q->quantval[i + 6], q->quantval[i + 7]);
    length -= DCTSIZE2 + 1;
    if (prec) length -= DCTSIZE2;
  }
  if (length != 0) ERREXIT(cinfo, JERR_BAD_LENGTH);
}

static void get_dri(j_decompress_ptr cinfo)
{ /* get_dri jdmarker.c:568-589 */
  unsigned int tmp;
  if (src_2bytes(cinfo) != 4) ERREXIT(cinfo, JERR_BAD_LENGTH);
  tmp = (unsigned int)src_2bytes(cinfo);
  TRACEMS1(cinfo, 1, JTRC_DRI, tmp);
  cinfo->restart_interval = tmp;
}

/* The decoder's marker walk guesses the colour space from APP0 / APP14 as default_decompress_parms does, so a segment this
 * reader recognised goes into the rebuilt file -- its examined bytes alone, never a thumbnail. */
static void examine_app0(j_decompress_ptr cinfo, const JOCTET *data, unsigned int datalen, long remaining)
{ /* examine_app0 jdmarker.c:604-674 */
  long totallen = (long)datalen + remaining;
  if (datalen >= APP0_DATA_LEN && data[0] == 0x4A && data[1] == 0x46 && data[2] == 0x49 && data[3] == 0x46 && data[4] == 0) {
    static const unsigned char head[4] = { 0xFF, M_APP0, 0, 16 };
    cinfo->saw_JFIF_marker = TRUE;
    cinfo->JFIF_major_version = data[5];
    cinfo->JFIF_minor_version = data[6];
    cinfo->density_unit = data[7];
    cinfo->X_density = (UINT16)((data[8] << 8) + data[9]);
    cinfo->Y_density = (UINT16)((data[10] << 8) + data[11]);
    if (cinfo->JFIF_major_version != 1) WARNMS2(cinfo, JWRN_JFIF_MAJOR, cinfo->JFIF_major_version, cinfo->JFIF_minor_version);
    TRACEMS5(cinfo, 1, JTRC_JFIF, cinfo->JFIF_major_version, cinfo->JFIF_minor_version, cinfo->X_density, cinfo->Y_density, cinfo->density_unit);
    if (data[12] | data[13]) TRACEMS2(cinfo, 1, JTRC_JFIF_THUMBNAIL, data[12], data[13]);
    totallen -= APP0_DATA_LEN;
    if (totallen != (long)data[12] * (long)data[13] * 3L) TRACEMS1(cinfo, 1, JTRC_JFIF_BADTHUMBNAILSIZE, (int)totallen);
    file_put(cinfo, head, 4);
    file_put(cinfo, data, 12);
    file_put1(cinfo, 0); file_put1(cinfo, 0);
  } else if (datalen >= 6 && data[0] == 0x4A && data[1] == 0x46 && data[2] == 0x58 && data[3] == 0x58 && data[4] == 0) {
    switch (data[5]) {
    case 0x10: TRACEMS1(cinfo, 1, JTRC_THUMB_JPEG, (int)totallen); break;
    case 0x11: TRACEMS1(cinfo, 1, JTRC_THUMB_PALETTE, (int)totallen); break;
    case 0x13: TRACEMS1(cinfo, 1, JTRC_THUMB_RGB, (int)totallen); break;
    default: TRACEMS2(cinfo, 1, JTRC_JFIF_EXTENSION, data[5], (int)totallen); break;
    }
  } else
    TRACEMS1(cinfo, 1, JTRC_APP0, (int)totallen);
}

static void examine_app14(j_decompress_ptr cinfo, const JOCTET *data, unsigned int datalen, long remaining)
{ /* examine_app14 jdmarker.c:677-705 */
  if (datalen >= APP14_DATA_LEN && data[0] == 0x41 && data[1] == 0x64 && data[2] == 0x6F && data[3] == 0x62 && data[4] == 0x65) {
    static const unsigned char head[4] = { 0xFF, M_APP14, 0, 14 };
    const unsigned int version = (data[5] << 8) + data[6], flags0 = (data[7] << 8) + data[8], flags1 = (data[9] << 8) + data[10], transform = data[11];
    TRACEMS4(cinfo, 1, JTRC_ADOBE, version, flags0, flags1, transform);
    cinfo->saw_Adobe_marker = TRUE;
    cinfo->Adobe_transform = (UINT8)transform;
    file_put(cinfo, head, 4);
    file_put(cinfo, data, 12);
  } else
    TRACEMS1(cinfo, 1, JTRC_APP14, (int)(datalen + remaining));
}

/* COM / APPn as the library handles them: saved up to the limit jpeg_save_markers set (save_marker jdmarker.c:756-855), else
 * looked at (APP0 / APP14, get_interesting_appn :708-751) or skipped (skip_variable :860-877) */
static void library_marker(j_decompress_ptr cinfo, int slot)
{
  const int code = cinfo->unread_marker;
  unsigned int limit = DK(cinfo)->limit[slot];
  long length = src_2bytes(cinfo) - 2;
  unsigned int i;
  if (limit > 0) {
    jpeg_saved_marker_ptr cur = NULL;
    JOCTET *data = NULL;
    unsigned int data_length = 0;
    if (length >= 0) {
      if ((unsigned int)length < limit) limit = (unsigned int)length;
      cur = (jpeg_saved_marker_ptr)(*cinfo->mem->alloc_large) ((j_common_ptr)cinfo, JPOOL_IMAGE, sizeof(struct jpeg_marker_struct) + limit);
      cur->next = NULL;
      cur->marker = (UINT8)code;
      cur->original_length = (unsigned int)length;
      cur->data_length = data_length = limit;
      data = cur->data = (JOCTET *)(cur + 1);
      for (i = 0; i < limit; i++) data[i] = (JOCTET)src_byte(cinfo);
      if (cinfo->marker_list == NULL || cinfo->master->marker_list_end == NULL) cinfo->marker_list = cinfo->master->marker_list_end = cur;
      else { cinfo->master->marker_list_end->next = cur; cinfo->master->marker_list_end = cur; }
      length = (long)cur->original_length - (long)data_length;
    }
    if (code == M_APP0) examine_app0(cinfo, data, data_length, length);
    else if (code == M_APP14) examine_app14(cinfo, data, data_length, length);
    else TRACEMS2(cinfo, 1, JTRC_MISC_MARKER, code, (int)(data_length + length));
  } else if (code == M_APP0 || code == M_APP14) {
    JOCTET b[APPN_DATA_LEN];
    const unsigned int numtoread = length >= APPN_DATA_LEN ? APPN_DATA_LEN : (length > 0 ? (unsigned int)length : 0);
    for (i = 0; i < numtoread; i++) b[i] = (JOCTET)src_byte(cinfo);
    length -= numtoread;
    if (code == M_APP0) examine_app0(cinfo, b, numtoread, length);
    else examine_app14(cinfo, b, numtoread, length);
  } else
    TRACEMS2(cinfo, 1, JTRC_MISC_MARKER, code, (int)length);
  if (length > 0) (*cinfo->src->skip_input_data) (cinfo, length);
}

/* a segment the decoder's marker walk reads: recorded byte for byte while this reader parses it */
#define RECORDED(cinfo, stmt) do { file_put1(cinfo, 0xFF); file_put1(cinfo, (cinfo)->unread_marker); DM(cinfo)->recording = 1; stmt; DM(cinfo)->recording = 0; } while (0)

static int read_markers(j_decompress_ptr cinfo)
{ /* read_markers jdmarker.c:967-1121: up to and including an SOS header, or EOI */
  for (;;) {
    if (cinfo->unread_marker == 0) {
      if (!cinfo->marker->saw_SOI) {
        const int c = src_byte(cinfo), c2 = src_byte(cinfo);       /* first_marker: no garbage in front of SOI */
        if (c != 0xFF || c2 != M_SOI) ERREXIT2(cinfo, JERR_NO_SOI, c, c2);
        cinfo->unread_marker = c2;
      } else
        next_marker(cinfo);
    }
    switch (cinfo->unread_marker) {
    case M_SOI: get_soi(cinfo); break;
    case M_SOF0: case M_SOF1: RECORDED(cinfo, get_sof(cinfo, FALSE, FALSE, FALSE)); break;
    case M_SOF2: RECORDED(cinfo, get_sof(cinfo, TRUE, FALSE, FALSE)); break;
    case M_SOF3: RECORDED(cinfo, get_sof(cinfo, FALSE, TRUE, FALSE)); break;
    case M_SOF9: RECORDED(cinfo, get_sof(cinfo, FALSE, FALSE, TRUE)); break;
    case M_SOF10: RECORDED(cinfo, get_sof(cinfo, TRUE, FALSE, TRUE)); break;
    case M_SOF11: RECORDED(cinfo, get_sof(cinfo, FALSE, TRUE, TRUE)); break;
    case 0xC5: case 0xC6: case 0xC7: case M_JPG: case 0xCD: case 0xCE: case 0xCF:
      ERREXIT1(cinfo, JERR_SOF_UNSUPPORTED, cinfo->unread_marker);
      break;
    case M_SOS:
      RECORDED(cinfo, get_sos(cinfo));
      cinfo->unread_marker = 0;
      return JPEG_REACHED_SOS;
    case M_EOI:
      TRACEMS(cinfo, 1, JTRC_EOI);
      cinfo->unread_marker = 0;
      return JPEG_REACHED_EOI;
    case M_DAC: RECORDED(cinfo, get_dac(cinfo)); break;
    case M_DHT: RECORDED(cinfo, get_dht(cinfo)); break;
    case M_DQT: RECORDED(cinfo, get_dqt(cinfo)); break;
    case M_DRI: RECORDED(cinfo, get_dri(cinfo)); break;
    case M_COM:
      if (DK(cinfo)->client[16]) { if (!(*DK(cinfo)->client[16]) (cinfo)) ERREXIT(cinfo, JERR_CANT_SUSPEND); }
      else library_marker(cinfo, 16);
      break;
    case M_DNL: {                /* the reference skips it; the decoder's walk refuses such a file, so it has to see it */
      long length;
      RECORDED(cinfo, { length = src_2bytes(cinfo) - 2; TRACEMS2(cinfo, 1, JTRC_MISC_MARKER, cinfo->unread_marker, (int)length); while (length-- > 0) (void)src_byte(cinfo); });
      break;
    }
    case M_TEM:
      TRACEMS1(cinfo, 1, JTRC_PARMLESS_MARKER, cinfo->unread_marker);
      break;
    default:
      if (cinfo->unread_marker >= M_APP0 && cinfo->unread_marker <= M_APP15) {
        const int slot = cinfo->unread_marker - M_APP0;
        if (DK(cinfo)->client[slot]) { if (!(*DK(cinfo)->client[slot]) (cinfo)) ERREXIT(cinfo, JERR_CANT_SUSPEND); }
        else library_marker(cinfo, slot);
      } else if (cinfo->unread_marker >= M_RST0 && cinfo->unread_marker <= M_RST7)
        TRACEMS1(cinfo, 1, JTRC_PARMLESS_MARKER, cinfo->unread_marker);
      else
        ERREXIT1(cinfo, JERR_UNKNOWN_MARKER, cinfo->unread_marker);
      break;
    }
    cinfo->unread_marker = 0;
  }
}

static boolean read_restart_marker(j_decompress_ptr cinfo)
{ /* read_restart_marker jdmarker.c:1136-1163 (exported through cinfo->marker; the device decoder does not come here) */
  if (cinfo->unread_marker == 0) next_marker(cinfo);
  if (cinfo->unread_marker == M_RST0 + cinfo->marker->next_restart_num) {
    TRACEMS1(cinfo, 3, JTRC_RST, cinfo->marker->next_restart_num);
    cinfo->unread_marker = 0;
  } else if (!(*cinfo->src->resync_to_restart) (cinfo, cinfo->marker->next_restart_num))
    return FALSE;
  cinfo->marker->next_restart_num = (cinfo->marker->next_restart_num + 1) & 7;
  return TRUE;
}

boolean jpeg_resync_to_restart(j_decompress_ptr cinfo, int desired)
{ /* jdmarker.c:1214-1262 */
  int marker = cinfo->unread_marker, action;
  WARNMS2(cinfo, JWRN_MUST_RESYNC, marker, desired);
  for (;;) {
    if (marker < M_SOF0) action = 2;                              /* no marker at all: move on */
    else if (marker < M_RST0 || marker > M_RST7) action = 3;      /* another marker: leave it to the caller */
    else if (marker == M_RST0 + ((desired + 1) & 7) || marker == M_RST0 + ((desired + 2) & 7)) action = 3;
    else if (marker == M_RST0 + ((desired - 1) & 7) || marker == M_RST0 + ((desired - 2) & 7)) action = 2;
    else action = 1;
    TRACEMS2(cinfo, 4, JTRC_RECOVERY_ACTION, marker, action);
    if (action == 1) { cinfo->unread_marker = 0; return TRUE; }
    if (action == 3) return TRUE;
    next_marker(cinfo);
    marker = cinfo->unread_marker;
  }
}

static void reset_marker_reader(j_decompress_ptr cinfo)
{ /* reset_marker_reader jdmarker.c:1269-1283 */
  cinfo->comp_info = NULL;
  cinfo->input_scan_number = 0;
  cinfo->unread_marker = 0;
  cinfo->marker->saw_SOI = FALSE;
  cinfo->marker->saw_SOF = FALSE;
  cinfo->marker->discarded_bytes = 0;
}

void jpeg_save_markers(j_decompress_ptr cinfo, int marker_code, unsigned int length_limit)
{ /* jdmarker.c:1325-1370 */
  const long maxlength = cinfo->mem->max_alloc_chunk - (long)sizeof(struct jpeg_marker_struct);
  int slot;
  if ((long)length_limit > maxlength) length_limit = (unsigned int)maxlength;
  if (length_limit) {      /* APP0 / APP14: at least what the library itself looks at */
    if (marker_code == M_APP0 && length_limit < APP0_DATA_LEN) length_limit = APP0_DATA_LEN;
    else if (marker_code == M_APP14 && length_limit < APP14_DATA_LEN) length_limit = APP14_DATA_LEN;
  }
  if (marker_code == M_COM) slot = 16;
  else if (marker_code >= M_APP0 && marker_code <= M_APP15) slot = marker_code - M_APP0;
  else { ERREXIT1(cinfo, JERR_UNKNOWN_MARKER, marker_code); return; }
  DK(cinfo)->client[slot] = NULL;
  DK(cinfo)->limit[slot] = length_limit;
}

void jpeg_set_marker_processor(j_decompress_ptr cinfo, int marker_code, jpeg_marker_parser_method routine)
{ /* jdmarker.c:1379-1391 */
  if (marker_code == M_COM) DK(cinfo)->client[16] = routine;
  else if (marker_code >= M_APP0 && marker_code <= M_APP15) DK(cinfo)->client[marker_code - M_APP0] = routine;
  else ERREXIT1(cinfo, JERR_UNKNOWN_MARKER, marker_code);
}

/* ---- ICC profiles -- jdicc.c ------------------------------------------------------------------------------------------ */
#define ICC_OVERHEAD_LEN 14
static int marker_is_icc(jpeg_saved_marker_ptr m)
{
  return m->marker == M_APP0 + 2 && m->data_length >= ICC_OVERHEAD_LEN && memcmp(m->data, "ICC_PROFILE", 12) == 0;
}

boolean jpeg_read_icc_profile(j_decompress_ptr cinfo, JOCTET **icc_data_ptr, unsigned int *icc_data_len)
{ /* jdicc.c:69-167: the APP2 "ICC_PROFILE" segments of marker_list put together by their sequence numbers */
  jpeg_saved_marker_ptr m;
  int num_markers = 0, seq;
  unsigned int total = 0, length[256], offset[256];
  char present[256];
  JOCTET *icc;
  if (icc_data_ptr == NULL || icc_data_len == NULL) ERREXIT(cinfo, JERR_BUFFER_SIZE);
  if (cinfo->global_state < DSTATE_READY) ERREXIT1(cinfo, JERR_BAD_STATE, cinfo->global_state);
  *icc_data_ptr = NULL;
  *icc_data_len = 0;
  memset(present, 0, sizeof(present));
  for (m = cinfo->marker_list; m != NULL; m = m->next) {
    if (!marker_is_icc(m)) continue;
    if (num_markers == 0) num_markers = m->data[13];
    else if (num_markers != m->data[13]) { WARNMS(cinfo, JWRN_BOGUS_ICC); return FALSE; }
    seq = m->data[12];
    if (seq <= 0 || seq > num_markers || present[seq]) { WARNMS(cinfo, JWRN_BOGUS_ICC); return FALSE; }
    present[seq] = 1;
    length[seq] = m->data_length - ICC_OVERHEAD_LEN;
  }
  if (num_markers == 0) return FALSE;
  for (seq = 1; seq <= num_markers; seq++) {
    if (!present[seq]) { WARNMS(cinfo, JWRN_BOGUS_ICC); return FALSE; }
    offset[seq] = total;
    total += length[seq];
  }
  if (total == 0) { WARNMS(cinfo, JWRN_BOGUS_ICC); return FALSE; }
  icc = (JOCTET *)malloc(total);
  if (icc == NULL) ERREXIT1(cinfo, JERR_OUT_OF_MEMORY, 11);
  for (m = cinfo->marker_list; m != NULL; m = m->next)
    if (marker_is_icc(m)) memcpy(icc + offset[m->data[12]], m->data + ICC_OVERHEAD_LEN, length[m->data[12]]);
  *icc_data_ptr = icc;
  *icc_data_len = total;
  return TRUE;
}

/* =====================================================================================================================
 * object life cycle and header -- jdapimin.c, jdinput.c
 * ===================================================================================================================== */
static int input_not_here(j_decompress_ptr cinfo) { refuse(cinfo, "the input controller's methods are not part of this library (jpeg_read_header / jpeg_start_decompress read the datastream)"); return 0; }
static void input_reset(j_decompress_ptr cinfo)
{ /* reset_input_controller jdinput.c:360-377 */
  cinfo->inputctl->has_multiple_scans = FALSE;
  cinfo->inputctl->eoi_reached = FALSE;
  (*cinfo->err->reset_error_mgr) ((j_common_ptr)cinfo);
  (*cinfo->marker->reset_marker_reader) (cinfo);
  cinfo->coef_bits = NULL;
}
static void input_nop(j_decompress_ptr cinfo) { (void)cinfo; }

void jpeg_CreateDecompress(j_decompress_ptr cinfo, int version, size_t structsize)
{ /* jdapimin.c:35-99 */
  int i;
  cinfo->mem = NULL;
  if (version != JPEG_LIB_VERSION) ERREXIT2(cinfo, JERR_BAD_LIB_VERSION, JPEG_LIB_VERSION, version);
  if (structsize != sizeof(struct jpeg_decompress_struct))
    ERREXIT2(cinfo, JERR_BAD_STRUCT_SIZE, (int)sizeof(struct jpeg_decompress_struct), (int)structsize);
  {
    struct jpeg_error_mgr *err = cinfo->err;
    void *client_data = cinfo->client_data;
    memset(cinfo, 0, sizeof(struct jpeg_decompress_struct));
    cinfo->err = err;
    cinfo->client_data = client_data;
  }
  cinfo->is_decompressor = TRUE;
  jinit_memory_mgr((j_common_ptr)cinfo);
  /* the marker reader (jinit_marker_reader jdmarker.c:1290-1318): COM and APPn are skipped, APP0 / APP14 looked at */
  cinfo->marker = (struct jpeg_marker_reader *)(*cinfo->mem->alloc_small) ((j_common_ptr)cinfo, JPOOL_PERMANENT, sizeof(d_marker));
  memset(cinfo->marker, 0, sizeof(d_marker));
  cinfo->marker->reset_marker_reader = reset_marker_reader;
  cinfo->marker->read_markers = read_markers;
  cinfo->marker->read_restart_marker = read_restart_marker;
  reset_marker_reader(cinfo);
  /* the input controller (jinit_input_controller jdinput.c:384-404): its state variables are the public part */
  cinfo->inputctl = (struct jpeg_input_controller *)(*cinfo->mem->alloc_small) ((j_common_ptr)cinfo, JPOOL_PERMANENT, sizeof(struct jpeg_input_controller));
  memset(cinfo->inputctl, 0, sizeof(struct jpeg_input_controller));
  cinfo->inputctl->consume_input = input_not_here;
  cinfo->inputctl->reset_input_controller = input_reset;
  cinfo->inputctl->start_input_pass = input_nop;
  cinfo->inputctl->finish_input_pass = input_nop;
  for (i = 0; i < NUM_QUANT_TBLS; i++) cinfo->quant_tbl_ptrs[i] = NULL;
  cinfo->data_precision = BITS_IN_JSAMPLE;
  cinfo->global_state = DSTATE_START;
  cinfo->master = (struct jpeg_decomp_master *)(*cinfo->mem->alloc_small) ((j_common_ptr)cinfo, JPOOL_PERMANENT, sizeof(d_master));
  memset(cinfo->master, 0, sizeof(d_master));
}

void jpeg_destroy_decompress(j_decompress_ptr cinfo) { jpeg_destroy((j_common_ptr)cinfo); }   /* jdapimin.c:106-110 */
void jpeg_abort_decompress(j_decompress_ptr cinfo) { jpeg_abort((j_common_ptr)cinfo); }       /* jdapimin.c:118-122 */

static void default_decompress_parms(j_decompress_ptr cinfo)
{ /* default_decompress_parms jdapimin.c:129-236 */
  switch (cinfo->num_components) {
  case 1:
    cinfo->jpeg_color_space = JCS_GRAYSCALE;
    cinfo->out_color_space = JCS_GRAYSCALE;
    break;
  case 3:
    if (cinfo->saw_JFIF_marker) cinfo->jpeg_color_space = JCS_YCbCr;
    else if (cinfo->saw_Adobe_marker) {
      if (cinfo->Adobe_transform == 0) cinfo->jpeg_color_space = JCS_RGB;
      else {
        if (cinfo->Adobe_transform != 1) WARNMS1(cinfo, JWRN_ADOBE_XFORM, cinfo->Adobe_transform);
        cinfo->jpeg_color_space = JCS_YCbCr;
      }
    } else {
      const int cid0 = cinfo->comp_info[0].component_id, cid1 = cinfo->comp_info[1].component_id, cid2 = cinfo->comp_info[2].component_id;
      if (cid0 == 1 && cid1 == 2 && cid2 == 3) cinfo->jpeg_color_space = cinfo->master->lossless ? JCS_RGB : JCS_YCbCr;
      else if (cid0 == 82 && cid1 == 71 && cid2 == 66) cinfo->jpeg_color_space = JCS_RGB;
      else {
        TRACEMS3(cinfo, 1, JTRC_UNKNOWN_IDS, cid0, cid1, cid2);
        cinfo->jpeg_color_space = cinfo->master->lossless ? JCS_RGB : JCS_YCbCr;
      }
    }
    cinfo->out_color_space = JCS_RGB;
    break;
  case 4:
    if (cinfo->saw_Adobe_marker) {
      if (cinfo->Adobe_transform == 0) cinfo->jpeg_color_space = JCS_CMYK;
      else {
        if (cinfo->Adobe_transform != 2) WARNMS1(cinfo, JWRN_ADOBE_XFORM, cinfo->Adobe_transform);
        cinfo->jpeg_color_space = JCS_YCCK;
      }
    } else cinfo->jpeg_color_space = JCS_CMYK;
    cinfo->out_color_space = JCS_CMYK;
    break;
  default:
    cinfo->jpeg_color_space = JCS_UNKNOWN;
    cinfo->out_color_space = JCS_UNKNOWN;
    break;
  }
  cinfo->scale_num = 1;
  cinfo->scale_denom = 1;
  cinfo->output_gamma = 1.0;
  cinfo->buffered_image = FALSE;
  cinfo->raw_data_out = FALSE;
  cinfo->dct_method = JDCT_DEFAULT;
  cinfo->do_fancy_upsampling = TRUE;
  cinfo->do_block_smoothing = TRUE;
  cinfo->quantize_colors = FALSE;
  cinfo->dither_mode = JDITHER_FS;
  cinfo->two_pass_quantize = TRUE;
  cinfo->desired_number_of_colors = 256;
  cinfo->colormap = NULL;
  cinfo->enable_1pass_quant = FALSE;
  cinfo->enable_external_quant = FALSE;
  cinfo->enable_2pass_quant = FALSE;
}

static void initial_setup(j_decompress_ptr cinfo)
{ /* initial_setup jdinput.c:43-135, as far as it fills public fields */
  int ci;
  jpeg_component_info *comp;
  if ((long)cinfo->image_height > (long)JPEG_MAX_DIMENSION || (long)cinfo->image_width > (long)JPEG_MAX_DIMENSION)
    ERREXIT1(cinfo, JERR_IMAGE_TOO_BIG, (unsigned int)JPEG_MAX_DIMENSION);
  if (cinfo->num_components > MAX_COMPONENTS) ERREXIT2(cinfo, JERR_COMPONENT_COUNT, cinfo->num_components, MAX_COMPONENTS);
  cinfo->max_h_samp_factor = 1;
  cinfo->max_v_samp_factor = 1;
  for (ci = 0, comp = cinfo->comp_info; ci < cinfo->num_components; ci++, comp++) {
    if (comp->h_samp_factor <= 0 || comp->h_samp_factor > MAX_SAMP_FACTOR || comp->v_samp_factor <= 0 || comp->v_samp_factor > MAX_SAMP_FACTOR)
      ERREXIT(cinfo, JERR_BAD_SAMPLING);
    if (comp->h_samp_factor > cinfo->max_h_samp_factor) cinfo->max_h_samp_factor = comp->h_samp_factor;
    if (comp->v_samp_factor > cinfo->max_v_samp_factor) cinfo->max_v_samp_factor = comp->v_samp_factor;
  }
  cinfo->min_DCT_scaled_size = DCTSIZE;
  for (ci = 0, comp = cinfo->comp_info; ci < cinfo->num_components; ci++, comp++) {
    comp->DCT_scaled_size = DCTSIZE;
    comp->width_in_blocks = (JDIMENSION)jdiv_round_up((long)cinfo->image_width * comp->h_samp_factor, (long)cinfo->max_h_samp_factor * DCTSIZE);
    comp->height_in_blocks = (JDIMENSION)jdiv_round_up((long)cinfo->image_height * comp->v_samp_factor, (long)cinfo->max_v_samp_factor * DCTSIZE);
    comp->downsampled_width = (JDIMENSION)jdiv_round_up((long)cinfo->image_width * comp->h_samp_factor, (long)cinfo->max_h_samp_factor);
    comp->downsampled_height = (JDIMENSION)jdiv_round_up((long)cinfo->image_height * comp->v_samp_factor, (long)cinfo->max_v_samp_factor);
    comp->component_needed = TRUE;
    comp->quant_table = NULL;
  }
  cinfo->total_iMCU_rows = (JDIMENSION)jdiv_round_up((long)cinfo->image_height, (long)cinfo->max_v_samp_factor * DCTSIZE);
  cinfo->inputctl->has_multiple_scans = (cinfo->comps_in_scan < cinfo->num_components || cinfo->progressive_mode) ? TRUE : FALSE;
}

int jpeg_read_header(j_decompress_ptr cinfo, boolean require_image)
{ /* jdapimin.c:266-297 with the DSTATE_START / DSTATE_INHEADER half of jpeg_consume_input (:312-352) */
  d_master *m = DM(cinfo);
  static const unsigned char soi[2] = { 0xFF, M_SOI };
  if (cinfo->global_state != DSTATE_START && cinfo->global_state != DSTATE_INHEADER) ERREXIT1(cinfo, JERR_BAD_STATE, cinfo->global_state);
  if (cinfo->global_state == DSTATE_START) {
    (*cinfo->inputctl->reset_input_controller) (cinfo);
    (*cinfo->src->init_source) (cinfo);
    cinfo->global_state = DSTATE_INHEADER;
  }
  m->file_len = 0; m->recording = 0; m->q_seen = m->dc_seen = m->ac_seen = 0; m->eof_seen = 0;
  file_put(cinfo, soi, 2);
  if (read_markers(cinfo) == JPEG_REACHED_EOI) {
    cinfo->inputctl->eoi_reached = TRUE;
    if (require_image) ERREXIT(cinfo, JERR_NO_IMAGE);
    jpeg_abort((j_common_ptr)cinfo);            /* a tables-only datastream: the tables stay in the object */
    return JPEG_HEADER_TABLES_ONLY;
  }
  initial_setup(cinfo);
  default_decompress_parms(cinfo);
  cinfo->global_state = DSTATE_READY;
  /* the sources the device decoder has no path for (mjh_jpeg_probe's list) */
  if (cinfo->progressive_mode) refuse(cinfo, "progressive JPEG files are not decoded on the GPU path (no CPU fallback)");
  if (cinfo->arith_code) refuse(cinfo, "arithmetic-coded JPEG files are not decoded on the GPU path (no CPU fallback)");
  if (cinfo->master->lossless) refuse(cinfo, "lossless JPEG files are not decoded on the GPU path (no CPU fallback)");
  if (cinfo->data_precision != 8) refuse(cinfo, "12-bit JPEG files are not decoded on the GPU path (no CPU fallback)");
  if (cinfo->num_components != 1 && cinfo->num_components != 3 && cinfo->num_components != 4) refuse(cinfo, "JPEG files of 2 components are not decoded on the GPU path (no CPU fallback)");
  return JPEG_HEADER_OK;
}

boolean jpeg_input_complete(j_decompress_ptr cinfo)
{ /* jdapimin.c:359-367 */
  if (cinfo->global_state < DSTATE_START || cinfo->global_state > DSTATE_STOPPING) ERREXIT1(cinfo, JERR_BAD_STATE, cinfo->global_state);
  return cinfo->inputctl->eoi_reached;
}

boolean jpeg_has_multiple_scans(j_decompress_ptr cinfo)
{ /* jdapimin.c:374-382 */
  if (cinfo->global_state < DSTATE_READY || cinfo->global_state > DSTATE_STOPPING) ERREXIT1(cinfo, JERR_BAD_STATE, cinfo->global_state);
  return cinfo->inputctl->has_multiple_scans;
}

/* =====================================================================================================================
 * output dimensions -- jdmaster.c
 * ===================================================================================================================== */
/* red, green, blue offsets and pixel size of the RGB family (jmorecfg.h:332-358); 0: not of it */
static int rgb_layout(J_COLOR_SPACE cs, int off[3])
{
  static const signed char t[10][4] = { { 0, 1, 2, 3 }, { 0, 1, 2, 4 }, { 2, 1, 0, 3 }, { 2, 1, 0, 4 }, { 3, 2, 1, 4 }, { 1, 2, 3, 4 },
                                        { 0, 1, 2, 4 }, { 2, 1, 0, 4 }, { 3, 2, 1, 4 }, { 1, 2, 3, 4 } };
  int i = -1;
  if (cs == JCS_RGB) i = 0;
  else if ((int)cs >= (int)JCS_EXT_RGB && (int)cs <= (int)JCS_EXT_ARGB) i = (int)cs - (int)JCS_EXT_RGB;
  if (i < 0) return 0;
  off[0] = t[i][0]; off[1] = t[i][1]; off[2] = t[i][2];
  return t[i][3];
}

static boolean use_merged_upsample(j_decompress_ptr cinfo)
{ /* use_merged_upsample jdmaster.c:38-85: only rec_outbuf_height depends on it here */
  int off[3], px;
  if (cinfo->master->lossless || cinfo->do_fancy_upsampling || cinfo->CCIR601_sampling) return FALSE;
  if (cinfo->jpeg_color_space != JCS_YCbCr || cinfo->num_components != 3) return FALSE;
  px = cinfo->out_color_space == JCS_RGB565 ? 3 : rgb_layout(cinfo->out_color_space, off);
  if (px == 0 || cinfo->out_color_components != px) return FALSE;
  if (cinfo->comp_info[0].h_samp_factor != 2 || cinfo->comp_info[1].h_samp_factor != 1 || cinfo->comp_info[2].h_samp_factor != 1 ||
      cinfo->comp_info[0].v_samp_factor > 2 || cinfo->comp_info[1].v_samp_factor != 1 || cinfo->comp_info[2].v_samp_factor != 1)
    return FALSE;
  if (cinfo->comp_info[0].DCT_scaled_size != cinfo->min_DCT_scaled_size || cinfo->comp_info[1].DCT_scaled_size != cinfo->min_DCT_scaled_size ||
      cinfo->comp_info[2].DCT_scaled_size != cinfo->min_DCT_scaled_size)
    return FALSE;
  return TRUE;
}

static void calc_output_dimensions(j_decompress_ptr cinfo)
{ /* jpeg_core_output_dimensions jdmaster.c:99-235 + jpeg_calc_output_dimensions :265-377 */
  int ci, k = 1, off[3];
  jpeg_component_info *comp;
  while (k < 16 && (long)cinfo->scale_num * DCTSIZE > (long)cinfo->scale_denom * k) k++;
  cinfo->output_width = (JDIMENSION)jdiv_round_up((long)cinfo->image_width * k, (long)DCTSIZE);
  cinfo->output_height = (JDIMENSION)jdiv_round_up((long)cinfo->image_height * k, (long)DCTSIZE);
  cinfo->min_DCT_scaled_size = k;
  for (ci = 0, comp = cinfo->comp_info; ci < cinfo->num_components; ci++, comp++) {
    int ssize = k;
    while (ssize < DCTSIZE && (cinfo->max_h_samp_factor * k) % (comp->h_samp_factor * ssize * 2) == 0 &&
           (cinfo->max_v_samp_factor * k) % (comp->v_samp_factor * ssize * 2) == 0)
      ssize *= 2;
    comp->DCT_scaled_size = ssize;
    comp->downsampled_width = (JDIMENSION)jdiv_round_up((long)cinfo->image_width * (long)(comp->h_samp_factor * ssize), (long)(cinfo->max_h_samp_factor * DCTSIZE));
    comp->downsampled_height = (JDIMENSION)jdiv_round_up((long)cinfo->image_height * (long)(comp->v_samp_factor * ssize), (long)(cinfo->max_v_samp_factor * DCTSIZE));
  }
  switch (cinfo->out_color_space) {
  case JCS_GRAYSCALE: cinfo->out_color_components = 1; break;
  case JCS_YCbCr: case JCS_RGB565: cinfo->out_color_components = 3; break;
  case JCS_CMYK: case JCS_YCCK: cinfo->out_color_components = 4; break;
  default:
    cinfo->out_color_components = rgb_layout(cinfo->out_color_space, off);
    if (cinfo->out_color_components == 0) cinfo->out_color_components = cinfo->num_components;
    break;
  }
  cinfo->output_components = cinfo->quantize_colors ? 1 : cinfo->out_color_components;
  cinfo->rec_outbuf_height = use_merged_upsample(cinfo) ? cinfo->max_v_samp_factor : 1;
}

void jpeg_calc_output_dimensions(j_decompress_ptr cinfo)
{
  if (cinfo->global_state != DSTATE_READY) ERREXIT1(cinfo, JERR_BAD_STATE, cinfo->global_state);
  calc_output_dimensions(cinfo);
}

/* =====================================================================================================================
 * jpeg_start_decompress: the rest of the datastream, one call of the device decoder, the pixels to host memory
 * ===================================================================================================================== */
/* the segments of tables the object kept from earlier datastreams and this one did not define (an abbreviated image), put
 * behind SOI: whatever the file defines later replaces them for the decoder's marker walk as it does in the object */
static void put_kept_tables(j_decompress_ptr cinfo, unsigned char *dst, size_t *n)
{
  d_master *m = DM(cinfo);
  int t, k, is_ac;
  size_t p = 0;
  for (t = 0; t < NUM_QUANT_TBLS; t++) {
    const JQUANT_TBL *q = cinfo->quant_tbl_ptrs[t];
    int wide = 0;
    if (q == NULL || (m->q_seen >> t & 1)) continue;
    for (k = 0; k < DCTSIZE2; k++) if (q->quantval[k] > 255) wide = 1;
    dst[p++] = 0xFF; dst[p++] = M_DQT; dst[p++] = 0; dst[p++] = (unsigned char)(3 + DCTSIZE2 * (wide ? 2 : 1));
    dst[p++] = (unsigned char)((wide << 4) | t);
    for (k = 0; k < DCTSIZE2; k++) {
      const unsigned v = q->quantval[jpeg_natural_order[k]];
      if (wide) dst[p++] = (unsigned char)(v >> 8);
      dst[p++] = (unsigned char)(v & 0xFF);
    }
  }
  for (is_ac = 0; is_ac < 2; is_ac++)
    for (t = 0; t < NUM_HUFF_TBLS; t++) {
      const JHUFF_TBL *h = is_ac ? cinfo->ac_huff_tbl_ptrs[t] : cinfo->dc_huff_tbl_ptrs[t];
      int count = 0;
      if (h == NULL || ((is_ac ? m->ac_seen : m->dc_seen) >> t & 1)) continue;
      for (k = 1; k <= 16; k++) count += h->bits[k];
      if (count > 256) ERREXIT(cinfo, JERR_BAD_HUFF_TABLE);
      dst[p++] = 0xFF; dst[p++] = M_DHT; dst[p++] = (unsigned char)((19 + count) >> 8); dst[p++] = (unsigned char)((19 + count) & 0xFF);
      dst[p++] = (unsigned char)((is_ac << 4) | t);
      for (k = 1; k <= 16; k++) dst[p++] = h->bits[k];
      memcpy(dst + p, h->huffval, (size_t)count);
      p += (size_t)count;
    }
  *n = p;
}

/* latch_quant_tables jdinput.c:233-260: the components of the scan that starts keep a copy of their table as it is NOW */
static void latch_quant_tables(j_decompress_ptr cinfo)
{
  int ci;
  for (ci = 0; ci < cinfo->comps_in_scan; ci++) {
    jpeg_component_info *comp = cinfo->cur_comp_info[ci];
    const int qn = comp->quant_tbl_no;
    if (comp->quant_table != NULL) continue;
    if (qn < 0 || qn >= NUM_QUANT_TBLS || cinfo->quant_tbl_ptrs[qn] == NULL) ERREXIT1(cinfo, JERR_NO_QUANT_TABLE, qn);
    comp->quant_table = (JQUANT_TBL *)(*cinfo->mem->alloc_small) ((j_common_ptr)cinfo, JPOOL_IMAGE, sizeof(JQUANT_TBL));
    memcpy(comp->quant_table, cinfo->quant_tbl_ptrs[qn], sizeof(JQUANT_TBL));
  }
}

/* from behind an SOS header to EOI: entropy-coded data in whole runs, the segments between scans through read_markers */
static void read_to_eoi(j_decompress_ptr cinfo)
{
  struct jpeg_source_mgr *s = cinfo->src;
  for (;;) {
    const JOCTET *ff;
    int c;
    if (s->bytes_in_buffer == 0) src_fill(cinfo);
    ff = (const JOCTET *)memchr(s->next_input_byte, 0xFF, s->bytes_in_buffer);
    if (ff == NULL) {
      file_put(cinfo, s->next_input_byte, s->bytes_in_buffer);
      s->next_input_byte += s->bytes_in_buffer; s->bytes_in_buffer = 0;
      continue;
    }
    file_put(cinfo, s->next_input_byte, (size_t)(ff - s->next_input_byte));
    s->bytes_in_buffer -= (size_t)(ff - s->next_input_byte) + 1;
    s->next_input_byte = ff + 1;
    do c = src_byte(cinfo); while (c == 0xFF);           /* (fill bytes in front of a marker are dropped) */
    if (c == 0 || (c >= M_RST0 && c <= M_RST7)) { file_put1(cinfo, 0xFF); file_put1(cinfo, c); continue; }
    cinfo->unread_marker = c;
    if (read_markers(cinfo) == JPEG_REACHED_EOI) break;
    cinfo->inputctl->has_multiple_scans = TRUE;
    if (DM(cinfo)->latching) latch_quant_tables(cinfo);
  }
  file_put1(cinfo, 0xFF); file_put1(cinfo, M_EOI);
  cinfo->inputctl->eoi_reached = TRUE;
}

static void decoder_failed(j_decompress_ptr cinfo, int rc, int damaged)
{
  const int eof = DM(cinfo)->eof_seen;
  fprintf(stderr, "mozjpeg_hip: %s\n", mjh_last_error());
  mjh_dapi_drop(cinfo);
  if (rc == MJH_EUNSUPPORTED) ERREXIT(cinfo, JERR_NOT_COMPILED);
  if (eof) ERREXIT(cinfo, JERR_INPUT_EOF);
  if (damaged) ERREXIT(cinfo, JWRN_HUFF_BAD_CODE);        /* fatal here; the reference warns and goes on */
  if (rc == MJH_EINVAL) ERREXIT(cinfo, JERR_BAD_LENGTH);  /* the marker walk found a malformed header */
  ERREXIT1(cinfo, JERR_OUT_OF_MEMORY, 0);
}

/* What jpeg_start_decompress and jpeg_read_coefficients share: the tables the file may leave out, the rest of the datastream
 * through the source manager, an encoder leased for the frame, ONE file decoded with the call's options and waited for.  The
 * lease (DM(cinfo)->enc) is the caller's to end. */
static void decode_file(j_decompress_ptr cinfo, const mjh_decode_opts *opts)
{
  d_master *m = DM(cinfo);
  mjh_jpeg_info *info;
  mjh_params *p;
  int ci, rc;
  double t0 = 0.0, t1;
  /* slots 0 and 1 without a table get the standard ones (std_huff_tables from jinit_huff_decoder jdhuff.c:816-823: Motion JPEG
   * frames come without DHT); an abbreviated image then carries them like every other kept table */
  for (ci = 0; ci < 4; ci++) {
    JHUFF_TBL **slot = (ci & 1) ? &cinfo->ac_huff_tbl_ptrs[ci >> 1] : &cinfo->dc_huff_tbl_ptrs[ci >> 1];
    const uint8_t *bits, *vals;
    int n;
    if (*slot != NULL) continue;
    *slot = jpeg_alloc_huff_table((j_common_ptr)cinfo);
    mjh_std_huffman_table(ci & 1, ci >> 1, &bits, &vals, &n);
    memcpy((*slot)->bits, bits, 17);
    memset((*slot)->huffval, 0, sizeof((*slot)->huffval));
    memcpy((*slot)->huffval, vals, (size_t)n);
  }
  /* the tables the frame and its first scan name must exist by now (latch_quant_tables jdinput.c, start_pass jdhuff.c) */
  for (ci = 0; ci < cinfo->num_components; ci++) {
    const int qn = cinfo->comp_info[ci].quant_tbl_no;
    if (qn < 0 || qn >= NUM_QUANT_TBLS || cinfo->quant_tbl_ptrs[qn] == NULL) ERREXIT1(cinfo, JERR_NO_QUANT_TABLE, qn);
  }
  for (ci = 0; ci < cinfo->comps_in_scan; ci++) {
    const int dc = cinfo->cur_comp_info[ci]->dc_tbl_no, ac = cinfo->cur_comp_info[ci]->ac_tbl_no;
    if (dc < 0 || dc >= NUM_HUFF_TBLS || cinfo->dc_huff_tbl_ptrs[dc] == NULL) ERREXIT1(cinfo, JERR_NO_HUFF_TABLE, dc);
    if (ac < 0 || ac >= NUM_HUFF_TBLS || cinfo->ac_huff_tbl_ptrs[ac] == NULL) ERREXIT1(cinfo, JERR_NO_HUFF_TABLE, ac);
  }
  {   /* an abbreviated image: the kept tables go in behind SOI */
    unsigned char kept[NUM_QUANT_TBLS * 133 + 2 * NUM_HUFF_TBLS * 277];
    size_t n = 0;
    put_kept_tables(cinfo, kept, &n);
    if (n) {
      file_put(cinfo, kept, n);                              /* (grows the buffer) */
      memmove(m->file + 2 + n, m->file + 2, m->file_len - n - 2);
      memcpy(m->file + 2, kept, n);
    }
  }
  if (d_timing) t0 = d_now();
  read_to_eoi(cinfo);
  if (d_timing) { t1 = d_now(); d_acc(0, t1 - t0, 0); t0 = t1; }
  info = (mjh_jpeg_info *)malloc(sizeof(*info) + sizeof(*p));
  if (info == NULL) ERREXIT1(cinfo, JERR_OUT_OF_MEMORY, 9);
  p = (mjh_params *)(info + 1);
  rc = mjh_jpeg_probe(m->file, m->file_len, info);
  if (rc == MJH_OK) rc = mjh_params_from_jpeg(info, MJH_PROFILE_FASTEST, p);
  if (rc == MJH_OK && (m->enc = mjh_shim_cache_acquire(p)) == NULL) rc = MJH_EUNSUPPORTED;
  free(info);
  if (rc != MJH_OK) decoder_failed(cinfo, rc, 0);
  if (d_timing) { t1 = d_now(); d_acc(1, t1 - t0, 0); t0 = t1; }
  {
    const void *files[1];
    size_t sizes[1];
    files[0] = m->file; sizes[0] = m->file_len;
    rc = mjh_decode_host(m->enc, files, sizes, 1, opts);
    if (rc != MJH_OK) decoder_failed(cinfo, rc, 0);
    rc = mjh_decode_wait(m->enc);
    if (rc != MJH_OK) decoder_failed(cinfo, rc, 1);
  }
  if (d_timing) { t1 = d_now(); d_acc(2, t1 - t0, 0); t0 = t1; }
}

static int regions_enabled(void)
{
  const char *v = getenv("MOZJPEG_HIP_REGIONS");
  return v && v[0] == '1' && v[1] == 0;
}

/* The GPU call jpeg_start_decompress left open (MOZJPEG_HIP_REGIONS=1): the columns jpeg_crop_scanline named, at full height --
 * jpeg_skip_scanlines only moves over rows of the image this makes. */
static void decode_pending(j_decompress_ptr cinfo)
{
  d_master *m = DM(cinfo);
  mjh_decode_opts o;
  int rc;
  if (!m->pending) return;
  m->pending = 0;
  o = m->opts;
  if (m->crop_w) { o.crop_x = (int)m->crop_x; o.crop_w = (int)m->crop_w; }
  decode_file(cinfo, &o);
  m->row_bytes = (size_t)cinfo->output_width * (size_t)m->px;
  m->pixels = (unsigned char *)malloc(m->row_bytes * cinfo->output_height);
  if (m->pixels == NULL) { mjh_dapi_drop(cinfo); ERREXIT1(cinfo, JERR_OUT_OF_MEMORY, 10); }
  rc = mjh_get_pixels(m->enc, 0, m->pixels, m->row_bytes);
  if (rc != MJH_OK) decoder_failed(cinfo, rc, 0);
  mjh_shim_cache_release(m->enc);
  m->enc = NULL;
  free(m->file); m->file = NULL; m->file_len = m->file_cap = 0;
}

boolean jpeg_start_decompress(j_decompress_ptr cinfo)
{
  d_master *m = DM(cinfo);
  mjh_decode_opts o;
  int ci, k, rc, off[3], px, every;
  double t0 = 0.0;
  if (cinfo->global_state != DSTATE_READY) ERREXIT1(cinfo, JERR_BAD_STATE, cinfo->global_state);
  if (cinfo->buffered_image) refuse(cinfo, "buffered-image mode is not built (the GPU path decodes a whole file at once)");
  if (cinfo->quantize_colors) refuse(cinfo, "colour quantization (djpeg -gif / -colors / -map) is not built on the GPU path (no CPU fallback)");
  if (cinfo->dct_method != JDCT_ISLOW && cinfo->dct_method != JDCT_IFAST) refuse(cinfo, "the float inverse DCT (djpeg -dct float) is not built on the GPU path (no CPU fallback)");
  calc_output_dimensions(cinfo);
  k = cinfo->min_DCT_scaled_size;
  /* MOZJPEG_HIP_ALL_SCALES=1: every size of jidctint.c decodes (mjh_decode_opts.all_scales); read here, per file, not at load */
  {
    const char *v = getenv("MOZJPEG_HIP_ALL_SCALES");
    every = v && v[0] == '1' && v[1] == 0;
  }
  if (!every && k != 1 && k != 2 && k != 4 && k != 8) {
    char why[160];
    snprintf(why, sizeof(why), "scale %u/%u decodes with the %dx%d inverse DCT; the sizes built on the GPU path are 1x1, 2x2, 4x4 and 8x8", cinfo->scale_num, cinfo->scale_denom, k, k);
    refuse(cinfo, why);
  }
  mjh_decode_opts_defaults(&o);
  o.scale_num = k; o.scale_denom = 8;
  o.all_scales = every;
  o.dct_method = cinfo->dct_method == JDCT_IFAST ? 1 : 0;
  o.fancy_upsampling = cinfo->do_fancy_upsampling ? 1 : 0;
  px = 0;
  if (cinfo->raw_data_out) {
    for (ci = 0; ci < cinfo->num_components; ci++)
      if (cinfo->comp_info[ci].DCT_scaled_size != k) refuse(cinfo, "raw_data_out with a scale at which the components are transformed at different sizes is not built on the GPU path");
    o.raw_planes = 1;
  } else if (cinfo->num_components == 4 || cinfo->out_color_space == JCS_CMYK) {
    /* jinit_color_deconverter jdcolor.c:901-918: CMYK from a CMYK file (null_convert) or a YCCK file (ycck_cmyk_convert), and
     * nothing else from either; JCS_CMYK from no other file (djpeg's writers turn the four samples into RGB, wrppm.c cmyk_to_rgb) */
    if (cinfo->out_color_space != JCS_CMYK || (cinfo->jpeg_color_space != JCS_CMYK && cinfo->jpeg_color_space != JCS_YCCK)) ERREXIT(cinfo, JERR_CONVERSION_NOTIMPL);
    o.out_color_space = MJH_CS_CMYK; px = 4; o.pixel_size = 4;
  } else if (cinfo->out_color_space == JCS_GRAYSCALE) {
    if (cinfo->jpeg_color_space != JCS_GRAYSCALE && cinfo->jpeg_color_space != JCS_YCbCr && cinfo->jpeg_color_space != JCS_RGB) ERREXIT(cinfo, JERR_CONVERSION_NOTIMPL);
    o.out_color_space = MJH_CS_GRAYSCALE; px = 1;
  } else if (cinfo->out_color_space == JCS_RGB565) {
    o.out_color_space = MJH_CS_RGB565; px = 2;
    o.rgb_offset[0] = o.rgb_offset[1] = o.rgb_offset[2] = 0;
    o.no_dither = cinfo->dither_mode == JDITHER_NONE;
  } else if ((px = rgb_layout(cinfo->out_color_space, off)) != 0) {
    o.out_color_space = MJH_CS_RGB; o.pixel_size = px;
    o.rgb_offset[0] = off[0]; o.rgb_offset[1] = off[1]; o.rgb_offset[2] = off[2];
  } else
    ERREXIT(cinfo, JERR_CONVERSION_NOTIMPL);              /* JCS_YCbCr, JCS_YCCK */
  /* MOZJPEG_HIP_REGIONS=1 (read here, per file): pixels of a one- or three-component file wait for the first row to be asked
   * for; without the variable nothing moves and the decode stays inside this call */
  if (regions_enabled() && !cinfo->raw_data_out && cinfo->num_components != 4) {
    m->pending = 1; m->px = px; m->opts = o; m->crop_x = m->crop_w = 0;
    (*cinfo->mem->realize_virt_arrays) ((j_common_ptr)cinfo);
    cinfo->output_scanline = 0;
    cinfo->output_scan_number = cinfo->input_scan_number;
    cinfo->global_state = DSTATE_SCANNING;
    return TRUE;
  }
  decode_file(cinfo, &o);
  if (d_timing) t0 = d_now();
  if (cinfo->raw_data_out) {
    for (ci = 0; ci < cinfo->num_components; ci++) {
      m->plane_w[ci] = (size_t)cinfo->comp_info[ci].width_in_blocks * (size_t)k;
      m->plane_h[ci] = (size_t)cinfo->comp_info[ci].height_in_blocks * (size_t)k;
      m->planes[ci] = (unsigned char *)malloc(m->plane_w[ci] * m->plane_h[ci]);
      if (m->planes[ci] == NULL) { mjh_dapi_drop(cinfo); ERREXIT1(cinfo, JERR_OUT_OF_MEMORY, 10); }
      rc = mjh_get_plane(m->enc, 0, ci, m->planes[ci], m->plane_w[ci], (int)m->plane_w[ci], (int)m->plane_h[ci]);
      if (rc != MJH_OK) decoder_failed(cinfo, rc, 0);
    }
  } else {
    m->row_bytes = (size_t)cinfo->output_width * (size_t)px;
    m->pixels = (unsigned char *)malloc(m->row_bytes * cinfo->output_height);
    if (m->pixels == NULL) { mjh_dapi_drop(cinfo); ERREXIT1(cinfo, JERR_OUT_OF_MEMORY, 10); }
    rc = mjh_get_pixels(m->enc, 0, m->pixels, m->row_bytes);
    if (rc != MJH_OK) decoder_failed(cinfo, rc, 0);
  }
  if (d_timing) d_acc(3, d_now() - t0, 1);
  mjh_shim_cache_release(m->enc);                             /* the lease ends here: the image is the object's own now */
  m->enc = NULL;
  free(m->file); m->file = NULL; m->file_len = m->file_cap = 0;
  (*cinfo->mem->realize_virt_arrays) ((j_common_ptr)cinfo);   /* the client's own (wrbmp.c keeps the image in one), as master_selection does */
  cinfo->output_scanline = 0;
  cinfo->output_scan_number = cinfo->input_scan_number;
  cinfo->global_state = cinfo->raw_data_out ? DSTATE_RAW_OK : DSTATE_SCANNING;
  return TRUE;
}

JDIMENSION jpeg_read_scanlines(j_decompress_ptr cinfo, JSAMPARRAY scanlines, JDIMENSION max_lines)
{ /* jdapistd.c:279-314; every row asked for that the image still has is delivered in one call */
  d_master *m = DM(cinfo);
  JDIMENSION n, left;
  if (cinfo->global_state != DSTATE_SCANNING) ERREXIT1(cinfo, JERR_BAD_STATE, cinfo->global_state);
  if (cinfo->output_scanline >= cinfo->output_height) { WARNMS(cinfo, JWRN_TOO_MUCH_DATA); return 0; }
  if (cinfo->progress != NULL) {
    cinfo->progress->pass_counter = (long)cinfo->output_scanline;
    cinfo->progress->pass_limit = (long)cinfo->output_height;
    (*cinfo->progress->progress_monitor) ((j_common_ptr)cinfo);
  }
  left = cinfo->output_height - cinfo->output_scanline;
  if (max_lines > left) max_lines = left;
  decode_pending(cinfo);
  if (d_timing) {
    const double t0 = d_now();
    for (n = 0; n < max_lines; n++) memcpy(scanlines[n], m->pixels + (size_t)(cinfo->output_scanline + n) * m->row_bytes, m->row_bytes);
    d_acc(4, d_now() - t0, 0);
  } else
    for (n = 0; n < max_lines; n++) memcpy(scanlines[n], m->pixels + (size_t)(cinfo->output_scanline + n) * m->row_bytes, m->row_bytes);
  cinfo->output_scanline += max_lines;
  return max_lines;
}

JDIMENSION jpeg_read_raw_data(j_decompress_ptr cinfo, JSAMPIMAGE data, JDIMENSION max_lines)
{ /* jdapistd.c:589-626: one iMCU row; the samples of real blocks, the rest of the client's buffer stays as it is */
  d_master *m = DM(cinfo);
  JDIMENSION lines, imcu;
  int ci;
  if (cinfo->global_state != DSTATE_RAW_OK) ERREXIT1(cinfo, JERR_BAD_STATE, cinfo->global_state);
  if (cinfo->output_scanline >= cinfo->output_height) { WARNMS(cinfo, JWRN_TOO_MUCH_DATA); return 0; }
  if (cinfo->progress != NULL) {
    cinfo->progress->pass_counter = (long)cinfo->output_scanline;
    cinfo->progress->pass_limit = (long)cinfo->output_height;
    (*cinfo->progress->progress_monitor) ((j_common_ptr)cinfo);
  }
  lines = (JDIMENSION)(cinfo->max_v_samp_factor * cinfo->min_DCT_scaled_size);
  if (max_lines < lines) ERREXIT(cinfo, JERR_BUFFER_SIZE);
  imcu = cinfo->output_scanline / lines;
  for (ci = 0; ci < cinfo->num_components; ci++) {
    const size_t rows = (size_t)cinfo->comp_info[ci].v_samp_factor * (size_t)cinfo->min_DCT_scaled_size;
    size_t r;
    for (r = 0; r < rows; r++) {
      const size_t y = (size_t)imcu * rows + r;
      if (y < m->plane_h[ci]) memcpy(data[ci][r], m->planes[ci] + y * m->plane_w[ci], m->plane_w[ci]);
    }
  }
  cinfo->output_scanline += lines;
  return lines;
}

/* =====================================================================================================================
 * jpeg_read_coefficients -- jdtrans.c: the same call of the device decoder, stopped after the Huffman decoder
 * ===================================================================================================================== */
jvirt_barray_ptr *jpeg_read_coefficients(j_decompress_ptr cinfo)
{ /* jdtrans.c:48-95 + transdecode_master_selection :103-161; the full-buffer case of jinit_d_coef_controller jdcoefct.c:834-860 */
  d_master *m = DM(cinfo);
  if (cinfo->master->lossless) ERREXIT(cinfo, JERR_NOTIMPL);
  if (cinfo->global_state == DSTATE_READY) {
    mjh_decode_opts o;
    jpeg_component_info *comp;
    int ci, rc;
    cinfo->buffered_image = TRUE;               /* "this is effectively a buffered-image operation" */
    m->coef_arrays = (jvirt_barray_ptr *)(*cinfo->mem->alloc_small) ((j_common_ptr)cinfo, JPOOL_IMAGE, sizeof(jvirt_barray_ptr) * MAX_COMPONENTS);
    for (ci = 0, comp = cinfo->comp_info; ci < cinfo->num_components; ci++, comp++)
      m->coef_arrays[ci] = (*cinfo->mem->request_virt_barray) ((j_common_ptr)cinfo, JPOOL_IMAGE, TRUE,
                                                               (JDIMENSION)jround_up((long)comp->width_in_blocks, (long)comp->h_samp_factor),
                                                               (JDIMENSION)jround_up((long)comp->height_in_blocks, (long)comp->v_samp_factor),
                                                               (JDIMENSION)comp->v_samp_factor);
    (*cinfo->mem->realize_virt_arrays) ((j_common_ptr)cinfo);     /* these and the client's own (jtransform_request_workspace) */
    if (cinfo->progress != NULL) {
      cinfo->progress->pass_counter = 0L;
      cinfo->progress->pass_limit = (long)cinfo->total_iMCU_rows * (cinfo->inputctl->has_multiple_scans ? cinfo->num_components : 1);
      cinfo->progress->completed_passes = 0;
      cinfo->progress->total_passes = 1;
      (*cinfo->progress->progress_monitor) ((j_common_ptr)cinfo);
    }
    m->latching = 1;
    latch_quant_tables(cinfo);                  /* the first scan's header was read by jpeg_read_header */
    mjh_decode_opts_defaults(&o);
    o.raw_coefs = 1;
    decode_file(cinfo, &o);
    m->latching = 0;
    for (ci = 0, comp = cinfo->comp_info; ci < cinfo->num_components; ci++, comp++) {
      /* the real blocks row by row; the rows and columns of padding are the pre-zeroed array's */
      const size_t row_bytes = (size_t)comp->width_in_blocks * sizeof(JBLOCK);
      JDIMENSION r;
      unsigned char *tmp = (unsigned char *)malloc(row_bytes * comp->height_in_blocks);
      if (tmp == NULL) { mjh_dapi_drop(cinfo); ERREXIT1(cinfo, JERR_OUT_OF_MEMORY, 11); }
      rc = mjh_get_coefs(m->enc, 0, ci, tmp, comp->width_in_blocks);
      if (rc != MJH_OK) { free(tmp); decoder_failed(cinfo, rc, 0); }
      for (r = 0; r < (JDIMENSION)jround_up((long)comp->height_in_blocks, (long)comp->v_samp_factor); r++) {
        JBLOCKARRAY ba = (*cinfo->mem->access_virt_barray) ((j_common_ptr)cinfo, m->coef_arrays[ci], r, 1, TRUE);
        if (r < comp->height_in_blocks) memcpy(ba[0], tmp + (size_t)r * row_bytes, row_bytes);
      }
      free(tmp);
    }
    mjh_shim_cache_release(m->enc);
    m->enc = NULL;
    free(m->file); m->file = NULL; m->file_len = m->file_cap = 0;
    if (cinfo->progress != NULL) {
      cinfo->progress->pass_counter = cinfo->progress->pass_limit;
      (*cinfo->progress->progress_monitor) ((j_common_ptr)cinfo);
    }
    cinfo->global_state = DSTATE_STOPPING;      /* so that jpeg_finish_decompress does the right thing */
  }
  if (cinfo->global_state == DSTATE_STOPPING && cinfo->buffered_image && m->coef_arrays != NULL) return m->coef_arrays;
  ERREXIT1(cinfo, JERR_BAD_STATE, cinfo->global_state);
  return NULL;
}

boolean jpeg_finish_decompress(j_decompress_ptr cinfo)
{ /* jdapimin.c:394-425: the datastream was read up to EOI by jpeg_start_decompress, so the source stands just behind it */
  if (cinfo->global_state == DSTATE_SCANNING || cinfo->global_state == DSTATE_RAW_OK) {
    if (cinfo->output_scanline < cinfo->output_height) ERREXIT(cinfo, JERR_TOO_LITTLE_DATA);
    decode_pending(cinfo);                      /* (a client that skipped every row: the datastream is still read and decoded) */
    cinfo->global_state = DSTATE_STOPPING;
  } else if (cinfo->global_state != DSTATE_STOPPING)
    ERREXIT1(cinfo, JERR_BAD_STATE, cinfo->global_state);
  (*cinfo->src->term_source) (cinfo);
  jpeg_abort((j_common_ptr)cinfo);
  return TRUE;
}

/* =====================================================================================================================
 * entry points that exist because clients name them (djpeg is linked with immediate binding) and raise JERR_NOT_COMPILED
 * ===================================================================================================================== */
#define NOT_BUILT(what) refuse(cinfo, what " is not built on the GPU path (no CPU fallback)")
/* Partial decompression, with MOZJPEG_HIP_REGIONS=1 in the environment (without it both raise JERR_NOT_COMPILED as they always
 * did: that refusal is part of the tested contract).
 * jpeg_crop_scanline, jdapistd.c:185-300: its checks in its order, *xoffset moved left to a multiple of the iMCU column width,
 * *width grown by as much, output_width set; a second call names new columns of the image (not of the first crop), checked
 * against the width the first one left, as there. */
void jpeg_crop_scanline(j_decompress_ptr cinfo, JDIMENSION *xoffset, JDIMENSION *width)
{
  d_master *m = DM(cinfo);
  JDIMENSION input_xoffset;
  int align;
  if (!regions_enabled()) NOT_BUILT("jpeg_crop_scanline (djpeg -crop)");
  if (cinfo->data_precision != 8) ERREXIT1(cinfo, JERR_BAD_PRECISION, cinfo->data_precision);
  if (cinfo->master->lossless) ERREXIT(cinfo, JERR_NOTIMPL);
  if ((cinfo->global_state != DSTATE_SCANNING && cinfo->global_state != DSTATE_BUFIMAGE) || cinfo->output_scanline != 0) ERREXIT1(cinfo, JERR_BAD_STATE, cinfo->global_state);
  if (!xoffset || !width) ERREXIT(cinfo, JERR_BAD_CROP_SPEC);
  if (*width == 0 || (unsigned long long)(*xoffset) + *width > cinfo->output_width) ERREXIT(cinfo, JERR_WIDTH_OVERFLOW);
  if (*width == cinfo->output_width) return;
  if (!m->pending) refuse(cinfo, "jpeg_crop_scanline on an image that was decoded whole (MOZJPEG_HIP_REGIONS was not set at jpeg_start_decompress, or the file has four components)");
  align = (cinfo->comps_in_scan == 1 && cinfo->num_components == 1) ? cinfo->min_DCT_scaled_size : cinfo->min_DCT_scaled_size * cinfo->max_h_samp_factor;
  input_xoffset = *xoffset;
  *xoffset = (input_xoffset / (JDIMENSION)align) * (JDIMENSION)align;
  *width = *width + input_xoffset - *xoffset;
  cinfo->output_width = *width;
  m->crop_x = *xoffset; m->crop_w = *width;
}

/* jpeg_skip_scanlines, jdapistd.c:470-660: its checks and return values; skipping changes no value, so it only moves over rows
 * of the image the GPU call makes (the columns at full height) */
JDIMENSION jpeg_skip_scanlines(j_decompress_ptr cinfo, JDIMENSION num_lines)
{
  if (!regions_enabled()) NOT_BUILT("jpeg_skip_scanlines (djpeg -skip)");
  if (cinfo->data_precision != 8) ERREXIT1(cinfo, JERR_BAD_PRECISION, cinfo->data_precision);
  if (cinfo->master->lossless) ERREXIT(cinfo, JERR_NOTIMPL);
  if (cinfo->quantize_colors && cinfo->two_pass_quantize) ERREXIT(cinfo, JERR_NOTIMPL);
  if (cinfo->global_state != DSTATE_SCANNING) ERREXIT1(cinfo, JERR_BAD_STATE, cinfo->global_state);
  if ((unsigned long long)cinfo->output_scanline + num_lines >= cinfo->output_height) {
    num_lines = cinfo->output_height - cinfo->output_scanline;
    cinfo->output_scanline = cinfo->output_height;
    return num_lines;
  }
  cinfo->output_scanline += num_lines;
  return num_lines;
}
boolean jpeg_start_output(j_decompress_ptr cinfo, int scan_number) { (void)scan_number; NOT_BUILT("jpeg_start_output (buffered-image mode)"); return FALSE; }
boolean jpeg_finish_output(j_decompress_ptr cinfo) { NOT_BUILT("jpeg_finish_output (buffered-image mode)"); return FALSE; }
int jpeg_consume_input(j_decompress_ptr cinfo) { NOT_BUILT("jpeg_consume_input"); return 0; }
void jpeg_new_colormap(j_decompress_ptr cinfo) { NOT_BUILT("jpeg_new_colormap (colour quantization)"); }
void jpeg12_crop_scanline(j_decompress_ptr cinfo, JDIMENSION *xoffset, JDIMENSION *width) { (void)xoffset; (void)width; NOT_BUILT("jpeg12_crop_scanline (12-bit files)"); }
JDIMENSION jpeg12_skip_scanlines(j_decompress_ptr cinfo, JDIMENSION num_lines) { (void)num_lines; NOT_BUILT("jpeg12_skip_scanlines (12-bit files)"); return 0; }
JDIMENSION jpeg12_read_scanlines(j_decompress_ptr cinfo, J12SAMPARRAY scanlines, JDIMENSION max_lines) { (void)scanlines; (void)max_lines; NOT_BUILT("jpeg12_read_scanlines (12-bit files)"); return 0; }
JDIMENSION jpeg12_read_raw_data(j_decompress_ptr cinfo, J12SAMPIMAGE data, JDIMENSION max_lines) { (void)data; (void)max_lines; NOT_BUILT("jpeg12_read_raw_data (12-bit files)"); return 0; }
JDIMENSION jpeg16_read_scanlines(j_decompress_ptr cinfo, J16SAMPARRAY scanlines, JDIMENSION max_lines) { (void)scanlines; (void)max_lines; NOT_BUILT("jpeg16_read_scanlines (lossless 16-bit files)"); return 0; }
