/* lossless_client.c -- a libjpeg client in lossless mode (SOF3), written against the public API only: what an application sees of
 * a compress object from image to image.  The same binary runs on the reference's libjpeg.so.62 (expected output), with the
 * interposing library in front of it, and on the stand-alone library; tests/test_gpu_lossless_client.py and
 * tests/test_simt_lossless_dropin.py compare every printed line (file hashes and the object's fields).
 *   scenario names on the command line; images are deterministic and synthetic.
 *   `lossless_client bench THREADS IMAGES_PER_THREAD WIDTH HEIGHT PSV [each]`: throughput of client threads, each with a compress
 *   object and a frame of its own (each: one scan per component, set through scan_info); tools/bench_lossless.py --through libjpeg. */
#include <pthread.h>
#include <setjmp.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "jpeglib.h"
#include "jerror.h"

static jmp_buf env;
static void my_exit(j_common_ptr cinfo)
{
  char buf[JMSG_LENGTH_MAX];
  (*cinfo->err->format_message) (cinfo, buf);
  printf("  error %d: %s\n", cinfo->err->msg_code, buf);
  longjmp(env, 1);
}

static unsigned long hash(const unsigned char *b, unsigned long n) { unsigned long h = 1469598103934665603ul, i; for (i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ul; return h; }

/* samples of `bits` bits in unsigned shorts (8 bits: in bytes) */
static void *make_image(int w, int h, int comps, int bits, int seed)
{
  const size_t n = (size_t)w * h * comps;
  unsigned short *p16 = bits > 8 ? (unsigned short *)malloc(n * 2) : NULL;
  unsigned char *p8 = bits > 8 ? NULL : (unsigned char *)malloc(n);
  unsigned s = 777u + (unsigned)seed * 7919u;
  size_t i;
  for (i = 0; i < n; i++) {
    const int x = (int)(i / comps % w), y = (int)(i / comps / w), c = (int)(i % comps);
    unsigned v;
    s = s * 1664525u + 1013904223u;
    v = (unsigned)((x * (3 + c) + y * (5 - c)) * (1 << (bits - 8)) / 2 + ((s >> 20) & ((1u << (bits - 3)) - 1u))) & ((1u << bits) - 1u);
    if (p16) p16[i] = (unsigned short)v; else p8[i] = (unsigned char)v;
  }
  return p16 ? (void *)p16 : (void *)p8;
}

static void base(struct jpeg_compress_struct *c, int w, int h, int comps)
{
  c->image_width = w; c->image_height = h; c->input_components = comps; c->in_color_space = comps == 1 ? JCS_GRAYSCALE : JCS_RGB;
  jpeg_c_set_int_param(c, JINT_COMPRESS_PROFILE, JCP_FASTEST);
  jpeg_set_defaults(c);
  c->dct_method = JDCT_ISLOW;
}

static int geometry_defined = 0;      /* a jpeg_start_compress of this scenario's object has returned */

static void fields(const char *when, struct jpeg_compress_struct *c)
{
  int ci;
  if (c->global_state != 100) geometry_defined = 1;      /* (100 = CSTATE_START: no image begun) */
  printf("  %s: state %d raw %d smooth %d jcs %d ncomp %d optimize %d arith %d progressive %d num_scans %d jfif %d adobe %d precision %d maxh %d maxv %d imcu_rows %u next %u restart %u/%d Ss %d Se %d Ah %d Al %d\n",
         when, c->global_state, c->raw_data_in, c->smoothing_factor, (int)c->jpeg_color_space, c->num_components, c->optimize_coding, c->arith_code,
         c->progressive_mode, c->num_scans, c->write_JFIF_header, c->write_Adobe_marker, c->data_precision, c->max_h_samp_factor, c->max_v_samp_factor,
         (unsigned)c->total_iMCU_rows, (unsigned)c->next_scanline, c->restart_interval, c->restart_in_rows, c->Ss, c->Se, c->Ah, c->Al);
  for (ci = 0; ci < c->num_components; ci++) {
    const jpeg_component_info *k = &c->comp_info[ci];
    printf("    comp %d: id %d h %d v %d tq %d td %d ta %d", ci, k->component_id, k->h_samp_factor, k->v_samp_factor, k->quant_tbl_no, k->dc_tbl_no, k->ac_tbl_no);
    /* (the geometry is jpeg_start_compress's to fill in: before the object's first image nothing defines it) */
    if (geometry_defined) printf(" wib %u hib %u dw %u dh %u", (unsigned)k->width_in_blocks, (unsigned)k->height_in_blocks, (unsigned)k->downsampled_width, (unsigned)k->downsampled_height);
    printf("\n");
  }
}

static void tables(const char *when, struct jpeg_compress_struct *c)
{
  int t;
  printf("  %s:", when);
  for (t = 0; t < NUM_HUFF_TBLS; t++) {
    const JHUFF_TBL *d = c->dc_huff_tbl_ptrs[t];
    if (d) printf(" dc%d sent %d bits %lx vals %lx", t, d->sent_table, hash(d->bits, 17), hash(d->huffval, 17)); else printf(" dc%d -", t);
  }
  printf("\n");
}

/* rows [from, upto), `piece` at a time */
static void rows(struct jpeg_compress_struct *c, void *img, int bits, int upto, int piece)
{
  const size_t pitch = (size_t)c->image_width * c->input_components * (bits > 8 ? 2 : 1);
  while ((int)c->next_scanline < upto) {
    void *r[8];
    int k, n = piece;
    if (n > upto - (int)c->next_scanline) n = upto - (int)c->next_scanline;
    for (k = 0; k < n; k++) r[k] = (unsigned char *)img + ((size_t)c->next_scanline + k) * pitch;
    if (bits == 16) jpeg16_write_scanlines(c, (J16SAMPARRAY)r, (JDIMENSION)n);
    else if (bits == 12) jpeg12_write_scanlines(c, (J12SAMPARRAY)r, (JDIMENSION)n);
    else jpeg_write_scanlines(c, (JSAMPARRAY)r, (JDIMENSION)n);
  }
}

static unsigned char *mem = NULL;
static unsigned long memsize = 0;
static void report(const char *what) { printf("  %s: %lu bytes %lx\n", what, memsize, hash(mem, memsize)); }

static void one_image(struct jpeg_compress_struct *c, const char *what, void *img, int bits, int piece, boolean all_tables)
{
  jpeg_start_compress(c, all_tables);
  fields(what, c);
  rows(c, img, bits, (int)c->image_height, piece);
  jpeg_finish_compress(c);
  report(what);
  tables(what, c);
}

static int passes_seen = 0, passes_total = 0;
static void monitor(j_common_ptr cinfo) { passes_seen = cinfo->progress->completed_passes; passes_total = cinfo->progress->total_passes; }

/* ---- bench: T client threads ------------------------------------------------------------------------------------------------- */
static int bT, bN, bW, bH, bPSV, bEACH;
static unsigned long long bbytes[256];
static void *bench_worker(void *arg)
{
  const int id = (int)(long)arg;
  static const jpeg_scan_info each[3] = { { 1, { 0 }, 1, 0, 0, 0 }, { 1, { 1 }, 1, 0, 0, 0 }, { 1, { 2 }, 1, 0, 0, 0 } };
  jpeg_scan_info mine[3];
  struct jpeg_compress_struct c;
  struct jpeg_error_mgr err;
  unsigned char *img = (unsigned char *)make_image(bW, bH, 3, 8, 100 + id);
  JSAMPROW *rowp = (JSAMPROW *)malloc(sizeof(JSAMPROW) * bH);
  int i, y;
  for (y = 0; y < bH; y++) rowp[y] = img + (size_t)y * bW * 3;
  for (i = 0; i < 3; i++) { mine[i] = each[i]; mine[i].Ss = bPSV; }
  c.err = jpeg_std_error(&err);
  jpeg_create_compress(&c);
  for (i = 0; i < bN; i++) {
    unsigned char *out = NULL; unsigned long n = 0;
    jpeg_mem_dest(&c, &out, &n);
    base(&c, bW, bH, 3);
    jpeg_enable_lossless(&c, bPSV, 0);
    if (bEACH) { c.scan_info = mine; c.num_scans = 3; }
    jpeg_start_compress(&c, TRUE);
    while (c.next_scanline < c.image_height) jpeg_write_scanlines(&c, rowp + c.next_scanline, c.image_height - c.next_scanline);
    jpeg_finish_compress(&c);
    bbytes[id] += n;
    free(out);
  }
  jpeg_destroy_compress(&c);
  free(rowp); free(img);
  return NULL;
}

static int bench(int argc, char **argv)
{
  pthread_t th[256];
  struct timespec t0, t1;
  unsigned long long total = 0;
  double dt;
  int round, t;
  if (argc < 7) { fprintf(stderr, "usage: lossless_client bench THREADS IMAGES_PER_THREAD WIDTH HEIGHT PSV [each]\n"); return 2; }
  bT = atoi(argv[2]); bN = atoi(argv[3]); bW = atoi(argv[4]); bH = atoi(argv[5]); bPSV = atoi(argv[6]); bEACH = argc > 7;
  if (bT < 1 || bT > 256) return 2;
  for (round = 0; round < 2; round++) {      /* the first round warms up (encoder creation, first launches) */
    memset(bbytes, 0, sizeof(bbytes));
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (t = 0; t < bT; t++) pthread_create(&th[t], NULL, bench_worker, (void *)(long)t);
    for (t = 0; t < bT; t++) pthread_join(th[t], NULL);
    clock_gettime(CLOCK_MONOTONIC, &t1);
  }
  dt = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
  for (t = 0; t < bT; t++) total += bbytes[t];
  printf("{\"threads\": %d, \"images\": %d, \"width\": %d, \"height\": %d, \"psv\": %d, \"scans\": %d, \"seconds\": %.4f, \"images_per_s\": %.2f, \"file_bytes\": %llu}\n",
         bT, bT * bN, bW, bH, bPSV, bEACH ? 3 : 1, dt, bT * bN / dt, total);
  return 0;
}

int main(int argc, char **argv)
{
  struct jpeg_error_mgr err;
  int a;
  if (argc > 1 && !strcmp(argv[1], "bench")) return bench(argc, argv);
  for (a = 1; a < argc; a++) {
    struct jpeg_compress_struct c;
    const char *sc = argv[a];
    const int W = 53, H = 29;
    void *rgb8 = make_image(W, H, 3, 8, 1), *rgb8b = make_image(W, H, 3, 8, 2), *gray16 = make_image(W, H, 1, 16, 3), *rgb16 = make_image(W, H, 3, 16, 4), *rgb12 = make_image(W, H, 3, 12, 5);
    printf("scenario %s\n", sc);
    c.err = jpeg_std_error(&err);
    err.error_exit = my_exit;
    jpeg_create_compress(&c);
    mem = NULL; memsize = 0;
    geometry_defined = 0;
    jpeg_mem_dest(&c, &mem, &memsize);
    if (setjmp(env)) { printf("  (left through error_exit)\n"); jpeg_destroy_compress(&c); continue; }
    if (!strcmp(sc, "lossy_lossless_lossy")) {
      /* one object: a baseline image, a lossless one, a baseline one again (jpeg_set_defaults clears the mode, jcparam.c:427) */
      base(&c, W, H, 3); jpeg_set_quality(&c, 80, TRUE);
      one_image(&c, "lossy 1", rgb8, 8, 1, TRUE);
      jpeg_enable_lossless(&c, 4, 0);
      one_image(&c, "lossless", rgb8b, 8, 1, TRUE);
      fields("after lossless", &c);
      one_image(&c, "lossless again, other predictor untouched object", rgb8, 8, 2, TRUE);
      jpeg_set_defaults(&c); c.dct_method = JDCT_ISLOW; jpeg_set_quality(&c, 80, TRUE);
      one_image(&c, "lossy 2", rgb8, 8, 1, TRUE);
      jpeg_enable_lossless(&c, 2, 1);
      jpeg_simple_progression(&c);          /* switches lossless off again, jcparam.c:876-878 */
      one_image(&c, "progressive after enable_lossless", rgb8, 8, 1, TRUE);
    } else if (!strcmp(sc, "fields")) {
      /* everything lossless mode overrides at jpeg_start_compress (jinit_c_master_control jcmaster.c:1067-1094) */
      struct jpeg_progress_mgr pm;
      base(&c, W, H, 3);
      jpeg_set_quality(&c, 1, TRUE);
      jpeg_set_colorspace(&c, JCS_YCbCr);
      c.comp_info[0].h_samp_factor = 2; c.comp_info[0].v_samp_factor = 2;
      c.smoothing_factor = 60; c.optimize_coding = FALSE; c.dct_method = JDCT_FLOAT; c.raw_data_in = TRUE;
      pm.progress_monitor = monitor; c.progress = &pm;
      jpeg_enable_lossless(&c, 7, 2);
      fields("before start", &c);
      one_image(&c, "lossless over lossy settings", rgb8, 8, 3, TRUE);
      printf("  passes: %d of %d\n", passes_seen, passes_total);
      c.progress = NULL;
    } else if (!strcmp(sc, "sixteen")) {
      base(&c, W, H, 1); c.data_precision = 16;
      jpeg_enable_lossless(&c, 6, 0);
      one_image(&c, "gray 16, rows in pieces of 5", gray16, 16, 5, TRUE);
      c.input_components = 3; c.in_color_space = JCS_RGB; jpeg_set_defaults(&c); c.data_precision = 16;
      jpeg_enable_lossless(&c, 1, 3);
      c.restart_in_rows = 4;
      one_image(&c, "rgb 16, rows in pieces of 8", rgb16, 16, 8, TRUE);
      jpeg_set_defaults(&c); c.data_precision = 12; c.restart_in_rows = 0;
      jpeg_enable_lossless(&c, 5, 0);
      one_image(&c, "rgb 12", rgb12, 12, 3, TRUE);
    } else if (!strcmp(sc, "sixteen_lossy")) {
      base(&c, W, H, 3); c.data_precision = 16;
      one_image(&c, "16 bits without lossless mode", rgb16, 16, 1, TRUE);
    } else if (!strcmp(sc, "script")) {
      /* scan_info set by the client: lossless comes from the script alone (validate_script jcmaster.c:302-311) */
      static const jpeg_scan_info s2[2] = { { 1, { 0 }, 4, 0, 0, 0 }, { 2, { 1, 2 }, 2, 0, 0, 1 } };
      static const jpeg_scan_info s3[3] = { { 1, { 0 }, 5, 0, 0, 0 }, { 1, { 1 }, 6, 0, 0, 3 }, { 1, { 2 }, 3, 0, 0, 1 } };
      static const jpeg_scan_info dct[2] = { { 1, { 0 }, 0, 63, 0, 0 }, { 2, { 1, 2 }, 0, 63, 0, 0 } };
      base(&c, W, H, 3);
      c.scan_info = s2; c.num_scans = 2; c.restart_in_rows = 2;
      one_image(&c, "two scans, no jpeg_enable_lossless", rgb8, 8, 1, TRUE);
      c.scan_info = s3; c.num_scans = 3; c.restart_in_rows = 0;
      one_image(&c, "three scans", rgb8b, 8, 4, TRUE);
      jpeg_enable_lossless(&c, 1, 0);
      c.scan_info = dct; c.num_scans = 2;
      one_image(&c, "a sequential DCT script switches lossless off", rgb8, 8, 1, TRUE);
    } else if (!strcmp(sc, "bad_script")) {
      static const jpeg_scan_info twice[2] = { { 2, { 0, 1 }, 1, 0, 0, 0 }, { 2, { 1, 2 }, 1, 0, 0, 0 } };
      base(&c, W, H, 3);
      c.scan_info = twice; c.num_scans = 2;
      one_image(&c, "component 1 twice", rgb8, 8, 1, TRUE);
    } else if (!strcmp(sc, "abbreviated")) {
      base(&c, W, H, 3);
      jpeg_enable_lossless(&c, 3, 0);
      one_image(&c, "write_all_tables FALSE", rgb8, 8, 1, FALSE);
      jpeg_suppress_tables(&c, TRUE);
      one_image(&c, "suppressed, FALSE", rgb8b, 8, 1, FALSE);
      jpeg_write_tables(&c);
      report("jpeg_write_tables");
      tables("after jpeg_write_tables", &c);
      one_image(&c, "after jpeg_write_tables, FALSE", rgb8, 8, 1, FALSE);
    } else if (!strcmp(sc, "abort")) {
      base(&c, W, H, 3);
      jpeg_enable_lossless(&c, 2, 0);
      jpeg_start_compress(&c, TRUE);
      geometry_defined = 1;
      rows(&c, rgb8, 8, H / 2, 1);
      jpeg_abort_compress(&c);
      fields("after abort", &c);
      one_image(&c, "lossless after abort", rgb8b, 8, 1, TRUE);
      jpeg_set_defaults(&c); c.dct_method = JDCT_ISLOW; jpeg_set_quality(&c, 70, TRUE);
      one_image(&c, "lossy after that", rgb8, 8, 1, TRUE);
    } else if (!strcmp(sc, "markers")) {
      static unsigned char icc[300];
      int i;
      for (i = 0; i < 300; i++) icc[i] = (unsigned char)(i * 7);
      base(&c, W, H, 3);
      jpeg_enable_lossless(&c, 1, 0);
      jpeg_start_compress(&c, TRUE);
      jpeg_write_icc_profile(&c, icc, 300);
      jpeg_write_marker(&c, JPEG_COM, (const JOCTET *)"lossless", 8);
      rows(&c, rgb8, 8, H, 1);
      jpeg_finish_compress(&c);
      report("ICC + COM");
    } else if (!strcmp(sc, "raw_data")) {
      JSAMPROW r[8]; JSAMPARRAY planes[3]; int k;
      for (k = 0; k < 8; k++) r[k] = (JSAMPROW)rgb8;
      planes[0] = planes[1] = planes[2] = r;
      base(&c, W, H, 3);
      c.raw_data_in = TRUE;
      jpeg_enable_lossless(&c, 1, 0);
      jpeg_start_compress(&c, TRUE);
      fields("raw_data_in asked for", &c);
      jpeg_write_raw_data(&c, planes, 8);
    } else if (!strcmp(sc, "restart_blocks")) {
      base(&c, W, H, 3);
      jpeg_enable_lossless(&c, 1, 0);
      c.restart_interval = 7;
      one_image(&c, "restart interval 7 on a width of 53", rgb8, 8, 1, TRUE);
    } else {
      fprintf(stderr, "unknown scenario %s\n", sc);
      return 2;
    }
    jpeg_destroy_compress(&c);
    free(mem);
    free(rgb8); free(rgb8b); free(gray16); free(rgb16); free(rgb12);
  }
  return 0;
}
