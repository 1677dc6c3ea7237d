/* djpeg_client.c -- TEST INFRASTRUCTURE (tests/test_simt_djpeg.py, tests/test_gpu_djpeg.py): a client of the libjpeg DECOMPRESS API
 * beyond what djpeg reaches.  It is linked to a libjpeg.so.62 and run twice, with LD_LIBRARY_PATH at the reference's library and
 * at the stand-alone one; what it prints and the files it writes are compared.
 *
 *   djpeg_client fields FILE scale_denom fancy out_cs      every public field after jpeg_read_header / jpeg_calc_output_dimensions /
 *                                                          jpeg_start_decompress (out_cs < 0: the default)
 *   djpeg_client markers FILE                              marker_list after jpeg_save_markers(COM, 0xFFFF), (APP1, 16), (APP2, 0xFFFF)
 *   djpeg_client pixels FILE OUT out_cs rows dither        the pixels with out_color_space out_cs, `rows` per call (0: all), to OUT
 *   djpeg_client raw FILE OUT                              jpeg_read_raw_data: the samples of the real blocks of every component to OUT
 *   djpeg_client two FILE1 FILE2 OUT                       both files in ONE memory buffer, one object, read one after the other
 *   djpeg_client mkabbrev TABLES IMAGE                     writes a tables-only datastream and an abbreviated image (the compressor of
 *                                                          the library it runs on: the tests run this on the reference's)
 *   djpeg_client abbrev TABLES IMAGE OUT                   jpeg_read_header(FALSE) on the tables, then the abbreviated image, one object
 *   djpeg_client abort FILE1 FILE2 OUT                     jpeg_read_header(FILE1), jpeg_abort_decompress, then FILE2
 *   djpeg_client threads OUT FILE...                       one thread and one object per file; OUT.<i>
 *   djpeg_client damaged FILE                              a client error_exit (longjmp) and guard bytes behind the client's rows
 */
#include <pthread.h>
#include <setjmp.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "jpeglib.h"
#include "jerror.h"

typedef struct {
  struct jpeg_error_mgr pub;
  jmp_buf jb;
} client_err;

static void client_error_exit(j_common_ptr cinfo)
{
  client_err *e = (client_err *)cinfo->err;
  char msg[JMSG_LENGTH_MAX];
  (*cinfo->err->format_message) (cinfo, msg);
  printf("error_exit code=%d: %s\n", cinfo->err->msg_code, msg);
  longjmp(e->jb, 1);
}

static unsigned char *slurp(const char *path, size_t *n)
{
  FILE *f = fopen(path, "rb");
  unsigned char *b;
  long len;
  if (!f) { perror(path); exit(3); }
  fseek(f, 0, SEEK_END); len = ftell(f); fseek(f, 0, SEEK_SET);
  b = (unsigned char *)malloc((size_t)len + 1);
  if (fread(b, 1, (size_t)len, f) != (size_t)len) { perror(path); exit(3); }
  fclose(f);
  *n = (size_t)len;
  return b;
}

static unsigned sum(const void *p, size_t n)
{
  const unsigned char *b = (const unsigned char *)p;
  unsigned h = 2166136261u;
  size_t i;
  for (i = 0; i < n; i++) h = (h ^ b[i]) * 16777619u;
  return h;
}

static void print_header_fields(j_decompress_ptr c, const char *when)
{
  int i;
  printf("[%s]\n", when);
  printf("image %u x %u comps %d jcs %d out_cs %d state %d\n", c->image_width, c->image_height, c->num_components, (int)c->jpeg_color_space,
         (int)c->out_color_space, c->global_state);
  printf("scale %u/%u gamma %.2f buffered %d raw %d dct %d fancy %d smooth %d quantize %d dither %d two_pass %d colors %d e1 %d ee %d e2 %d\n", c->scale_num,
         c->scale_denom, c->output_gamma, c->buffered_image, c->raw_data_out, (int)c->dct_method, c->do_fancy_upsampling, c->do_block_smoothing,
         c->quantize_colors, (int)c->dither_mode, c->two_pass_quantize, c->desired_number_of_colors, c->enable_1pass_quant, c->enable_external_quant,
         c->enable_2pass_quant);
  for (i = 0; i < c->num_components; i++)
    printf("comp %d: id %d index %d h %d v %d tq %d td %d ta %d\n", i, c->comp_info[i].component_id, c->comp_info[i].component_index,
           c->comp_info[i].h_samp_factor, c->comp_info[i].v_samp_factor, c->comp_info[i].quant_tbl_no, c->comp_info[i].dc_tbl_no, c->comp_info[i].ac_tbl_no);
  printf("jfif %d %d.%d unit %d density %d x %d adobe %d transform %d restart %u precision %d maxh %d maxv %d\n", c->saw_JFIF_marker, c->JFIF_major_version,
         c->JFIF_minor_version, c->density_unit, c->X_density, c->Y_density, c->saw_Adobe_marker, c->Adobe_transform, c->restart_interval,
         c->data_precision, c->max_h_samp_factor, c->max_v_samp_factor);
  printf("progressive %d arith %d multiscan %d\n", c->progressive_mode, c->arith_code, jpeg_has_multiple_scans(c));
  for (i = 0; i < NUM_QUANT_TBLS; i++)
    if (c->quant_tbl_ptrs[i]) printf("quant %d: %08x\n", i, sum(c->quant_tbl_ptrs[i]->quantval, sizeof(c->quant_tbl_ptrs[i]->quantval)));
    else printf("quant %d: none\n", i);
  for (i = 0; i < NUM_HUFF_TBLS; i++) {
    if (c->dc_huff_tbl_ptrs[i]) printf("dc %d: %08x %08x\n", i, sum(c->dc_huff_tbl_ptrs[i]->bits, 17), sum(c->dc_huff_tbl_ptrs[i]->huffval, 256));
    else printf("dc %d: none\n", i);
    if (c->ac_huff_tbl_ptrs[i]) printf("ac %d: %08x %08x\n", i, sum(c->ac_huff_tbl_ptrs[i]->bits, 17), sum(c->ac_huff_tbl_ptrs[i]->huffval, 256));
    else printf("ac %d: none\n", i);
  }
}

static void print_output_fields(j_decompress_ptr c, const char *when)
{
  int i;
  printf("[%s]\n", when);
  printf("output %u x %u out_color_components %d output_components %d rec_outbuf_height %d output_scanline %u state %d\n", c->output_width, c->output_height,
         c->out_color_components, c->output_components, c->rec_outbuf_height, c->output_scanline, c->global_state);
  for (i = 0; i < c->num_components; i++)
    printf("comp %d: scaled %d down %u x %u blocks %u x %u\n", i, c->comp_info[i].DCT_scaled_size, c->comp_info[i].downsampled_width,
           c->comp_info[i].downsampled_height, c->comp_info[i].width_in_blocks, c->comp_info[i].height_in_blocks);
}

static size_t pixel_bytes(j_decompress_ptr c) { return c->out_color_space == JCS_RGB565 ? 2 : (size_t)c->output_components; }

/* reads the image of a started object `rows` rows per call (0: all) and appends the pixels to f */
static void read_image(j_decompress_ptr c, int rows, FILE *f)
{
  const size_t row_bytes = c->output_width * pixel_bytes(c);
  const JDIMENSION ask = rows > 0 ? (JDIMENSION)rows : c->output_height;
  unsigned char *buf = (unsigned char *)malloc(row_bytes * ask);
  JSAMPROW *ptr = (JSAMPROW *)malloc(sizeof(JSAMPROW) * ask);
  JDIMENSION i;
  for (i = 0; i < ask; i++) ptr[i] = buf + (size_t)i * row_bytes;
  while (c->output_scanline < c->output_height) {
    const JDIMENSION got = jpeg_read_scanlines(c, ptr, ask);
    if (got == 0 || got > ask) { printf("jpeg_read_scanlines returned %u\n", got); exit(4); }
    fwrite(buf, row_bytes, got, f);
  }
  free(ptr);
  free(buf);
}

static int do_fields(int argc, char **argv)
{
  struct jpeg_decompress_struct c;
  client_err err;
  FILE *in;
  const int denom = argc > 3 ? atoi(argv[3]) : 1, fancy = argc > 4 ? atoi(argv[4]) : 1, cs = argc > 5 ? atoi(argv[5]) : -1;
  c.err = jpeg_std_error(&err.pub);
  err.pub.error_exit = client_error_exit;
  if (setjmp(err.jb)) { jpeg_destroy_decompress(&c); return 1; }
  jpeg_create_decompress(&c);
  in = fopen(argv[2], "rb");
  if (!in) { perror(argv[2]); return 3; }
  jpeg_stdio_src(&c, in);
  printf("header %d\n", jpeg_read_header(&c, TRUE));
  print_header_fields(&c, "after jpeg_read_header");
  c.scale_num = 1; c.scale_denom = (unsigned)denom;
  c.do_fancy_upsampling = fancy;
  if (cs >= 0) c.out_color_space = (J_COLOR_SPACE)cs;
  jpeg_calc_output_dimensions(&c);
  print_output_fields(&c, "after jpeg_calc_output_dimensions");
  printf("start %d\n", jpeg_start_decompress(&c));
  print_header_fields(&c, "after jpeg_start_decompress");
  print_output_fields(&c, "after jpeg_start_decompress");
  {
    FILE *sink = fopen("/dev/null", "wb");
    read_image(&c, 1, sink);
    fclose(sink);
  }
  printf("scanline %u\n", c.output_scanline);
  printf("finish %d\n", jpeg_finish_decompress(&c));
  /* (asked after jpeg_finish_decompress: the stand-alone library has read EOI by the end of jpeg_start_decompress, the reference not) */
  printf("state %d complete %d\n", c.global_state, jpeg_input_complete(&c));
  jpeg_destroy_decompress(&c);
  fclose(in);
  return 0;
}

static int do_markers(char **argv)
{
  struct jpeg_decompress_struct c;
  client_err err;
  size_t n;
  unsigned char *file = slurp(argv[2], &n);
  jpeg_saved_marker_ptr m;
  JOCTET *icc = NULL;
  unsigned int icc_len = 0;
  c.err = jpeg_std_error(&err.pub);
  err.pub.error_exit = client_error_exit;
  if (setjmp(err.jb)) { jpeg_destroy_decompress(&c); return 1; }
  jpeg_create_decompress(&c);
  jpeg_mem_src(&c, file, (unsigned long)n);
  jpeg_save_markers(&c, JPEG_COM, 0xFFFF);
  jpeg_save_markers(&c, JPEG_APP0 + 1, 16);
  jpeg_save_markers(&c, JPEG_APP0 + 2, 0xFFFF);
  jpeg_read_header(&c, TRUE);
  for (m = c.marker_list; m; m = m->next)
    printf("marker 0x%02x original_length %u data_length %u data %08x\n", m->marker, m->original_length, m->data_length, sum(m->data, m->data_length));
  if (jpeg_read_icc_profile(&c, &icc, &icc_len)) printf("icc %u bytes %08x\n", icc_len, sum(icc, icc_len));
  else printf("no icc profile\n");
  free(icc);
  jpeg_start_decompress(&c);
  printf("list kept %d\n", c.marker_list != NULL);
  {
    FILE *sink = fopen("/dev/null", "wb");
    read_image(&c, 0, sink);
    fclose(sink);
  }
  jpeg_finish_decompress(&c);
  printf("list after finish %d\n", c.marker_list != NULL);
  jpeg_destroy_decompress(&c);
  return 0;
}

static int do_pixels(int argc, char **argv)
{
  struct jpeg_decompress_struct c;
  client_err err;
  size_t n;
  unsigned char *file = slurp(argv[2], &n);
  FILE *out = fopen(argv[3], "wb");
  const int cs = argc > 4 ? atoi(argv[4]) : -1, rows = argc > 5 ? atoi(argv[5]) : 1, dither = argc > 6 ? atoi(argv[6]) : 1;
  c.err = jpeg_std_error(&err.pub);
  err.pub.error_exit = client_error_exit;
  if (setjmp(err.jb)) { jpeg_destroy_decompress(&c); return 1; }
  jpeg_create_decompress(&c);
  jpeg_mem_src(&c, file, (unsigned long)n);
  jpeg_read_header(&c, TRUE);
  if (cs >= 0) c.out_color_space = (J_COLOR_SPACE)cs;
  if (!dither) c.dither_mode = JDITHER_NONE;
  jpeg_start_decompress(&c);
  printf("%u x %u, %d components\n", c.output_width, c.output_height, c.output_components);
  read_image(&c, rows, out);
  jpeg_finish_decompress(&c);
  jpeg_destroy_decompress(&c);
  fclose(out);
  return 0;
}

static int do_raw(char **argv)
{
  struct jpeg_decompress_struct c;
  client_err err;
  size_t n;
  unsigned char *file = slurp(argv[2], &n);
  FILE *out = fopen(argv[3], "wb");
  unsigned char *plane[3];
  size_t pw[3], ph[3];
  JSAMPROW rowptr[3][32];
  JSAMPARRAY image[3];
  int ci, r;
  c.err = jpeg_std_error(&err.pub);
  err.pub.error_exit = client_error_exit;
  if (setjmp(err.jb)) { jpeg_destroy_decompress(&c); return 1; }
  jpeg_create_decompress(&c);
  jpeg_mem_src(&c, file, (unsigned long)n);
  jpeg_read_header(&c, TRUE);
  c.raw_data_out = TRUE;
  jpeg_start_decompress(&c);
  for (ci = 0; ci < c.num_components; ci++) {
    /* whole iMCU rows, padded to whole MCUs across: the library writes the real blocks, the rest keeps the 0x5A put here */
    pw[ci] = (size_t)c.comp_info[ci].width_in_blocks * 8 + 64;
    ph[ci] = (size_t)c.total_iMCU_rows * c.comp_info[ci].v_samp_factor * 8;
    plane[ci] = (unsigned char *)malloc(pw[ci] * ph[ci]);
    memset(plane[ci], 0x5A, pw[ci] * ph[ci]);
    image[ci] = rowptr[ci];
  }
  while (c.output_scanline < c.output_height) {
    const JDIMENSION imcu = c.output_scanline / (JDIMENSION)(c.max_v_samp_factor * 8);
    JDIMENSION got;
    for (ci = 0; ci < c.num_components; ci++)
      for (r = 0; r < c.comp_info[ci].v_samp_factor * 8; r++) rowptr[ci][r] = plane[ci] + ((size_t)imcu * c.comp_info[ci].v_samp_factor * 8 + r) * pw[ci];
    got = jpeg_read_raw_data(&c, image, (JDIMENSION)(c.max_v_samp_factor * 8));
    if (got != (JDIMENSION)(c.max_v_samp_factor * 8)) { printf("jpeg_read_raw_data returned %u\n", got); return 4; }
  }
  printf("scanline %u of %u\n", c.output_scanline, c.output_height);
  for (ci = 0; ci < c.num_components; ci++) {
    /* the samples of real blocks; everything beyond them in the padded width must still be the fill */
    size_t y, x, touched = 0;
    for (y = 0; y < (size_t)c.comp_info[ci].height_in_blocks * 8; y++) fwrite(plane[ci] + y * pw[ci], 1, (size_t)c.comp_info[ci].width_in_blocks * 8, out);
    for (y = 0; y < ph[ci]; y++)
      for (x = (size_t)c.comp_info[ci].width_in_blocks * 8 + 16; x < pw[ci]; x++) touched += plane[ci][y * pw[ci] + x] != 0x5A;
    printf("component %d: %u x %u blocks, %zu bytes touched beyond the MCU-padded width\n", ci, c.comp_info[ci].width_in_blocks, c.comp_info[ci].height_in_blocks, touched);
  }
  jpeg_finish_decompress(&c);
  jpeg_destroy_decompress(&c);
  fclose(out);
  return 0;
}

static int do_two(char **argv)
{
  struct jpeg_decompress_struct c;
  client_err err;
  size_t n1, n2;
  unsigned char *f1 = slurp(argv[2], &n1), *f2 = slurp(argv[3], &n2);
  unsigned char *both = (unsigned char *)malloc(n1 + n2);
  FILE *out = fopen(argv[4], "wb");
  int i;
  memcpy(both, f1, n1);
  memcpy(both + n1, f2, n2);
  c.err = jpeg_std_error(&err.pub);
  err.pub.error_exit = client_error_exit;
  if (setjmp(err.jb)) { jpeg_destroy_decompress(&c); return 1; }
  jpeg_create_decompress(&c);
  jpeg_mem_src(&c, both, (unsigned long)(n1 + n2));
  for (i = 0; i < 2; i++) {
    jpeg_read_header(&c, TRUE);
    jpeg_start_decompress(&c);
    printf("image %d: %u x %u, %d components\n", i, c.output_width, c.output_height, c.output_components);
    read_image(&c, 2, out);
    jpeg_finish_decompress(&c);
    printf("image %d: %zu bytes of the buffer left\n", i, c.src->bytes_in_buffer);
  }
  jpeg_destroy_decompress(&c);
  fclose(out);
  return 0;
}

static int do_mkabbrev(char **argv)
{
  struct jpeg_compress_struct c;
  struct jpeg_error_mgr err;
  unsigned char *tables = NULL, *image = NULL;
  unsigned long ntables = 0, nimage = 0;
  unsigned char row[40 * 3];
  JSAMPROW rp = row;
  FILE *f;
  int x, y;
  c.err = jpeg_std_error(&err);
  jpeg_create_compress(&c);
  c.image_width = 40; c.image_height = 24; c.input_components = 3; c.in_color_space = JCS_RGB;
  if (jpeg_c_int_param_supported(&c, JINT_COMPRESS_PROFILE)) jpeg_c_set_int_param(&c, JINT_COMPRESS_PROFILE, JCP_FASTEST);   /* baseline, the standard Huffman tables */
  jpeg_set_defaults(&c);
  jpeg_set_quality(&c, 60, TRUE);
  jpeg_mem_dest(&c, &tables, &ntables);
  jpeg_write_tables(&c);
  jpeg_mem_dest(&c, &image, &nimage);
  jpeg_start_compress(&c, FALSE);
  for (y = 0; y < 24; y++) {
    for (x = 0; x < 40; x++) { row[3 * x] = (unsigned char)(x * 6 + y); row[3 * x + 1] = (unsigned char)(y * 10); row[3 * x + 2] = (unsigned char)(255 - x * 5); }
    jpeg_write_scanlines(&c, &rp, 1);
  }
  jpeg_finish_compress(&c);
  jpeg_destroy_compress(&c);
  f = fopen(argv[2], "wb"); fwrite(tables, 1, ntables, f); fclose(f);
  f = fopen(argv[3], "wb"); fwrite(image, 1, nimage, f); fclose(f);
  printf("tables %lu bytes, image %lu bytes\n", ntables, nimage);
  return 0;
}

static int do_abbrev(char **argv)
{
  struct jpeg_decompress_struct c;
  client_err err;
  size_t n1, n2;
  unsigned char *tables = slurp(argv[2], &n1), *image = slurp(argv[3], &n2);
  FILE *out = fopen(argv[4], "wb");
  c.err = jpeg_std_error(&err.pub);
  err.pub.error_exit = client_error_exit;
  if (setjmp(err.jb)) { jpeg_destroy_decompress(&c); return 1; }
  jpeg_create_decompress(&c);
  jpeg_mem_src(&c, tables, (unsigned long)n1);
  printf("tables: jpeg_read_header %d state %d quant0 %d dc0 %d ac1 %d\n", jpeg_read_header(&c, FALSE), c.global_state, c.quant_tbl_ptrs[0] != NULL,
         c.dc_huff_tbl_ptrs[0] != NULL, c.ac_huff_tbl_ptrs[1] != NULL);
  jpeg_mem_src(&c, image, (unsigned long)n2);
  printf("image: jpeg_read_header %d\n", jpeg_read_header(&c, TRUE));
  jpeg_start_decompress(&c);
  printf("%u x %u, %d components\n", c.output_width, c.output_height, c.output_components);
  read_image(&c, 1, out);
  jpeg_finish_decompress(&c);
  jpeg_destroy_decompress(&c);
  fclose(out);
  return 0;
}

static int do_abort(char **argv)
{
  struct jpeg_decompress_struct c;
  client_err err;
  size_t n1, n2;
  unsigned char *f1 = slurp(argv[2], &n1), *f2 = slurp(argv[3], &n2);
  FILE *out = fopen(argv[4], "wb");
  c.err = jpeg_std_error(&err.pub);
  err.pub.error_exit = client_error_exit;
  if (setjmp(err.jb)) { jpeg_destroy_decompress(&c); return 1; }
  jpeg_create_decompress(&c);
  jpeg_mem_src(&c, f1, (unsigned long)n1);
  jpeg_save_markers(&c, JPEG_COM, 0xFFFF);
  jpeg_read_header(&c, TRUE);
  printf("first: %u x %u state %d\n", c.image_width, c.image_height, c.global_state);
  jpeg_abort_decompress(&c);
  printf("aborted: state %d marker_list %d\n", c.global_state, c.marker_list != NULL);
  jpeg_mem_src(&c, f2, (unsigned long)n2);
  jpeg_read_header(&c, TRUE);
  jpeg_start_decompress(&c);
  printf("second: %u x %u, %d components\n", c.output_width, c.output_height, c.output_components);
  read_image(&c, 3, out);
  jpeg_finish_decompress(&c);
  jpeg_destroy_decompress(&c);
  fclose(out);
  return 0;
}

typedef struct { const char *in; char out[512]; int rc; } job;

static void *thread_main(void *arg)
{
  job *j = (job *)arg;
  struct jpeg_decompress_struct c;
  client_err err;
  size_t n;
  unsigned char *file = slurp(j->in, &n);
  FILE *out = fopen(j->out, "wb");
  int round;
  c.err = jpeg_std_error(&err.pub);
  err.pub.error_exit = client_error_exit;
  if (setjmp(err.jb)) { jpeg_destroy_decompress(&c); j->rc = 1; return NULL; }
  jpeg_create_decompress(&c);
  for (round = 0; round < 2; round++) {                /* (the second round: an encoder out of the cache) */
    jpeg_mem_src(&c, file, (unsigned long)n);
    jpeg_read_header(&c, TRUE);
    jpeg_start_decompress(&c);
    if (round == 1) read_image(&c, 4, out);
    else { FILE *sink = fopen("/dev/null", "wb"); read_image(&c, 0, sink); fclose(sink); }
    jpeg_finish_decompress(&c);
  }
  jpeg_destroy_decompress(&c);
  fclose(out);
  free(file);
  j->rc = 0;
  return NULL;
}

static int do_threads(int argc, char **argv)
{
  const int n = argc - 3;
  pthread_t th[64];
  job jobs[64];
  int i, bad = 0;
  if (n < 1 || n > 64) return 2;
  for (i = 0; i < n; i++) { jobs[i].in = argv[3 + i]; snprintf(jobs[i].out, sizeof(jobs[i].out), "%s.%d", argv[2], i); jobs[i].rc = -1; }
  for (i = 0; i < n; i++) pthread_create(&th[i], NULL, thread_main, &jobs[i]);
  for (i = 0; i < n; i++) { pthread_join(th[i], NULL); bad += jobs[i].rc != 0; }
  printf("%d threads, %d failed\n", n, bad);
  return bad ? 1 : 0;
}

static int do_damaged(char **argv)
{
  struct jpeg_decompress_struct c;
  client_err err;
  size_t n, row_bytes = 0, i;
  unsigned char *file = slurp(argv[2], &n);
  static unsigned char *volatile buf = NULL;
  static volatile size_t buf_size = 0;
  static volatile int rows_read = 0;
  c.err = jpeg_std_error(&err.pub);
  err.pub.error_exit = client_error_exit;
  if (setjmp(err.jb)) {
    size_t touched = 0;
    for (i = 0; buf && i < buf_size; i++) touched += buf[i] != 0xA5;
    printf("after error_exit: %d rows were delivered, %zu bytes of the client's buffer and its guard changed\n", rows_read, touched);
    jpeg_destroy_decompress(&c);
    return 1;
  }
  jpeg_create_decompress(&c);
  jpeg_mem_src(&c, file, (unsigned long)n);
  jpeg_read_header(&c, TRUE);
  jpeg_calc_output_dimensions(&c);
  row_bytes = (size_t)c.output_width * (size_t)c.output_components;
  buf_size = row_bytes + 4096;
  buf = (unsigned char *)malloc(buf_size);
  memset(buf, 0xA5, buf_size);
  jpeg_start_decompress(&c);
  while (c.output_scanline < c.output_height) {
    JSAMPROW rp = buf;
    size_t touched = 0;
    jpeg_read_scanlines(&c, &rp, 1);
    rows_read++;
    for (i = row_bytes; i < buf_size; i++) touched += buf[i] != 0xA5;
    if (touched) { printf("%zu guard bytes behind row %d changed\n", touched, rows_read - 1); return 4; }
  }
  jpeg_finish_decompress(&c);
  jpeg_destroy_decompress(&c);
  printf("decoded: %d rows, %ld warnings\n", rows_read, err.pub.num_warnings);
  return 0;
}

int main(int argc, char **argv)
{
  if (argc < 3) { fprintf(stderr, "usage: djpeg_client scenario arguments (see the head of djpeg_client.c)\n"); return 2; }
  if (!strcmp(argv[1], "fields")) return do_fields(argc, argv);
  if (!strcmp(argv[1], "markers")) return do_markers(argv);
  if (!strcmp(argv[1], "pixels") && argc >= 4) return do_pixels(argc, argv);
  if (!strcmp(argv[1], "raw") && argc >= 4) return do_raw(argv);
  if (!strcmp(argv[1], "two") && argc >= 5) return do_two(argv);
  if (!strcmp(argv[1], "mkabbrev") && argc >= 4) return do_mkabbrev(argv);
  if (!strcmp(argv[1], "abbrev") && argc >= 5) return do_abbrev(argv);
  if (!strcmp(argv[1], "abort") && argc >= 5) return do_abort(argv);
  if (!strcmp(argv[1], "threads") && argc >= 4) return do_threads(argc, argv);
  if (!strcmp(argv[1], "damaged")) return do_damaged(argv);
  fprintf(stderr, "djpeg_client: unknown scenario %s\n", argv[1]);
  return 2;
}
