/* coef_dump.c -- TEST INFRASTRUCTURE (tests/coef_cases.py): a client of jpeg_read_coefficients.  It is linked to a libjpeg.so.62 and
 * run twice, with LD_LIBRARY_PATH at the reference's library and at the stand-alone one; what it prints and the files it writes
 * are compared, and its output on the reference's library is the expected value of mozjpeg_amd.decode_coefficients.
 *
 *   coef_dump dump FILE OUT [fields]      the coefficient arrays to OUT: per component two uint32 (width_in_blocks, height_in_blocks,
 *                                         host byte order) and the REAL blocks, row-major, 64 int16 each; with `fields` the public
 *                                         fields a transcoding client reads are printed, before and after jpeg_finish_decompress
 *   coef_dump two FILE1 FILE2 OUT         both files through ONE object, dumped one after the other
 *   coef_dump abbrev TABLES IMAGE OUT     jpeg_read_header(FALSE) on a tables-only datastream, then the abbreviated image, one object
 *   coef_dump badstate FILE               jpeg_read_coefficients after jpeg_start_decompress: the error text
 *   coef_dump abort FILE1 FILE2 OUT       jpeg_read_coefficients(FILE1), jpeg_abort_decompress, then FILE2 through the same object
 *   coef_dump zeroac FILE OUT             every AC coefficient of component 0 zeroed in the arrays, then jpeg_write_coefficients to OUT
 */
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

static FILE *open_or_die(const char *path, const char *mode)
{
  FILE *f = fopen(path, mode);
  if (!f) { perror(path); exit(3); }
  return f;
}

static unsigned sum(const void *p, size_t n)
{
  const unsigned char *b = (const unsigned char *)p;
  unsigned h = 2166136261u;
  size_t i;
  for (i = 0; i < n; i++) h = (h ^ b[i]) * 16777619u;
  return h;
}

static void print_fields(j_decompress_ptr c, const char *when)
{
  int i;
  jpeg_saved_marker_ptr mk;
  printf("[%s]\n", when);
  printf("image %u x %u comps %d jcs %d precision %d maxh %d maxv %d iMCU rows %u output %u x %u\n", c->image_width, c->image_height, c->num_components,
         (int)c->jpeg_color_space, c->data_precision, c->max_h_samp_factor, c->max_v_samp_factor, c->total_iMCU_rows, c->output_width, c->output_height);
  printf("output_scanline %u input_scan_number %d buffered %d multiscan %d complete %d\n", c->output_scanline, c->input_scan_number, c->buffered_image,
         jpeg_has_multiple_scans(c), jpeg_input_complete(c));
  printf("jfif %d %d.%d unit %d density %d x %d adobe %d transform %d\n", c->saw_JFIF_marker, c->JFIF_major_version, c->JFIF_minor_version, c->density_unit,
         c->X_density, c->Y_density, c->saw_Adobe_marker, c->Adobe_transform);
  for (i = 0; i < c->num_components; i++) {
    const jpeg_component_info *ci = &c->comp_info[i];
    printf("comp %d: id %d h %d v %d tq %d blocks %u x %u down %u x %u scaled %d quant_table ", i, ci->component_id, ci->h_samp_factor, ci->v_samp_factor,
           ci->quant_tbl_no, ci->width_in_blocks, ci->height_in_blocks, ci->downsampled_width, ci->downsampled_height, ci->DCT_scaled_size);
    if (ci->quant_table) printf("%08x\n", sum(ci->quant_table->quantval, sizeof(ci->quant_table->quantval)));
    else printf("none\n");
  }
  for (i = 0; i < NUM_QUANT_TBLS; i++)
    if (c->quant_tbl_ptrs[i]) printf("quant %d: %08x\n", i, sum(c->quant_tbl_ptrs[i]->quantval, sizeof(c->quant_tbl_ptrs[i]->quantval)));
    else printf("quant %d: none\n", i);
  for (mk = c->marker_list; mk; mk = mk->next)
    printf("marker %02x original %u kept %u %08x\n", mk->marker, mk->original_length, mk->data_length, sum(mk->data, mk->data_length));
}

/* the real blocks of every component, through access_virt_barray one row at a time */
static void dump_arrays(j_decompress_ptr c, jvirt_barray_ptr *arrays, FILE *out)
{
  int i;
  for (i = 0; i < c->num_components; i++) {
    const jpeg_component_info *ci = &c->comp_info[i];
    const unsigned dims[2] = { ci->width_in_blocks, ci->height_in_blocks };
    JDIMENSION r;
    fwrite(dims, sizeof(dims), 1, out);
    for (r = 0; r < ci->height_in_blocks; r++) {
      JBLOCKARRAY ba = (*c->mem->access_virt_barray) ((j_common_ptr)c, arrays[i], r, 1, FALSE);
      fwrite(ba[0], sizeof(JBLOCK), ci->width_in_blocks, out);
    }
  }
}

static void read_and_dump(j_decompress_ptr c, const char *path, FILE *out, int fields)
{
  FILE *in = open_or_die(path, "rb");
  jvirt_barray_ptr *arrays;
  jpeg_stdio_src(c, in);
  if (fields) { jpeg_save_markers(c, JPEG_COM, 0xFFFF); jpeg_save_markers(c, JPEG_APP0 + 1, 16); jpeg_save_markers(c, JPEG_APP0 + 2, 0xFFFF); }
  (void)jpeg_read_header(c, TRUE);
  arrays = jpeg_read_coefficients(c);
  if (fields) print_fields(c, "after jpeg_read_coefficients");
  dump_arrays(c, arrays, out);
  if (jpeg_read_coefficients(c) != arrays) printf("a second jpeg_read_coefficients returned other arrays\n");
  (void)jpeg_finish_decompress(c);
  if (fields) printf("after jpeg_finish_decompress: output_scanline %u input_scan_number %d\n", c->output_scanline, c->input_scan_number);
  fclose(in);
}

int main(int argc, char **argv)
{
  struct jpeg_decompress_struct c;
  client_err err;
  const char *what = argc > 1 ? argv[1] : "";
  FILE *out = NULL;
  c.err = jpeg_std_error(&err.pub);
  err.pub.error_exit = client_error_exit;
  if (setjmp(err.jb)) { jpeg_destroy_decompress(&c); return 1; }
  jpeg_create_decompress(&c);
  if (!strcmp(what, "dump") && argc >= 4) {
    out = open_or_die(argv[3], "wb");
    read_and_dump(&c, argv[2], out, argc > 4 && !strcmp(argv[4], "fields"));
  } else if (!strcmp(what, "two") && argc == 5) {
    out = open_or_die(argv[4], "wb");
    read_and_dump(&c, argv[2], out, 1);
    read_and_dump(&c, argv[3], out, 1);
  } else if (!strcmp(what, "abbrev") && argc == 5) {
    FILE *t = open_or_die(argv[2], "rb");
    out = open_or_die(argv[4], "wb");
    jpeg_stdio_src(&c, t);
    printf("tables: jpeg_read_header returned %d\n", jpeg_read_header(&c, FALSE));
    fclose(t);
    read_and_dump(&c, argv[3], out, 1);
  } else if (!strcmp(what, "badstate") && argc == 3) {
    FILE *in = open_or_die(argv[2], "rb");
    jpeg_stdio_src(&c, in);
    (void)jpeg_read_header(&c, TRUE);
    (void)jpeg_start_decompress(&c);
    (void)jpeg_read_coefficients(&c);             /* error_exit: JERR_BAD_STATE */
    printf("jpeg_read_coefficients returned\n");
  } else if (!strcmp(what, "abort") && argc == 5) {
    FILE *in = open_or_die(argv[2], "rb");
    out = open_or_die(argv[4], "wb");
    jpeg_stdio_src(&c, in);
    (void)jpeg_read_header(&c, TRUE);
    (void)jpeg_read_coefficients(&c);
    jpeg_abort_decompress(&c);
    fclose(in);
    printf("aborted: state %d\n", c.global_state);
    read_and_dump(&c, argv[3], out, 1);
  } else if (!strcmp(what, "zeroac") && argc == 4) {
    struct jpeg_compress_struct d;
    FILE *in = open_or_die(argv[2], "rb");
    jvirt_barray_ptr *arrays;
    JDIMENSION r, b;
    int k;
    out = open_or_die(argv[3], "wb");
    d.err = c.err;
    jpeg_create_compress(&d);
    jpeg_stdio_src(&c, in);
    (void)jpeg_read_header(&c, TRUE);
    arrays = jpeg_read_coefficients(&c);
    for (r = 0; r < c.comp_info[0].height_in_blocks; r++) {
      JBLOCKARRAY ba = (*c.mem->access_virt_barray) ((j_common_ptr)&c, arrays[0], r, 1, TRUE);
      for (b = 0; b < c.comp_info[0].width_in_blocks; b++)
        for (k = 1; k < DCTSIZE2; k++) ba[0][b][k] = 0;
    }
    jpeg_copy_critical_parameters(&c, &d);
    jpeg_stdio_dest(&d, out);
    jpeg_write_coefficients(&d, arrays);
    jpeg_finish_compress(&d);
    jpeg_destroy_compress(&d);
    (void)jpeg_finish_decompress(&c);
    fclose(in);
  } else {
    fprintf(stderr, "usage: coef_dump dump|two|abbrev|badstate|abort|zeroac ...\n");
    return 2;
  }
  jpeg_destroy_decompress(&c);
  if (out) fclose(out);
  return 0;
}
