/* A client of the libjpeg DECOMPRESS API for files of up to four components (TEST INFRASTRUCTURE, tests/cmyk_cases.py compiles it at
 * test time against the reference's headers; it runs on the reference's libjpeg.so.62 and on the stand-alone one).
 *   cmyk_client raw FILE OUT          jpeg_read_raw_data: per component its height_in_blocks * 8 rows of width_in_blocks * 8 samples
 *   cmyk_client pixels FILE OUT CS    jpeg_read_scanlines with out_color_space CS (-1: the library's choice): the rows, tight
 * Both print the fields a client reads after jpeg_start_decompress.  Exit status 1: the library's error_exit (its message is printed). */
#include <setjmp.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "jpeglib.h"

typedef struct { struct jpeg_error_mgr pub; jmp_buf jb; } client_err;

static void client_error_exit(j_common_ptr c)
{
  char msg[JMSG_LENGTH_MAX];
  (*c->err->format_message)(c, msg);
  printf("error_exit: %s\n", msg);
  longjmp(((client_err *)c->err)->jb, 1);
}

static void quiet_message(j_common_ptr c, int level) { (void)c; (void)level; }

static unsigned char *slurp(const char *path, size_t *n)
{
  FILE *f = fopen(path, "rb");
  unsigned char *p;
  if (!f) { perror(path); exit(3); }
  fseek(f, 0, SEEK_END);
  *n = (size_t)ftell(f);
  fseek(f, 0, SEEK_SET);
  p = (unsigned char *)malloc(*n + 1);
  if (fread(p, 1, *n, f) != *n) { perror(path); exit(3); }
  fclose(f);
  return p;
}

static void print_fields(j_decompress_ptr c)
{
  int ci;
  printf("%u x %u, %d components, jpeg_color_space %d, out_color_space %d, out_color_components %d, output_components %d, Adobe %d/%d\n", c->output_width,
         c->output_height, c->num_components, (int)c->jpeg_color_space, (int)c->out_color_space, c->out_color_components, c->output_components,
         (int)c->saw_Adobe_marker, (int)c->Adobe_transform);
  for (ci = 0; ci < c->num_components; ci++)
    printf("component %d: id %d, %dx%d, %u x %u blocks, downsampled %u x %u\n", ci, c->comp_info[ci].component_id, c->comp_info[ci].h_samp_factor,
           c->comp_info[ci].v_samp_factor, c->comp_info[ci].width_in_blocks, c->comp_info[ci].height_in_blocks, c->comp_info[ci].downsampled_width,
           c->comp_info[ci].downsampled_height);
}

static int do_raw(char **argv)
{
  struct jpeg_decompress_struct c;
  client_err err;
  size_t n;
  unsigned char *file = slurp(argv[2], &n);
  FILE *out = fopen(argv[3], "wb");
  unsigned char *plane[MAX_COMPONENTS];
  size_t pw[MAX_COMPONENTS], ph[MAX_COMPONENTS];
  JSAMPROW rowptr[4][32];
  JSAMPARRAY image[4];
  int ci, r;
  c.err = jpeg_std_error(&err.pub);
  err.pub.error_exit = client_error_exit;
  err.pub.emit_message = quiet_message;
  if (setjmp(err.jb)) { jpeg_destroy_decompress(&c); return 1; }
  jpeg_create_decompress(&c);
  jpeg_mem_src(&c, file, (unsigned long)n);
  jpeg_read_header(&c, TRUE);
  if (c.num_components > 4) return 5;
  c.raw_data_out = TRUE;
  jpeg_start_decompress(&c);
  print_fields(&c);
  for (ci = 0; ci < c.num_components; ci++) {
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
  for (ci = 0; ci < c.num_components; ci++) {
    size_t y;
    for (y = 0; y < (size_t)c.comp_info[ci].height_in_blocks * 8; y++) fwrite(plane[ci] + y * pw[ci], 1, (size_t)c.comp_info[ci].width_in_blocks * 8, out);
  }
  jpeg_finish_decompress(&c);
  jpeg_destroy_decompress(&c);
  fclose(out);
  return 0;
}

static int do_pixels(char **argv)
{
  struct jpeg_decompress_struct c;
  client_err err;
  size_t n;
  unsigned char *file = slurp(argv[2], &n);
  FILE *out = fopen(argv[3], "wb");
  const int cs = atoi(argv[4]);
  unsigned char *row;
  c.err = jpeg_std_error(&err.pub);
  err.pub.error_exit = client_error_exit;
  err.pub.emit_message = quiet_message;
  if (setjmp(err.jb)) { jpeg_destroy_decompress(&c); return 1; }
  jpeg_create_decompress(&c);
  jpeg_mem_src(&c, file, (unsigned long)n);
  jpeg_read_header(&c, TRUE);
  printf("after the header: jpeg_color_space %d, out_color_space %d\n", (int)c.jpeg_color_space, (int)c.out_color_space);
  if (cs >= 0) c.out_color_space = (J_COLOR_SPACE)cs;
  jpeg_start_decompress(&c);
  print_fields(&c);
  row = (unsigned char *)malloc((size_t)c.output_width * (size_t)c.output_components + 16);
  while (c.output_scanline < c.output_height) {
    JSAMPROW rp = row;
    if (jpeg_read_scanlines(&c, &rp, 1) != 1) { printf("jpeg_read_scanlines returned no row\n"); return 4; }
    fwrite(row, 1, (size_t)c.output_width * (size_t)c.output_components, out);
  }
  jpeg_finish_decompress(&c);
  jpeg_destroy_decompress(&c);
  fclose(out);
  return 0;
}

int main(int argc, char **argv)
{
  if (argc >= 4 && !strcmp(argv[1], "raw")) return do_raw(argv);
  if (argc >= 5 && !strcmp(argv[1], "pixels")) return do_pixels(argv);
  fprintf(stderr, "usage: cmyk_client raw FILE OUT | pixels FILE OUT CS\n");
  return 2;
}
