/* region_client.c -- a small client of the libjpeg partial-decompression API (TEST INFRASTRUCTURE, tests/region_cases.py):
 * jpeg_crop_scanline (twice when a second pair is given: the second call narrows the first), jpeg_skip_scanlines, one
 * jpeg_read_scanlines call per row as djpeg makes them, jpeg_skip_scanlines to the end, jpeg_finish_decompress.  It prints every
 * value the calls return or set and writes the rows it read, as they are, to a file.  Linked to libjpeg.so.62: run on the
 * reference's library it is the reference of the RGB565 regions, which the reference's djpeg cannot write (its BMP writer has
 * no -crop), and of every number jpeg_crop_scanline hands back.
 *
 *   region_client in.jpg out.bin <rgb565 0|1> <dither 0|1> <scale_num> <scale_denom> <fancy 0|1> <x> <w> <y> <h> [<x2> <w2>]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <setjmp.h>
#include <jpeglib.h>

struct err_mgr { struct jpeg_error_mgr pub; jmp_buf jb; };

static void on_error(j_common_ptr cinfo)
{
  char text[JMSG_LENGTH_MAX];
  (*cinfo->err->format_message)(cinfo, text);
  printf("error %d: %s\n", cinfo->err->msg_code, text);
  longjmp(((struct err_mgr *)cinfo->err)->jb, 1);
}

int main(int argc, char **argv)
{
  if (argc != 12 && argc != 14) { fprintf(stderr, "usage: region_client in.jpg out.bin rgb565 dither num denom fancy x w y h [x2 w2]\n"); return 2; }
  FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  if (!in || !out) { perror("region_client"); return 2; }
  const int rgb565 = atoi(argv[3]), dither = atoi(argv[4]), num = atoi(argv[5]), denom = atoi(argv[6]), fancy = atoi(argv[7]);
  JDIMENSION x = (JDIMENSION)atol(argv[8]), w = (JDIMENSION)atol(argv[9]);
  const JDIMENSION y = (JDIMENSION)atol(argv[10]), h = (JDIMENSION)atol(argv[11]);
  struct jpeg_decompress_struct cinfo;
  struct err_mgr err;
  JSAMPLE *row = NULL;
  cinfo.err = jpeg_std_error(&err.pub);
  err.pub.error_exit = on_error;
  if (setjmp(err.jb)) { jpeg_destroy_decompress(&cinfo); free(row); fclose(out); return 1; }
  jpeg_create_decompress(&cinfo);
  jpeg_stdio_src(&cinfo, in);
  jpeg_read_header(&cinfo, TRUE);
  cinfo.scale_num = (unsigned)num; cinfo.scale_denom = (unsigned)denom;
  cinfo.do_fancy_upsampling = fancy ? TRUE : FALSE;
  if (rgb565) { cinfo.out_color_space = JCS_RGB565; cinfo.dither_mode = dither ? JDITHER_ORDERED : JDITHER_NONE; }
  jpeg_start_decompress(&cinfo);
  printf("output %u x %u, %d components\n", cinfo.output_width, cinfo.output_height, cinfo.output_components);
  const JDIMENSION full_width = cinfo.output_width;
  jpeg_crop_scanline(&cinfo, &x, &w);
  printf("crop: xoffset %u width %u output_width %u\n", x, w, cinfo.output_width);
  if (argc == 14) {
    x = (JDIMENSION)atol(argv[12]); w = (JDIMENSION)atol(argv[13]);
    jpeg_crop_scanline(&cinfo, &x, &w);
    printf("crop again: xoffset %u width %u output_width %u\n", x, w, cinfo.output_width);
  }
  row = (JSAMPLE *)malloc((size_t)full_width * 4);
  printf("skip %u: %u\n", y, jpeg_skip_scanlines(&cinfo, y));
  printf("output_scanline %u\n", cinfo.output_scanline);
  const size_t row_bytes = (size_t)cinfo.output_width * (rgb565 ? 2u : (size_t)cinfo.output_components);     /* (output_components is 3 for 16-bit pixels) */
  while (cinfo.output_scanline < y + h) {
    JSAMPROW rows[1] = { row };
    if (jpeg_read_scanlines(&cinfo, rows, 1) != 1) { printf("a read returned no row\n"); break; }
    fwrite(row, 1, row_bytes, out);
  }
  printf("output_scanline %u\n", cinfo.output_scanline);
  printf("skip to the end: %u\n", jpeg_skip_scanlines(&cinfo, cinfo.output_height));      /* (clamped at the bottom) */
  printf("output_scanline %u\n", cinfo.output_scanline);
  printf("finish: %d, warnings %ld\n", (int)jpeg_finish_decompress(&cinfo), cinfo.err->num_warnings);
  jpeg_destroy_decompress(&cinfo);
  free(row);
  fclose(out);
  fclose(in);
  return 0;
}
