/* djpeg_bench.c -- decompress throughput of a libjpeg client (MEASUREMENT TOOL, public API only): T threads, each with its own
 * decompress object, reading JPEG files from memory (jpeg_mem_src) through jpeg_read_header / jpeg_start_decompress /
 * jpeg_read_scanlines / jpeg_finish_decompress -- exactly what an application does.  The same binary is timed against the
 * reference's libjpeg.so.62 (CPU) and against the stand-alone library (tools/bench_djpeg_dropin.py picks it through
 * LD_LIBRARY_PATH).  Thread t starts at file t and takes every file in turn.
 *      usage: djpeg_bench THREADS FILES_PER_THREAD ROWS_PER_CALL(0 = all) FILE...       */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "jpeglib.h"

static int NPER, ROWS, NFILES;
static unsigned char **files;
static size_t *sizes;
static unsigned long long hashes[256];
static unsigned long long pixels[256];

static double now(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; }

static void *worker(void *arg)
{
  const int id = (int)(long)arg;
  struct jpeg_decompress_struct c;
  struct jpeg_error_mgr err;
  unsigned char *buf = NULL;
  JSAMPROW *rowp = NULL;
  size_t cap = 0;
  int i;
  c.err = jpeg_std_error(&err);
  jpeg_create_decompress(&c);
  for (i = 0; i < NPER; i++) {
    const int f = (id + i) % NFILES;
    size_t row_bytes;
    JDIMENSION y, ask;
    jpeg_mem_src(&c, files[f], (unsigned long)sizes[f]);
    jpeg_read_header(&c, TRUE);
    jpeg_start_decompress(&c);
    row_bytes = (size_t)c.output_width * c.output_components;
    if (row_bytes * c.output_height > cap) {
      cap = row_bytes * c.output_height;
      buf = (unsigned char *)realloc(buf, cap);
      rowp = (JSAMPROW *)realloc(rowp, sizeof(JSAMPROW) * c.output_height);
    }
    for (y = 0; y < c.output_height; y++) rowp[y] = buf + (size_t)y * row_bytes;
    ask = ROWS > 0 ? (JDIMENSION)ROWS : c.output_height;
    while (c.output_scanline < c.output_height) jpeg_read_scanlines(&c, rowp + c.output_scanline, ask);
    pixels[id] += (unsigned long long)c.output_width * c.output_height;
    if (i == 0 && id == 0) { unsigned long long h = 1469598103934665603ull; size_t k; for (k = 0; k < cap; k++) h = (h ^ buf[k]) * 1099511628211ull; hashes[0] = h; }
    jpeg_finish_decompress(&c);
  }
  jpeg_destroy_decompress(&c);
  free(buf);
  free(rowp);
  return NULL;
}

int main(int argc, char **argv)
{
  int T, t, i;
  pthread_t th[256];
  double t0, t1, tw;
  unsigned long long px = 0;
  if (argc < 5) { fprintf(stderr, "usage: djpeg_bench THREADS FILES_PER_THREAD ROWS_PER_CALL FILE...\n"); return 2; }
  T = atoi(argv[1]); NPER = atoi(argv[2]); ROWS = atoi(argv[3]); NFILES = argc - 4;
  if (T < 1 || T > 256 || NPER < 1) return 2;
  files = (unsigned char **)malloc(sizeof(*files) * NFILES);
  sizes = (size_t *)malloc(sizeof(*sizes) * NFILES);
  for (i = 0; i < NFILES; i++) {
    FILE *f = fopen(argv[4 + i], "rb");
    long n;
    if (!f) { perror(argv[4 + i]); return 3; }
    fseek(f, 0, SEEK_END); n = ftell(f); fseek(f, 0, SEEK_SET);
    files[i] = (unsigned char *)malloc((size_t)n);
    if (fread(files[i], 1, (size_t)n, f) != (size_t)n) return 3;
    sizes[i] = (size_t)n;
    fclose(f);
  }
  {   /* one untimed file per thread first: library load, device context, encoder construction */
    const int keep = NPER;
    NPER = 1; tw = now();
    for (t = 0; t < T; t++) pthread_create(&th[t], NULL, worker, (void *)(long)t);
    for (t = 0; t < T; t++) pthread_join(th[t], NULL);
    tw = now() - tw; NPER = keep;
    memset(pixels, 0, sizeof pixels);
  }
  t0 = now();
  for (t = 0; t < T; t++) pthread_create(&th[t], NULL, worker, (void *)(long)t);
  for (t = 0; t < T; t++) pthread_join(th[t], NULL);
  t1 = now();
  for (t = 0; t < T; t++) px += pixels[t];
  printf("{\"threads\": %d, \"files\": %d, \"distinct_files\": %d, \"rows_per_call\": %d, \"first_file_s\": %.3f, \"seconds\": %.4f, \"files_per_s\": %.2f, "
         "\"mpix_per_s\": %.1f, \"fnv1a_first\": \"%016llx\"}\n", T, T * NPER, NFILES, ROWS, tw, t1 - t0, T * NPER / (t1 - t0), (double)px / (t1 - t0) / 1e6, hashes[0]);
  return 0;
}
