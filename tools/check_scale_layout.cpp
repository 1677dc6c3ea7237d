// check_scale_layout.cpp -- stand-alone check of the host arithmetic of a scaled decode call (mozjpeg_amd/csrc/mjh_scale_layout.h):
// the IDCT size of a fraction, the size of every component, and the layout of the sample planes of a call whose components
// outgrow the full-size planes.  Build and run under the host sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Imozjpeg_amd/csrc tools/check_scale_layout.cpp -o check_scale_layout
// It writes every plane of every geometry into a heap buffer of exactly the size the layout asks for (the small geometries), so
// an offset or a stride that is too small is an AddressSanitizer report; the 65500 x 65500 header is checked by arithmetic alone.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "mjh_scale_layout.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

struct Geo { const char *name; int W, H, ncomp, h[4], v[4]; };

static long ceil_div(long a, long b) { return (a + b - 1) / b; }

static void check_geometry(const Geo &g, int k, bool raw, int batch, bool touch)
{
  int maxh = 1, maxv = 1, wib[4], hib[4], ss[4];
  for (int c = 0; c < g.ncomp; c++) { if (g.h[c] > maxh) maxh = g.h[c]; if (g.v[c] > maxv) maxv = g.v[c]; }
  bool any_big = false;
  for (int c = 0; c < g.ncomp; c++) {
    wib[c] = (int)ceil_div((long)g.W * g.h[c], (long)maxh * 8);
    hib[c] = (int)ceil_div((long)g.H * g.v[c], (long)maxv * 8);
    ss[c] = raw ? k : mjh_scaled_size(k, g.h[c], g.v[c], maxh, maxv);
    CHECK(ss[c] >= k && ss[c] <= 16 && (ss[c] == k || ss[c] / 2 < 8) && ss[c] % k == 0, "%s k %d comp %d: size %d", g.name, k, c, ss[c]);
    // the upsampling factors the colour kernels divide by are whole numbers
    CHECK((maxh * k) % (g.h[c] * ss[c]) == 0 && (maxv * k) % (g.v[c] * ss[c]) == 0, "%s k %d comp %d: fractional expansion", g.name, k, c);
    any_big |= ss[c] > 8;
  }
  MjhPlaneLayout L;
  mjh_plane_layout(g.ncomp, wib, hib, ss, &L);
  CHECK(L.own == any_big, "%s k %d: own %d", g.name, k, (int)L.own);
  for (int c = 0; c < g.ncomp; c++) {
    CHECK(L.pitch[c] % 4 == 0 && L.pitch[c] >= wib[c] * ss[c] && L.pitch[c] < wib[c] * ss[c] + 4, "%s k %d comp %d: pitch %d", g.name, k, c, L.pitch[c]);
    if (!L.own) CHECK((size_t)L.pitch[c] * hib[c] * ss[c] <= (size_t)wib[c] * 8 * hib[c] * 8, "%s k %d comp %d: outgrows the full-size plane", g.name, k, c);
  }
  if (!L.own) return;
  size_t end = 0;
  for (int c = 0; c < g.ncomp; c++) {
    const size_t bytes = (size_t)L.pitch[c] * (size_t)hib[c] * (size_t)ss[c];
    CHECK(L.off[c] % 16 == 0 && L.off[c] >= end, "%s k %d comp %d: offset %zu overlaps (%zu)", g.name, k, c, L.off[c], end);
    end = L.off[c] + bytes;
  }
  CHECK(L.stride % 16 == 0 && L.stride >= end, "%s k %d: stride %zu < %zu", g.name, k, L.stride, end);
  const size_t total = mjh_plane_layout_bytes(&L, batch);
  CHECK(total == L.stride * (size_t)batch, "%s k %d: %zu bytes for %d images", g.name, k, total, batch);
  if (!touch) return;
  // every byte a kernel writes or reads, in a buffer of exactly `total` bytes: the last word of the last row of the last
  // component of the last image is the one closest to the end
  uint8_t *buf = (uint8_t *)malloc(total);
  CHECK(buf != NULL, "malloc(%zu)", total);
  if (!buf) return;
  memset(buf, 0, total);
  for (int i = 0; i < batch; i++)
    for (int c = 0; c < g.ncomp; c++)
      for (int y = 0; y < hib[c] * ss[c]; y++) {
        uint8_t *row = buf + (size_t)i * L.stride + L.off[c] + (size_t)y * L.pitch[c];
        for (int x = 0; x < L.pitch[c]; x += 4) { uint32_t w; memcpy(&w, row + x, 4); CHECK(w == 0, "%s k %d: planes overlap", g.name, k); w = 0x01010101u; memcpy(row + x, &w, 4); }
      }
  free(buf);
}

int main()
{
  // resolve_scale: the smallest k with num * 8 <= denom * k, else 16
  for (int k = 1; k <= 16; k++) CHECK(mjh_scale_idct_size(k, 8) == k, "%d/8", k);
  const int fr[][3] = { {1, 3, 3}, {2, 3, 6}, {3, 5, 5}, {5, 4, 10}, {17, 10, 14}, {3, 1, 16}, {1, 5, 2}, {1, 100, 1}, {9, 10, 8}, {1000, 1, 16},
                        {2147483647, 2147483647, 8}, {1, 2147483647, 1}, {2147483647, 1, 16} };
  for (const auto &f : fr) CHECK(mjh_scale_idct_size(f[0], f[1]) == f[2], "%d/%d -> %d", f[0], f[1], mjh_scale_idct_size(f[0], f[1]));
  for (int k = 1; k <= 16; k++) CHECK(mjh_scale_size_is_classic(k) == (k == 1 || k == 2 || k == 4 || k == 8), "classic %d", k);
  // the sizes the issue names
  for (int k : { 3, 5, 6, 7 }) {
    CHECK(mjh_scaled_size(k, 2, 2, 2, 2) == k && mjh_scaled_size(k, 1, 1, 2, 2) == 2 * k, "4:2:0 at %d", k);
    CHECK(mjh_scaled_size(k, 2, 1, 2, 2) == k, "2x2,1x1,2x1 at %d: third component", k);
  }
  for (int k = 9; k <= 16; k++) CHECK(mjh_scaled_size(k, 1, 1, 2, 2) == k, "4:2:0 at %d", k);
  const Geo geos[] = {
    { "revert 4:2:0", 227, 149, 3, { 2, 1, 1 }, { 2, 1, 1 } }, { "s_mixed", 227, 149, 3, { 2, 1, 2 }, { 2, 1, 1 } }, { "gray", 227, 149, 1, { 1 }, { 1 } },
    { "2x1", 227, 149, 3, { 2, 1, 1 }, { 1, 1, 1 } }, { "1x2", 227, 149, 3, { 1, 1, 1 }, { 2, 1, 1 } }, { "1x1", 1, 1, 3, { 2, 1, 1 }, { 2, 1, 1 } },
    { "17x9 2x1", 17, 9, 3, { 2, 1, 1 }, { 1, 1, 1 } }, { "8x8 2x1", 8, 8, 3, { 2, 1, 1 }, { 1, 1, 1 } }, { "444", 128, 128, 3, { 1, 1, 1 }, { 1, 1, 1 } },
    { "absurd 45x37", 45, 37, 3, { 2, 1, 2 }, { 2, 1, 1 } }, { "ycck 4:2:0", 227, 149, 4, { 2, 1, 1, 2 }, { 2, 1, 1, 2 } }, { "1080p", 1920, 1080, 3, { 2, 1, 1 }, { 2, 1, 1 } },
    { "4:1:1", 227, 149, 3, { 4, 1, 1 }, { 1, 1, 1 } },
  };
  for (const Geo &g : geos)
    for (int k = 1; k <= 16; k++)
      for (int raw = 0; raw < 2; raw++)
        for (int batch : { 1, 3 }) check_geometry(g, k, raw != 0, batch, g.W <= 256);
  const Geo huge = { "65500 x 65500", 65500, 65500, 3, { 2, 1, 1 }, { 2, 1, 1 } };
  for (int k = 1; k <= 16; k++)
    for (int raw = 0; raw < 2; raw++) check_geometry(huge, k, raw != 0, 64, false);
  {
    // at 2/1 that frame is 3 planes of up to 131008 x 131008 samples: beyond 32 bits, inside size_t; and a batch that is not
    int wib[3] = { 8188, 4094, 4094 }, hib[3] = { 8188, 4094, 4094 }, ss[3] = { 16, 16, 16 };
    MjhPlaneLayout L;
    mjh_plane_layout(3, wib, hib, ss, &L);
    CHECK(L.own && L.off[1] == (size_t)131008 * 131008 && L.stride == (size_t)131008 * 131008 + 2 * ((size_t)65504 * 65504), "the 65500 x 65500 layout: %zu %zu", L.off[1], L.stride);
    CHECK(mjh_plane_layout_bytes(&L, 64) == L.stride * 64, "64 such images");
    CHECK(mjh_plane_layout_bytes(&L, 2147483647) == 0 && mjh_plane_layout_bytes(&L, 0) == 0, "a product beyond size_t is refused, not wrapped");
  }
  printf(failures ? "check_scale_layout: %d FAILED\n" : "check_scale_layout: ok\n", failures);
  return failures != 0;
}
