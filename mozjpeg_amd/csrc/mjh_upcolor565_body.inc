// mjh_upcolor565_body.inc -- the 4 pixels of one lane of k_upcolor_565 and k_upcolor_565_region (mjh_idct.hip), included as text
// (see mjh_upcolor_body.inc, whose names it reads, and dither).  y picks the row of the dither matrix: the row of the whole image.
  const unsigned dm = dither ? kDither565[y & 3] : 0u;
  unsigned p16[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int x = x0 + i < P.W ? x0 + i : P.W - 1;      // (the pad of the last group, as in k_upcolor)
    const int d = (int)((dm >> (8 * i)) & 0xFFu);       // x0 is a multiple of 4: x & 3 = i
    const int a = up_sample(P.c[0], pl + P.c[0].plane_off, x, y);
    int r, g, b;
    if (P.ncomp == 3) {
      const int c1 = up_sample(P.c[1], pl + P.c[1].plane_off, x, y), c2 = up_sample(P.c[2], pl + P.c[2].plane_off, x, y);
      if (P.conv == MJH_CC_YCC_RGB) {                  // the tables of build_ycc_rgb_table, as k_upcolor
        const int cb = c1 - 128, cr = c2 - 128;
        r = a + ((91881 * cr + 32768) >> 16);
        g = a + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
        b = a + ((116130 * cb + 32768) >> 16);
      } else { r = a; g = c1; b = c2; }                // rgb_rgb565(D)_convert
      r = clamp255(r + d); g = clamp255(g + (d >> 1)); b = clamp255(b + d);
    } else r = g = b = clamp255(a + d);                // gray_rgb565(D)_convert
    p16[i] = (((unsigned)r << 8) & 0xF800u) | (((unsigned)g << 3) & 0x7E0u) | ((unsigned)b >> 3);      // PACK_SHORT_565_LE
  }
  uint2 v;
  v.x = p16[0] | (p16[1] << 16); v.y = p16[2] | (p16[3] << 16);
  *reinterpret_cast<uint2 *>(pixels + (size_t)img * P.image_stride + (size_t)yo * P.row_pitch + (size_t)x0 * 2) = v;
