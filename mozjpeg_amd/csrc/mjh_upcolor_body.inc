// mjh_upcolor_body.inc -- the 4 pixels of one lane of k_upcolor and k_upcolor_region (mjh_idct.hip): upsampling, colour conversion
// and the store, included as text so that both kernels hold one copy and k_upcolor's machine code is what it was.  It reads: P,
// pl (the image's planes), x0 (the first of the 4 pixels), y (the row of the whole image the samples are taken at), yo (the
// output row), img, pixels.
  unsigned px[4][3];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int x = x0 + i < P.W ? x0 + i : P.W - 1;      // (the pad of the last group: an in-range position, its bytes mean nothing)
    const int a = up_sample(P.c[0], pl + P.c[0].plane_off, x, y);
    int r = a, g = a, b = a;
    if (P.ncomp == 3) {
      const int c1 = up_sample(P.c[1], pl + P.c[1].plane_off, x, y), c2 = up_sample(P.c[2], pl + P.c[2].plane_off, x, y);
      if (P.conv == MJH_CC_YCC_RGB) {                  // ycc_rgb_convert with the tables of build_ycc_rgb_table (jdcolor.c:215-251), SCALEBITS 16
        const int cb = c1 - 128, cr = c2 - 128;
        r = clamp255(a + ((91881 * cr + 32768) >> 16));
        g = clamp255(a + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
        b = clamp255(a + ((116130 * cb + 32768) >> 16));
      } else if (P.conv == MJH_CC_RGB_GRAY) {           // rgb_gray_convert (build_rgb_y_table jdcolor.c:306-327)
        r = g = b = (19595 * a + 38470 * c1 + 7471 * c2 + 32768) >> 16;
      } else { g = c1; b = c2; }
    }
    px[i][0] = (unsigned)r; px[i][1] = (unsigned)g; px[i][2] = (unsigned)b;
  }
  uint8_t *out = pixels + (size_t)img * P.image_stride + (size_t)yo * P.row_pitch + (size_t)x0 * P.px_size;
  if (P.px_size == 1) {
    *reinterpret_cast<unsigned *>(out) = px[0][0] | (px[1][0] << 8) | (px[2][0] << 16) | (px[3][0] << 24);
  } else if (P.px_size == 4) {
    uint4 v;
    unsigned w[4];
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = 0xFFFFFFFFu ^ ((0xFFu ^ px[i][0]) << (8 * P.off_r)) ^ ((0xFFu ^ px[i][1]) << (8 * P.off_g)) ^ ((0xFFu ^ px[i][2]) << (8 * P.off_b));
    v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
    *reinterpret_cast<uint4 *>(out) = v;
  } else {
    // twelve bytes: byte j of pixel i is the colour whose offset is j
    unsigned w[3] = { 0u, 0u, 0u };
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const unsigned p24 = (px[i][0] << (8 * P.off_r)) | (px[i][1] << (8 * P.off_g)) | (px[i][2] << (8 * P.off_b));
      const unsigned long long sh = (unsigned long long)p24 << (8 * (3 * i & 3));     // pixel i starts at byte 3 i: word 3 i / 4, byte 3 i % 4
      w[(3 * i) >> 2] |= (unsigned)sh;
      if (((3 * i) >> 2) + 1 < 3) w[((3 * i) >> 2) + 1] |= (unsigned)(sh >> 32);
    }
    unsigned *o32 = reinterpret_cast<unsigned *>(out);
    o32[0] = w[0]; o32[1] = w[1]; o32[2] = w[2];
  }
