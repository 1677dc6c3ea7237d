// mjh_idct8_body.inc -- one block through both passes of jpeg_idct_islow (jidctint.c:173-413): the body of k_idct and of
// k_idct_region<false> (mjh_idct.hip), included as text so that both kernels hold one copy of the arithmetic and k_idct's
// machine code is what it was.  It reads: in (the block's entry of zig-zag plane 0), q (the 64 multipliers), cc.kstride, and
// for the address of the block's samples b (the lane's block), cc.wib, cc.pw, cc.plane_off, planes, img, C.planes_per_image.
  int ws[64];
  // pass 1: columns, results scaled up by 2^PASS1_BITS (2)
#pragma unroll
  for (int c = 0; c < 8; c++) {
    int x[8];
#pragma unroll
    for (int r = 0; r < 8; r++) x[r] = (int)in[(size_t)kZigOfNat[r * 8 + c] * cc.kstride] * q[r * 8 + c];
    long long o[8];
    idct8(x, o);
#pragma unroll
    for (int r = 0; r < 8; r++) ws[r * 8 + c] = (int)((o[r] + 1024) >> 11);
  }
  // pass 2: rows; descale by 2^(CONST_BITS + PASS1_BITS + 3), then the range limit with the sample's centre added
  const int by = b / cc.wib, bx = b - by * cc.wib;
  uint8_t *out = planes + (size_t)img * C.planes_per_image + cc.plane_off + (size_t)(by * 8) * cc.pw + (size_t)bx * 8;
#pragma unroll
  for (int r = 0; r < 8; r++) {
    int x[8];
#pragma unroll
    for (int c = 0; c < 8; c++) x[c] = ws[r * 8 + c];
    long long o[8];
    idct8(x, o);
    unsigned s[8];
#pragma unroll
    for (int c = 0; c < 8; c++) s[c] = idct_range_limit((int)((o[c] + (1 << 17)) >> 18));
    uint2 v;
    v.x = s[0] | (s[1] << 8) | (s[2] << 16) | (s[3] << 24);
    v.y = s[4] | (s[5] << 8) | (s[6] << 16) | (s[7] << 24);
    *reinterpret_cast<uint2 *>(out + (size_t)r * cc.pw) = v;
  }
