// mjh_idct8_ifast_body.inc -- one block through both passes of jpeg_idct_ifast (jidctfst.c:170-368): the body of k_idct_ifast
// and of k_idct_region<true> (mjh_idct.hip), included as text (see mjh_idct8_body.inc, whose names it reads).
  unsigned ws[64];
  // pass 1: columns; the multipliers carry the 2^PASS1_BITS the workspace is scaled up by
#pragma unroll
  for (int c = 0; c < 8; c++) {
    unsigned x[8], o[8];
#pragma unroll
    for (int r = 0; r < 8; r++) x[r] = (unsigned)(int)in[(size_t)kZigOfNat[r * 8 + c] * cc.kstride] * (unsigned)q[r * 8 + c];
    idct8_ifast(x, o);
#pragma unroll
    for (int r = 0; r < 8; r++) ws[r * 8 + c] = o[r];
  }
  // pass 2: rows; a plain shift by PASS1_BITS + 3, then the range limit with the sample's centre added
  const int by = b / cc.wib, bx = b - by * cc.wib;
  uint8_t *out = planes + (size_t)img * C.planes_per_image + cc.plane_off + (size_t)(by * 8) * cc.pw + (size_t)bx * 8;
#pragma unroll
  for (int r = 0; r < 8; r++) {
    unsigned x[8], o[8];
#pragma unroll
    for (int c = 0; c < 8; c++) x[c] = ws[r * 8 + c];
    idct8_ifast(x, o);
    unsigned s[8];
#pragma unroll
    for (int c = 0; c < 8; c++) s[c] = idct_range_limit((int)o[c] >> 5);
    uint2 v;
    v.x = s[0] | (s[1] << 8) | (s[2] << 16) | (s[3] << 24);
    v.y = s[4] | (s[5] << 8) | (s[6] << 16) | (s[7] << 24);
    *reinterpret_cast<uint2 *>(out + (size_t)r * cc.pw) = v;
  }
