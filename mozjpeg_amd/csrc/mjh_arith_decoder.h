// mjh_arith_decoder.h -- the QM decoder (ITU-T T.81 D.2; jdarith.c:114-191) and the five decision sequences of the JPEG
// statistics models as jdarith.c:235-630 runs them, the mirror image of mjh_arith_coder.h and written in its form: ONE wave is
// one scalar machine.  Every lane executes this code with wave-uniform values (the decoder's registers live in SGPRs, its
// branches are scalar jumps); the statistics live in vector registers used as 64-entry RAMs:
//   * one bin per lane, the bin's word carries the Qe of its state (Qe << 16 | MPS << 7 | index): the common decision -- the
//     more probable symbol, no renormalisation -- is one register read, a subtraction, a shift and two compares;
//   * the AC bins of a table are four registers by KIND (end-of-block / zero / first magnitude by position, the magnitude
//     tail by its offset from 189), the DC bins one register; four conditioning tables of each class (Td / Ta 0..3);
//   * the tables of the block being decoded are BOUND to fixed registers around the block (ad_bind / ad_unbind);
//   * the fixed 0.5 bin (state 113) is a constant, never a register access;
//   * renormalisation shifts by the whole distance at once (count-leading-zeros) and takes its bytes from SRC::next().
// The decoded block lands in AdModel::coef: lane k = zig-zag position k.  SRC supplies the de-stuffed bytes of the restart
// segment and zeros from its end onward (arith_decode :126-145: meeting a marker is legal, zeros follow).
// The file compiles for the host (MJH_ARI_HOST): tests/native/arith_decoder_check.cpp reads back what the host-compiled coder
// wrote.
#ifndef MJH_ARITH_DECODER_H
#define MJH_ARITH_DECODER_H
#include "mjh_arith_coder.h"      // ari_reg, rl / wl, the bin kinds, ARI_BIN_RESET, the probability table

enum { AD_BAD_DC = 1, AD_BAD_SPECTRAL = 2, AD_BAD_AC = 3 };      // which overflow: DC magnitude, end of band passed, AC magnitude

struct AdModel {       // vector registers as RAM
  ari_reg ac[4][4];    // AC statistics of conditioning table 0..3 by kind (ARI_E .. ARI_X), one bin per lane
  ari_reg dc[4];       // DC statistics of table 0..3: lane = jdarith.c's bin index (< 49)
  ari_reg cur[4];      // the bound AC table
  ari_reg dcur;        // the bound DC table
  ari_reg tab[2];      // T.81 Table D.3 as in AriModel
  ari_reg coef;        // the block being decoded: lane k = coefficient k (zig-zag)
  int dc_lo, dc_hi, ac_k;      // conditioning of the bound tables: (1 << L) >> 1, (1 << U) >> 1 (jdarith.c:300-302), Kx (:373)
};

template <class SRC>
struct AriDecoder {    // jdarith.c:28-46, all wave-uniform
  unsigned c, a;
  int ct;
  int bad;             // the reference's ct == -1 (JWRN_ARITH_BAD_CODE): AD_BAD_DC / AD_BAD_SPECTRAL / AD_BAD_AC, 0 = none
  SRC src;
  // start_pass / process_restart leave ct = -16 and the first arith_decode reads two bytes (:123-153); every chain decodes at
  // least one decision, so the two bytes are read here
  ARI_MFN void start()
  {
    const unsigned b0 = (unsigned)src.next();
    const unsigned b1 = (unsigned)src.next();
    c = (b0 << 8) | b1; a = 0x10000u; ct = 0; bad = 0;
  }
  // arith_decode on bin `lane` of kind KIND (known at every call site)
  template <int KIND>
  ARI_MFN int decode(AdModel &M, int lane)
  {
    if (a < 0x8000u) {           // renormalisation and data input (D.2.6): n shifts, a byte whenever the counter runs out
      const int n = __builtin_clz(a) - 16;
      a <<= n;
      ct -= n;
      while (ct < 0) { c = (c << 8) | (unsigned)src.next(); ct += 8; }
    }
    unsigned w;
    if (KIND == ARI_F) w = ((unsigned)0x5a1d << 16) | 113u;
    else if (KIND == ARI_D) w = (unsigned)rl(M.dcur, lane);
    else w = (unsigned)rl(M.cur[KIND == ARI_D || KIND == ARI_F ? 0 : KIND], lane);
    const unsigned qe = w >> 16, sv = w & 0xFFu;
    const int mps = (int)(sv >> 7);
    a -= qe;
    const unsigned t = a << ct;
    const bool upper = c >= t;                      // the code lies in the LPS sub-interval
    if (!upper && a >= 0x8000u) return mps;
    const bool lt = a < qe;
    const bool lps = upper != lt;                   // conditional exchange (D.2.4 / D.2.5)
    c -= upper ? t : 0u;
    a = upper ? qe : a;
    if (KIND != ARI_F) {
      const int s = (int)(sv & 0x7Fu);
      const unsigned lo = (unsigned)rl(M.tab[0], s & 63), hi = (unsigned)rl(M.tab[1], s & 63);
      const unsigned e = s < 64 ? lo : hi;
      const unsigned ns = (sv & 0x80u) ^ ((lps ? e : e >> 8) & 0xFFu);
      const int s2 = (int)(ns & 0x7Fu);
      const unsigned lo2 = (unsigned)rl(M.tab[0], s2 & 63), hi2 = (unsigned)rl(M.tab[1], s2 & 63);
      const int nw = (int)(((s2 < 64 ? lo2 : hi2) & 0xFFFF0000u) | ns);
      if (KIND == ARI_D) M.dcur = wl(nw, lane, M.dcur);
      else M.cur[KIND == ARI_D || KIND == ARI_F ? 0 : KIND] = wl(nw, lane, M.cur[KIND == ARI_D || KIND == ARI_F ? 0 : KIND]);
    }
    return mps ^ (lps ? 1 : 0);
  }
};

ARI_FN int ad_coef(const AdModel &M, int k) { return (int)(short)rl(M.coef, k); }
ARI_FN void ad_put(AdModel &M, int k, int v) { M.coef = wl((int)(short)v, k, M.coef); }

// Decode_DC_DIFF (Figures F.19 - F.24; jdarith.c:276-313 / :534-571) with the bound DC table: the running value, 16 bits.
// Returns 0 or AD_BAD_DC
template <class D>
ARI_FN int ad_dc(D &A, AdModel &M, int &last_dc, int &ctx)
{
  int st = ctx;
  if (A.template decode<ARI_D>(M, st) == 0) { ctx = 0; return 0; }
  const int sign = A.template decode<ARI_D>(M, st + 1);
  st += 2 + sign;
  int m = A.template decode<ARI_D>(M, st);
  if (m) {
    st = 20;
    while (A.template decode<ARI_D>(M, st)) {
      if ((m <<= 1) == 0x8000) return AD_BAD_DC;
      st++;
    }
  }
  if (m < M.dc_lo) ctx = 0;
  else if (m > M.dc_hi) ctx = 12 + sign * 4;
  else ctx = 4 + sign * 4;
  int v = m;
  st += 14;
  while (m >>= 1) if (A.template decode<ARI_D>(M, st)) v |= m;
  v += 1;
  if (sign) v = -v;
  last_dc = (last_dc + v) & 0xffff;
  return 0;
}

// Decode_AC_coefficients (Figure F.20; decode_mcu_AC_first jdarith.c:353-392, with Ss = 1, Se = 63, Al = 0 the AC part of
// decode_mcu :581-620) into the block, which holds zeros there.  *big: the largest magnitude stored.  Returns 0 or which overflow
template <class D>
ARI_FN int ad_ac_first(D &A, AdModel &M, int Ss, int Se, int Al, int *big)
{
  for (int k = Ss; k <= Se; k++) {
    int p = k - 1;
    if (A.template decode<ARI_E>(M, p)) break;
    while (A.template decode<ARI_Z>(M, p) == 0) {
      p++; k++;
      if (k > Se) return AD_BAD_SPECTRAL;
    }
    const int sign = A.template decode<ARI_F>(M, 0);
    int m = A.template decode<ARI_M>(M, p), x = 0;
    if (m) {
      if (A.template decode<ARI_M>(M, p)) {
        m <<= 1;
        x = k <= M.ac_k ? 0 : 28;
        while (A.template decode<ARI_X>(M, x)) {
          if ((m <<= 1) == 0x8000) return AD_BAD_AC;
          x++;
        }
      }
    }
    int v = m;
    x += 14;
    while (m >>= 1) if (A.template decode<ARI_X>(M, x)) v |= m;
    v += 1;
    const int mag = v << Al;
    if (mag > *big) *big = mag;
    if (sign) v = -v;
    ad_put(M, k, (int)((unsigned)v << Al));
  }
  return 0;
}

// decode_mcu_AC_refine jdarith.c:458-494 on the block the earlier scans left; kex: its last non-zero position in 1..Se (:462)
template <class D>
ARI_FN int ad_ac_refine(D &A, AdModel &M, int Ss, int Se, int Al, int kex)
{
  const int p1 = 1 << Al, m1 = -1 * (1 << Al);
  for (int k = Ss; k <= Se; k++) {
    int p = k - 1;
    if (k > kex) if (A.template decode<ARI_E>(M, p)) break;
    for (;;) {
      const int cv = ad_coef(M, k);
      if (cv) {
        if (A.template decode<ARI_M>(M, p)) ad_put(M, k, cv + (cv < 0 ? m1 : p1));
        break;
      }
      if (A.template decode<ARI_Z>(M, p)) {
        ad_put(M, k, A.template decode<ARI_F>(M, 0) ? m1 : p1);
        break;
      }
      p++; k++;
      if (k > Se) return AD_BAD_SPECTRAL;
    }
  }
  return 0;
}

// One block of a scan with the bound tables.  whole: decode_mcu (DC + AC 1..63); else by (Ss, Ah): decode_mcu_DC_first,
// decode_mcu_DC_refine, decode_mcu_AC_first, decode_mcu_AC_refine.  The block holds zeros (whole, first scans) or what the
// earlier scans left (refinements).  An overflow sets A.bad and leaves the block as far as it got.
template <class D>
ARI_FN void ad_block(D &A, AdModel &M, bool whole, int Ss, int Se, int Ah, int Al, int kex, int &last_dc, int &ctx, int *big)
{
  int why = 0;
  if (whole) {
    why = ad_dc(A, M, last_dc, ctx);
    if (!why) { ad_put(M, 0, last_dc); why = ad_ac_first(A, M, 1, 63, 0, big); }
  } else if (Ss == 0 && Ah == 0) {
    why = ad_dc(A, M, last_dc, ctx);
    if (!why) ad_put(M, 0, (int)((unsigned)last_dc << Al));
  } else if (Ss == 0) {
    if (A.template decode<ARI_F>(M, 0)) ad_put(M, 0, ad_coef(M, 0) | (1 << Al));
  } else if (Ah == 0) why = ad_ac_first(A, M, Ss, Se, Al, big);
  else why = ad_ac_refine(A, M, Ss, Se, Al, kex);
  if (why) A.bad = why;
}
#endif
