// TEST INFRASTRUCTURE.  The arithmetic decoder of the product (mozjpeg_amd/csrc/mjh_arith_decoder.h, compiled here for the
// host: a "vector register" is an array of 64 ints) in three steps:
//   1. the product's host-compiled coder (mjh_arith_coder.h) writes random scans -- whole blocks, DC first, AC first, DC
//      refinement, AC refinement, with restarts, conditioning drawn at random and table numbers 0..3;
//   2. the host-compiled decoder reads every restart segment back;
//   3. the coefficients must be what was coded; the decoder's final statistics bins must be the coder's; and the decoder
//      must agree with a plain restatement of jdarith.c (flat arrays of state bytes, bit-by-bit renormalisation, the
//      reference's bin numbering) in the coefficients, every bin, the registers and the number of bytes consumed.
// Then: segments cut short (continued with zeros, never read past the buffer: every segment sits in a heap block of exactly
// its size), and hand-made streams that drive every overflow branch (JWRN_ARITH_BAD_CODE) -- the product and the
// restatement must reach the "bad code" state together.  Exit status 0 = identical everywhere.
// usage: arith_decoder_check [scans] [seed]      (an optional -fsanitize=address,undefined build is made by hand)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define MJH_ARI_HOST 1
#include "../../mozjpeg_amd/csrc/mjh_arith_decoder.h"

static unsigned rnd_state = 1;
static unsigned rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }
static void fill(ari_reg &r, int v) { for (int i = 0; i < 64; i++) r.v[i] = v; }

// the bytes of one restart segment: de-stuffed as arith_decode reads them, zeros from the end (= the marker behind it) onward
struct Bytes {
  const unsigned char *p;
  size_t len, pos, zeros;
  bool hit;
  int raw() { if (pos >= len) { hit = true; return -1; } return p[pos++]; }
  int next()
  {
    if (!hit) {
      int d = raw();
      if (d == 0xFF) { do d = raw(); while (d == 0xFF); if (d == 0) d = 0xFF; else hit = true; }
      if (!hit) return d;
    }
    zeros++;
    return 0;
  }
};

// ---- plain restatement of jdarith.c ---------------------------------------------------------------------------------------
struct Ref {
  unsigned char ac[4][256], dc[4][64], fixed_bin;
  long c, a;
  int ct;
  int last_dc[4], ctx[4];
  int L[4], U[4], K[4];
  Bytes in;
  void start() { memset(ac, 0, sizeof ac); memset(dc, 0, sizeof dc); fixed_bin = 113; c = 0; a = 0; ct = -16; for (int i = 0; i < 4; i++) last_dc[i] = ctx[i] = 0; }
  int decode(unsigned char *st)
  {
    while (a < 0x8000L) {
      if (--ct < 0) {
        c = (c << 8) | in.next();
        if ((ct += 8) < 0) if (++ct == 0) a = 0x8000L;
      }
      a <<= 1;
    }
    int sv = *st;
    const long qe = mjh_ari_qe[sv & 0x7F];
    const int nl = mjh_ari_nlps[sv & 0x7F], nm = mjh_ari_nmps[sv & 0x7F];
    long temp = a - qe;
    a = temp;
    temp <<= ct;
    if (c >= temp) {
      c -= temp;
      if (a < qe) { a = qe; *st = (unsigned char)((sv & 0x80) ^ nm); }
      else { a = qe; *st = (unsigned char)((sv & 0x80) ^ nl); sv ^= 0x80; }
    } else if (a < 0x8000L) {
      if (a < qe) { *st = (unsigned char)((sv & 0x80) ^ nl); sv ^= 0x80; }
      else *st = (unsigned char)((sv & 0x80) ^ nm);
    }
    return sv >> 7;
  }
  bool dc_diff(int tbl, int ci)
  {
    unsigned char *st = dc[tbl] + ctx[ci];
    if (!decode(st)) { ctx[ci] = 0; return true; }
    const int sign = decode(st + 1);
    st += 2 + sign;
    int m = decode(st);
    if (m) { st = dc[tbl] + 20; while (decode(st)) { if ((m <<= 1) == 0x8000) { ct = -1; return false; } st++; } }
    if (m < (int)((1L << L[tbl]) >> 1)) ctx[ci] = 0;
    else if (m > (int)((1L << U[tbl]) >> 1)) ctx[ci] = 12 + sign * 4;
    else ctx[ci] = 4 + sign * 4;
    int v = m;
    st += 14;
    while (m >>= 1) if (decode(st)) v |= m;
    v += 1; if (sign) v = -v;
    last_dc[ci] = (last_dc[ci] + v) & 0xffff;
    return true;
  }
  bool ac_first(int tbl, short *blk, int Ss, int Se, int Al)
  {
    for (int k = Ss; k <= Se; k++) {
      unsigned char *st = ac[tbl] + 3 * (k - 1);
      if (decode(st)) break;
      while (!decode(st + 1)) { st += 3; k++; if (k > Se) { ct = -1; return false; } }
      const int sign = decode(&fixed_bin);
      st += 2;
      int m = decode(st);
      if (m && decode(st)) {
        m <<= 1;
        st = ac[tbl] + (k <= K[tbl] ? 189 : 217);
        while (decode(st)) { if ((m <<= 1) == 0x8000) { ct = -1; return false; } st++; }
      }
      int v = m;
      st += 14;
      while (m >>= 1) if (decode(st)) v |= m;
      v += 1; if (sign) v = -v;
      blk[k] = (short)((unsigned)v << Al);
    }
    return true;
  }
  bool ac_refine(int tbl, short *blk, int Ss, int Se, int Al)
  {
    const int p1 = 1 << Al, m1 = -p1;
    int kex = Se;
    while (kex > 0 && !blk[kex]) kex--;
    for (int k = Ss; k <= Se; k++) {
      unsigned char *st = ac[tbl] + 3 * (k - 1);
      if (k > kex && decode(st)) break;
      for (;;) {
        if (blk[k]) { if (decode(st + 2)) blk[k] = (short)(blk[k] + (blk[k] < 0 ? m1 : p1)); break; }
        if (decode(st + 1)) { blk[k] = (short)(decode(&fixed_bin) ? m1 : p1); break; }
        st += 3; k++;
        if (k > Se) { ct = -1; return false; }
      }
    }
    return true;
  }
};

// ---- the product's coder and decoder on the host ------------------------------------------------------------------------------
static void tables(ari_reg tab[2])
{
  for (int lane = 0; lane < 64; lane++) {
    tab[0].v[lane] = (int)(((unsigned)mjh_ari_qe[lane] << 16) | ((unsigned)mjh_ari_nmps[lane] << 8) | (unsigned)mjh_ari_nlps[lane]);
    const int j = lane + 64 < 114 ? lane + 64 : 113;
    tab[1].v[lane] = (int)(((unsigned)mjh_ari_qe[j] << 16) | ((unsigned)mjh_ari_nmps[j] << 8) | (unsigned)mjh_ari_nlps[j]);
  }
}
struct Enc {           // (the coder keeps two tables of each class: a table number's parity picks one)
  AriModel M;
  AriCoder A;
  int last_dc[4], ctx[4];
  std::vector<unsigned char> buf;
  Enc() : buf(1 << 22) { tables(M.tab); fill(M.coef, 0); A.lane0 = true; A.out = buf.data(); A.pos = 0; A.cap = (unsigned)buf.size(); restart(); }
  void restart()
  {
    for (int t = 0; t < 2; t++) { for (int r = 0; r < 4; r++) fill(M.ac[t][r], ARI_BIN_RESET); fill(M.dc[t], ARI_BIN_RESET); }
    for (int r = 0; r < 4; r++) fill(M.cur[r], ARI_BIN_RESET);
    fill(M.dcur, ARI_BIN_RESET);
    for (int i = 0; i < 4; i++) last_dc[i] = ctx[i] = 0;
    A.reset();
  }
};
struct Dec {
  AdModel M;
  AriDecoder<Bytes> A;
  int last_dc[4], ctx[4];
  Dec()
  {
    tables(M.tab); fill(M.coef, 0);
    for (int t = 0; t < 4; t++) { for (int r = 0; r < 4; r++) fill(M.ac[t][r], ARI_BIN_RESET); fill(M.dc[t], ARI_BIN_RESET); }
    for (int r = 0; r < 4; r++) fill(M.cur[r], ARI_BIN_RESET);
    fill(M.dcur, ARI_BIN_RESET);
    for (int i = 0; i < 4; i++) last_dc[i] = ctx[i] = 0;
  }
};

struct Scan {
  int mode;            // 0 whole blocks, 1 DC first, 2 DC refine, 3 AC first, 4 AC refine
  int ncomp, ta[4], td[4], Ss, Se, Ah, Al;
  int L[4], U[4], K[4];
};

static int last_nonzero(const short *blk, int Se) { int k = Se; while (k > 0 && !blk[k]) k--; return k; }

// one restart segment `seg` (a heap block of exactly its size) holding nblk blocks of scan S from block index b0 on; prev: what
// the earlier scans left (refinements), out: the decoded blocks.  Both decoders run; returns the number of disagreements.
static long decode_segment(const Scan &S, const std::vector<unsigned char> &seg, int b0, int nblk, const short *prev, short *out,
                           Dec &D, int *bad_out, size_t *consumed, const char *what, int scan)
{
  Ref R;
  R.start();
  for (int t = 0; t < 4; t++) { R.L[t] = S.L[t]; R.U[t] = S.U[t]; R.K[t] = S.K[t]; }
  R.in = Bytes{ seg.data(), seg.size(), 0, 0, false };
  D.A.src = Bytes{ seg.data(), seg.size(), 0, 0, false };
  D.A.start();
  std::vector<short> rblk((size_t)nblk * 64);
  long bad = 0;
  for (int b = 0; b < nblk; b++) {
    const int ci = (b0 + b) % S.ncomp, ta = S.ta[ci], td = S.td[ci];
    short *rb = &rblk[(size_t)b * 64], *ob = out + (size_t)b * 64;
    const bool refine = S.mode == 2 || S.mode == 4;
    for (int k = 0; k < 64; k++) rb[k] = refine ? prev[(size_t)b * 64 + k] : 0;
    // the restatement (the reference's "if error do nothing" for everything but DC refinement)
    if (S.mode == 2) { if (R.decode(&R.fixed_bin)) rb[0] = (short)(rb[0] | (1 << S.Al)); }
    else if (R.ct != -1) {
      if (S.mode == 0) { if (R.dc_diff(td, ci)) { rb[0] = (short)R.last_dc[ci]; R.ac_first(ta, rb, 1, 63, 0); } }
      else if (S.mode == 1) { if (R.dc_diff(td, ci)) rb[0] = (short)((unsigned)R.last_dc[ci] << S.Al); }
      else if (S.mode == 3) R.ac_first(ta, rb, S.Ss, S.Se, S.Al);
      else R.ac_refine(ta, rb, S.Ss, S.Se, S.Al);
    }
    // the product (a chain stops at the first bad code: the image is discarded)
    if (!D.A.bad) {
      for (int k = 0; k < 64; k++) D.M.coef.v[k] = refine ? prev[(size_t)b * 64 + k] : 0;
      for (int r = 0; r < 4; r++) D.M.cur[r] = D.M.ac[ta][r];
      D.M.dcur = D.M.dc[td];
      D.M.dc_lo = (int)((1L << S.L[td]) >> 1); D.M.dc_hi = (int)((1L << S.U[td]) >> 1); D.M.ac_k = S.K[ta];
      int big = 0;
      short before[64];
      for (int k = 0; k < 64; k++) before[k] = (short)D.M.coef.v[k];
      ad_block(D.A, D.M, S.mode == 0, S.mode == 0 ? 0 : S.Ss, S.mode == 0 ? 63 : S.Se, S.Ah, S.Al, last_nonzero(before, S.mode == 0 ? 63 : S.Se), D.last_dc[ci], D.ctx[ci], &big);
      for (int r = 0; r < 4; r++) D.M.ac[ta][r] = D.M.cur[r];
      D.M.dc[td] = D.M.dcur;
      for (int k = 0; k < 64; k++) ob[k] = (short)D.M.coef.v[k];
      if (!D.A.bad && memcmp(ob, rb, 128)) { if (bad < 3) printf("scan %d (%s): block %d differs from the restatement\n", scan, what, b0 + b); bad++; }
    }
    if ((D.A.bad != 0) != (R.ct == -1)) { printf("scan %d (%s): bad-code state differs at block %d\n", scan, what, b0 + b); bad++; break; }
    if (D.A.bad) break;
  }
  if (!D.A.bad) {
    if ((unsigned)R.c != D.A.c || (unsigned)R.a != D.A.a || R.ct != D.A.ct) { bad++; printf("scan %d (%s): registers differ\n", scan, what); }
    if (R.in.pos != D.A.src.pos || R.in.zeros != D.A.src.zeros) { bad++; printf("scan %d (%s): bytes consumed differ (%zu+%zu vs %zu+%zu)\n", scan, what, R.in.pos, R.in.zeros, D.A.src.pos, D.A.src.zeros); }
    for (int t = 0; t < 4; t++) {
      for (int b = 0; b < 245; b++) {
        const int w = b < 189 ? D.M.ac[t][b % 3].v[b / 3] : D.M.ac[t][ARI_X].v[b - 189];
        if ((w & 0xFF) != R.ac[t][b] || (unsigned)(w >> 16) != mjh_ari_qe[w & 0x7F] || (w & 0xFF00)) { bad++; printf("scan %d (%s): AC bin %d of table %d differs\n", scan, what, b, t); break; }
      }
      for (int b = 0; b < 64; b++) {
        const int w = D.M.dc[t].v[b];
        if ((w & 0xFF) != R.dc[t][b] || (unsigned)(w >> 16) != mjh_ari_qe[w & 0x7F]) { bad++; printf("scan %d (%s): DC bin %d of table %d differs\n", scan, what, b, t); break; }
      }
    }
  }
  *bad_out = D.A.bad;
  *consumed = D.A.src.pos;
  return bad;
}

static void make_block(short *blk, int dens, int amp, int dcamp)
{
  for (int k = 0; k < 64; k++) {
    int v = 0;
    if ((int)(rnd() % 100) < dens / (1 + k / 8)) {
      v = 1 + (int)(rnd() % (unsigned)amp);
      if (rnd() % 7 == 0) v = 1 + (int)(rnd() % 2);
      if (rnd() & 1) v = -v;
    }
    blk[k] = (short)v;
  }
  blk[0] = (short)((int)(rnd() % (unsigned)(2 * dcamp + 1)) - dcamp);
}

static const char *const kNames[5] = { "whole blocks", "DC first", "DC refine", "AC first", "AC refine" };

static Scan draw_scan(int scan)
{
  Scan S;
  memset(&S, 0, sizeof S);
  S.mode = (int)(rnd() % 5);
  S.ncomp = S.mode <= 2 ? 1 + (int)(rnd() % 3) : 1;
  // table numbers 0..3; the coder keeps one table per parity, so components that differ in their table differ in its parity
  for (int i = 0; i < 4; i++) { S.ta[i] = (int)(rnd() & 3); S.td[i] = (int)(rnd() & 3); }
  for (int i = 1; i < 4; i++) {
    for (int j = 0; j < i; j++) {
      if ((S.ta[i] & 1) == (S.ta[j] & 1)) S.ta[i] = S.ta[j];
      if ((S.td[i] & 1) == (S.td[j] & 1)) S.td[i] = S.td[j];
    }
  }
  const bool def = scan % 3 == 0;
  for (int t = 0; t < 4; t++) {
    S.L[t] = def ? 0 : (int)(rnd() % 6); S.U[t] = def ? 1 : S.L[t] + (int)(rnd() % (unsigned)(16 - S.L[t])); S.K[t] = def ? 5 : 1 + (int)(rnd() % 63);
  }
  S.Ss = 1; S.Se = 63;
  if (S.mode == 1) { S.Ss = S.Se = 0; S.Al = (int)(rnd() % 3); }
  if (S.mode == 2) { S.Ss = S.Se = 0; S.Ah = 1 + (int)(rnd() % 2); S.Al = S.Ah - 1; }
  if (S.mode >= 3) { S.Ss = 1 + (int)(rnd() % 40); S.Se = S.Ss + (int)(rnd() % (unsigned)(64 - S.Ss)); S.Al = (int)(rnd() % 3); }
  if (S.mode == 4) S.Ah = S.Al + 1;
  return S;
}

int main(int argc, char **argv)
{
  const int nscans = argc > 1 ? atoi(argv[1]) : 400;
  rnd_state = argc > 2 ? (unsigned)atoi(argv[2]) : 12345u;
  long bad = 0, blocks = 0, cut = 0, overflow = 0;
  // ---- 1..3: what the coder wrote is read back
  for (int scan = 0; scan < nscans && bad < 10; scan++) {
    const Scan S = draw_scan(scan);
    const int nblocks = 1 + (int)(rnd() % 300), dens = 5 + (int)(rnd() % 95), amp = 1 << (rnd() % 11), dcamp = 1 << (1 + rnd() % 11);
    const int ri = (rnd() % 3 == 0) ? S.ncomp * (1 + (int)(rnd() % 20)) : nblocks;      // blocks per restart segment (whole MCUs)
    std::vector<short> full((size_t)nblocks * 64), prev((size_t)nblocks * 64, 0), want((size_t)nblocks * 64, 0), got((size_t)nblocks * 64, 0);
    for (int b = 0; b < nblocks; b++) make_block(&full[(size_t)b * 64], dens, amp, dcamp);
    // what the earlier scans left (point transform by Ah) and what this scan makes of it
    for (int b = 0; b < nblocks; b++) {
      for (int k = 0; k < 64; k++) {
        const int v = full[(size_t)b * 64 + k], av = v < 0 ? -v : v;
        const bool in_band = S.mode == 0 || (k >= S.Ss && k <= S.Se);
        int p = 0, w = 0;
        if (k == 0) { p = S.Ah ? (v >> S.Ah) * (1 << S.Ah) : 0; w = (v >> S.Al) * (1 << S.Al); }
        else { p = S.Ah ? (v < 0 ? -((av >> S.Ah) << S.Ah) : ((av >> S.Ah) << S.Ah)) : 0; w = v < 0 ? -((av >> S.Al) << S.Al) : ((av >> S.Al) << S.Al); }
        if (S.mode == 0) { p = 0; w = v; }
        if (!in_band && S.mode != 4) p = w = 0;
        if (S.mode == 4 && !in_band) { p = w = (k == 0 ? 0 : (int)(rnd() % 3) - 1); }      // other bands: the EOBx search passes them (jdarith.c:462); they stay
        prev[(size_t)b * 64 + k] = (short)((S.mode == 2 || S.mode == 4) ? p : 0);
        want[(size_t)b * 64 + k] = (short)(in_band || S.mode == 4 ? w : 0);
      }
    }
    Enc E;
    for (int s0 = 0; s0 < nblocks; s0 += ri) {
      const int nb = nblocks - s0 < ri ? nblocks - s0 : ri;
      E.restart();
      const unsigned start = E.A.pos;
      for (int b = s0; b < s0 + nb; b++) {
        const short *blk = &full[(size_t)b * 64];
        const int ci = b % S.ncomp, ta = S.ta[ci] & 1, td = S.td[ci] & 1;
        int ke = 0, kex = 0;
        if (S.mode == 0 || S.mode >= 3) {
          const int al = S.mode == 0 ? 0 : S.Al, ah = S.mode == 0 ? 0 : S.Ah, se = S.mode == 0 ? 63 : S.Se;
          for (int k = 1; k <= se; k++) { const int av = blk[k] < 0 ? -blk[k] : blk[k]; if (av >> al) ke = k; }
          if (ah) for (int k = 1; k <= ke; k++) { const int av = blk[k] < 0 ? -blk[k] : blk[k]; if (av >> ah) kex = k; }
        }
        for (int k = 0; k < 64; k++) E.M.coef.v[k] = blk[k];
        for (int r = 0; r < 4; r++) E.M.cur[r] = E.M.ac[ta][r];
        E.M.dcur = E.M.dc[td];
        E.M.dc_lo = (int)((1L << S.L[S.td[ci]]) >> 1); E.M.dc_hi = (int)((1L << S.U[S.td[ci]]) >> 1); E.M.ac_k = S.K[S.ta[ci]];
        switch (S.mode) {
          case 0: ari_dc(E.A, E.M, E.last_dc[ci], E.ctx[ci], blk[0]); ari_ac_first(E.A, E.M, 1, 63, 0, ke); break;
          case 1: ari_dc(E.A, E.M, E.last_dc[ci], E.ctx[ci], blk[0] >> S.Al); break;
          case 2: E.A.encode<ARI_F>(E.M, 0, (blk[0] >> S.Al) & 1); break;
          case 3: ari_ac_first(E.A, E.M, S.Ss, S.Se, S.Al, ke); break;
          default: ari_ac_refine(E.A, E.M, S.Ss, S.Se, S.Ah, S.Al, ke, kex); break;
        }
        for (int r = 0; r < 4; r++) E.M.ac[ta][r] = E.M.cur[r];
        E.M.dc[td] = E.M.dcur;
      }
      E.A.finish();
      const std::vector<unsigned char> seg(E.buf.begin() + start, E.buf.begin() + E.A.pos);      // exactly its size
      Dec D;
      int isbad = 0;
      size_t used = 0;
      bad += decode_segment(S, seg, s0, nb, &prev[(size_t)s0 * 64], &got[(size_t)s0 * 64], D, &isbad, &used, kNames[S.mode], scan);
      if (isbad) { bad++; printf("scan %d (%s): a bad code in what the coder wrote\n", scan, kNames[S.mode]); }
      if (used > seg.size()) { bad++; printf("scan %d: read past the segment\n", scan); }
      // the decoder's bins against the coder's (a coder table serves every number of its parity)
      for (int i = 0; i < S.ncomp && !isbad; i++) {
        const int ta = S.ta[i], td = S.td[i];
        if (S.mode == 0 || S.mode >= 3)
          for (int r = 0; r < 4; r++) if (memcmp(D.M.ac[ta][r].v, E.M.ac[ta & 1][r].v, sizeof(D.M.ac[ta][r].v))) { bad++; printf("scan %d (%s): AC bins of kind %d differ from the coder's\n", scan, kNames[S.mode], r); break; }
        if (S.mode <= 1 && memcmp(D.M.dc[td].v, E.M.dc[td & 1].v, sizeof(D.M.dc[td].v))) { bad++; printf("scan %d (%s): DC bins differ from the coder's\n", scan, kNames[S.mode]); }
      }
      // ---- the same segment cut short: zeros follow, nothing behind the heap block is read, both decoders agree
      if (seg.size() > 2 && scan % 4 == 0) {
        const std::vector<unsigned char> shorter(seg.begin(), seg.begin() + (long)(seg.size() - 1 - rnd() % (seg.size() / 2)));
        std::vector<short> tmp((size_t)nb * 64);
        Dec D2;
        bad += decode_segment(S, shorter, s0, nb, &prev[(size_t)s0 * 64], tmp.data(), D2, &isbad, &used, "cut short", scan);
        if (used > shorter.size()) { bad++; printf("scan %d: read past the shortened segment\n", scan); }
        cut++;
      }
      blocks += nb;
    }
    if (S.mode != 4) {       // (AC refinement of a band leaves the other bands as they were: compared inside its band)
      if (memcmp(want.data(), got.data(), want.size() * 2)) { bad++; printf("scan %d (%s): the coefficients are not what was coded\n", scan, kNames[S.mode]); }
    } else {
      for (int b = 0; b < nblocks && bad < 10; b++) for (int k = S.Ss; k <= S.Se; k++)
        if (want[(size_t)b * 64 + k] != got[(size_t)b * 64 + k]) { bad++; printf("scan %d (AC refine): block %d position %d is %d, coded %d\n", scan, b, k, got[(size_t)b * 64 + k], want[(size_t)b * 64 + k]); break; }
    }
  }
  // ---- the overflow branches (JWRN_ARITH_BAD_CODE), each driven by a hand-made stream: the coder's own primitive writes a decision
  // sequence that no block stands for -- "no end of block, coefficient zero" until the band is passed (spectral overflow
  // :359 / :489 / :587), "one more magnitude bit" until 0x8000 (:292 / :550 DC, :376 / :604 AC).  Both decoders must reach the
  // state at the same block, and the product must name the branch.
  {
    struct Case { int mode, why; const char *what; };
    const Case cases[] = {
      { 0, AD_BAD_DC, "DC magnitude overflow, whole blocks (:550)" }, { 1, AD_BAD_DC, "DC magnitude overflow, DC first (:292)" },
      { 0, AD_BAD_SPECTRAL, "spectral overflow, whole blocks (:587)" }, { 0, AD_BAD_AC, "AC magnitude overflow, whole blocks (:604)" },
      { 3, AD_BAD_SPECTRAL, "spectral overflow, AC first (:359)" }, { 3, AD_BAD_AC, "AC magnitude overflow, AC first (:376)" },
      { 4, AD_BAD_SPECTRAL, "spectral overflow, AC refine (:489)" },
    };
    for (const Case &c : cases) {
      Scan S;
      memset(&S, 0, sizeof S);
      S.mode = c.mode; S.ncomp = 1;
      for (int t = 0; t < 4; t++) { S.L[t] = 0; S.U[t] = 1; S.K[t] = 5; }
      S.Ss = c.mode <= 1 ? 0 : 1 + (int)(rnd() % 20); S.Se = c.mode == 1 ? 0 : 63;
      if (c.mode == 4) { S.Ah = 1; S.Al = 0; }
      Enc E;
      E.M.dc_lo = 0; E.M.dc_hi = 1; E.M.ac_k = 5;
      if (c.mode == 0 && c.why != AD_BAD_DC) E.A.encode<ARI_D>(E.M, 0, 0);      // a DC difference of zero in front of the AC part
      const int first = c.mode == 0 ? 1 : S.Ss;
      if (c.why == AD_BAD_DC) {
        E.A.encode<ARI_D>(E.M, 0, 1); E.A.encode<ARI_D>(E.M, 1, 0); E.A.encode<ARI_D>(E.M, 2, 1);
        for (int i = 0; i < 15; i++) E.A.encode<ARI_D>(E.M, 20 + i, 1);
      } else if (c.why == AD_BAD_SPECTRAL) {
        E.A.encode<ARI_E>(E.M, first - 1, 0);
        for (int k = first; k <= 63; k++) E.A.encode<ARI_Z>(E.M, k - 1, 0);
      } else {
        E.A.encode<ARI_E>(E.M, first - 1, 0); E.A.encode<ARI_Z>(E.M, first - 1, 1); E.A.encode<ARI_F>(E.M, 0, 1);
        E.A.encode<ARI_M>(E.M, first - 1, 1); E.A.encode<ARI_M>(E.M, first - 1, 1);
        for (int i = 0; i < 15; i++) E.A.encode<ARI_X>(E.M, (first <= 5 ? 0 : 28) + i, 1);
      }
      E.A.finish();
      const std::vector<unsigned char> seg(E.buf.begin(), E.buf.begin() + E.A.pos);
      std::vector<short> prev(64 * 4, 0), out(64 * 4, 0);
      Dec D;
      int isbad = 0;
      size_t used = 0;
      bad += decode_segment(S, seg, 0, 4, prev.data(), out.data(), D, &isbad, &used, c.what, -1);
      if (used > seg.size()) { bad++; printf("%s: read past the segment\n", c.what); }
      if (isbad != c.why) { bad++; printf("%s: the stream reached state %d, not the branch\n", c.what, isbad); }
      else overflow++;
    }
    // random garbage: whatever happens, it happens in both decoders alike
    for (int g = 0; g < 200 && bad < 10; g++) {
      const Scan S = draw_scan(g + 1);
      std::vector<unsigned char> seg(1 + rnd() % 200);
      for (unsigned char &b : seg) b = (unsigned char)(rnd() % 5 == 0 ? 0xFF : rnd());
      std::vector<short> prev(64 * 40), out(64 * 40, 0);
      for (short &v : prev) v = (short)(rnd() % 4 == 0 ? ((int)(rnd() % 5) - 2) * (1 << S.Ah) : 0);
      Dec D;
      int isbad = 0;
      size_t used = 0;
      bad += decode_segment(S, seg, 0, 40, prev.data(), out.data(), D, &isbad, &used, "garbage", g);
      if (used > seg.size()) { bad++; printf("garbage %d: read past the segment\n", g); }
    }
  }
  printf("%ld blocks in %d scans, %ld segments cut short, %ld of 7 overflow branches reached: %s\n", blocks, nscans, cut, overflow, bad ? "MISMATCH" : "identical");
  return bad ? 1 : 0;
}
