// mjh_jpeg_parse.cpp -- host side of the re-compression path that needs no device: the marker segments of a JPEG file
// (jdmarker.c) and the parameters jpeg_copy_critical_parameters derives from them (jctrans.c:75-171).  Nothing here decodes
// a Huffman symbol: the entropy-coded data is only searched for 0xFF to find where a scan ends.
#include <initializer_list>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "../../include/mozjpeg_hip.h"
#include "mjh_internal.h"

typedef struct mjh_jpeg_arith_cond MjhArithCond;      // (the public header spells the type with its tag: the call bears the same name)
int mjh_transform_plan(const mjh_jpeg_info *f, const mjh_transform *t, MjhXformPlan *g);   // (also used by mjh_encoder.cpp)
int mjh_internal_fail(int code, const char *msg);

static int pfail(int code, const char *fmt, ...)
{
  char buf[400];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return mjh_internal_fail(code, buf);
}

static const int kNatural[64] = {
  0,  1,  8, 16,  9,  2,  3, 10, 17, 24, 32, 25, 18, 11,  4,  5,
  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,  6,  7, 14, 21, 28,
  35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
  58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63 };

// The marker walk behind mjh_jpeg_probe (accept = 0, ex = nullptr) and mjh_jpeg_probe_ex.  A progressive file (SOF2, accepted with
// MJH_SRC_PROGRESSIVE) leaves its scans in ex[] and info->num_scans at 0; its scan script is checked as start_pass_phuff_decoder
// checks it (jdphuff.c:91-144), except that what the reference only warns about (JWRN_BOGUS_PROGRESSION) refuses the file: the
// device decoder then never meets a refinement of something that was not sent.  A lossless file (SOF3, accepted with
// MJH_SRC_LOSSLESS) is reported the same way: its scans in ex[] with Ss = the predictor and Al = the point transform, checked as
// start_pass_lossless (jdlossls.c:249-258) and start_input_pass (jddiffct.c:104-110) check them.
#define MJH_SRC_ALL (MJH_SRC_PROGRESSIVE | MJH_SRC_LOSSLESS | MJH_SRC_ARITHMETIC)
static_assert(offsetof(mjh_jpeg_scan_ex, Ss) == sizeof(mjh_jpeg_scan), "mjh_jpeg_scan_ex begins with the fields of mjh_jpeg_scan");
// saves(mode, m): jcopy_markers_setup (transupp.c:2312-2336) -- does copy mode `mode` save marker code m
static bool copy_mode_saves(int mode, int m)
{
  if (m == 0xFE) return mode != MJH_COPY_NONE && mode != MJH_COPY_ICC;
  if (m < 0xE0 || m > 0xEF) return false;
  if (mode == MJH_COPY_ALL) return true;
  if (mode == MJH_COPY_ALL_EXCEPT_ICC) return m != 0xE2;
  return mode == MJH_COPY_ICC && m == 0xE2;
}

// copy_mode / saved: the walk also lists the COM / APPn segments that mode saves (mjh_jpeg_markers), wherever they stand
// cond: the arithmetic conditioning in force at every SOS, in file order (mjh_jpeg_arith_cond)
static int probe_walk(const void *jpeg, size_t size, unsigned accept, mjh_jpeg_info *info, mjh_jpeg_scan_ex *ex, int cap, int *num_ex,
                      int copy_mode = MJH_COPY_NONE, std::vector<mjh_jpeg_marker> *saved = nullptr, std::vector<MjhArithCond> *cond = nullptr)
{
  const uint8_t *d = (const uint8_t *)jpeg;
  memset(info, 0, sizeof(*info));
  if (num_ex) *num_ex = 0;
  bool prog = false, lossless = false, arith = false;
  const bool take_arith = (accept & MJH_SRC_ARITHMETIC) != 0;
  int dac_L[16], dac_U[16], dac_K[16];      // (jdmarker.c:203-207: L 0, U 1, K 5 at every SOI)
  for (int t = 0; t < 16; t++) { dac_L[t] = 0; dac_U[t] = 1; dac_K[t] = 5; }
  if (cond) cond->clear();
  int nex = 0;
  int coef_bits[MJH_MAX_COMPS][64];
  for (int c = 0; c < MJH_MAX_COMPS; c++) for (int k = 0; k < 64; k++) coef_bits[c][k] = -1;
  if (size < 4 || d[0] != 0xFF || d[1] != 0xD8) return pfail(MJH_EINVAL, "Not a JPEG file: no SOI marker (JERR_NO_SOI)");
  // the tables in force (DHT segments redefine them between scans)
  static thread_local uint8_t hbits[8][17], hvals[8][256];
  int hdef = 0;
  unsigned ri = 0;
  bool saw_sof = false, saw_eoi = false;
  int comp_scans[MJH_MAX_COMPS] = { 0, 0, 0, 0 };
  size_t pos = 2;
  while (!saw_eoi) {
    // next_marker (jdmarker.c:910-955): any number of 0xFF fill bytes, then the code
    if (pos >= size) return pfail(MJH_EINVAL, "Premature end of JPEG file (JWRN_JPEG_EOF)");
    if (d[pos] != 0xFF) return pfail(MJH_EINVAL, "Corrupt JPEG data: extraneous bytes before marker at offset %zu (JWRN_EXTRANEOUS_DATA)", pos);
    while (pos < size && d[pos] == 0xFF) pos++;
    if (pos >= size) return pfail(MJH_EINVAL, "Premature end of JPEG file (JWRN_JPEG_EOF)");
    const int m = d[pos++];
    if (m == 0) return pfail(MJH_EINVAL, "Corrupt JPEG data: extraneous bytes before marker at offset %zu (JWRN_EXTRANEOUS_DATA)", pos);
    if (m == 0xD9) { saw_eoi = true; break; }
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;              // TEM, a stray RSTn: no parameters
    if (m == 0xD8) return pfail(MJH_EINVAL, "Invalid JPEG file structure: two SOI markers (JERR_SOI_DUPLICATE)");
    if (pos + 2 > size) return pfail(MJH_EINVAL, "Premature end of JPEG file (JWRN_JPEG_EOF)");
    const size_t len = ((size_t)d[pos] << 8) | d[pos + 1];
    if (len < 2) return pfail(MJH_EINVAL, "Bogus marker length (JERR_BAD_LENGTH)");
    if (pos + len > size) return pfail(MJH_EINVAL, "Premature end of JPEG file (JWRN_JPEG_EOF)");
    const uint8_t *s = d + pos + 2;
    const size_t n = len - 2;
    pos += len;
    if (saved && copy_mode_saves(copy_mode, m)) saved->push_back(mjh_jpeg_marker{ m, (size_t)(s - d), (unsigned)n });
    switch (m) {
    case 0xC0: case 0xC1: case 0xC2: case 0xC3: case 0xC9: case 0xCA: case 0xCB:
    case 0xC5: case 0xC6: case 0xC7: case 0xCD: case 0xCE: case 0xCF: {
      if (m == 0xC2 && !(accept & MJH_SRC_PROGRESSIVE))
        return pfail(MJH_EUNSUPPORTED, "progressive source file (SOF2): only sequential Huffman-coded files are decoded on the device");
      if (m == 0xC3 && !(accept & MJH_SRC_LOSSLESS)) return pfail(MJH_EUNSUPPORTED, "lossless source file (SOF3): jpeg_copy_critical_parameters refuses it as well (JERR_NOTIMPL, jctrans.c:83)");
      if ((m == 0xC9 || m == 0xCA || m == 0xCB) && !take_arith) return pfail(MJH_EUNSUPPORTED, "arithmetic-coded source file (SOF%d)", m - 0xC0);
      if (m == 0xCB) return pfail(MJH_EUNSUPPORTED, "arithmetic-coded lossless source file (SOF11): SOF9 and SOF10 are decoded");
      if (m == 0xCA && !(accept & MJH_SRC_PROGRESSIVE))
        return pfail(MJH_EUNSUPPORTED, "progressive arithmetic-coded source file (SOF10): MJH_SRC_PROGRESSIVE is not set next to MJH_SRC_ARITHMETIC");
      if (m != 0xC0 && m != 0xC1 && m != 0xC2 && m != 0xC3 && m != 0xC9 && m != 0xCA) return pfail(MJH_EUNSUPPORTED, "Unsupported JPEG process: SOF type 0x%02x (JERR_SOF_UNSUPPORTED)", m);
      prog = m == 0xC2 || m == 0xCA;
      arith = m == 0xC9 || m == 0xCA;
      lossless = m == 0xC3;
      if (saw_sof) return pfail(MJH_EINVAL, "Invalid JPEG file structure: two SOF markers (JERR_SOF_DUPLICATE)");
      if (n < 6) return pfail(MJH_EINVAL, "Bogus marker length (JERR_BAD_LENGTH)");
      info->sof_type = m - 0xC0;
      info->data_precision = s[0];
      info->image_height = (s[1] << 8) | s[2];
      info->image_width = (s[3] << 8) | s[4];
      info->num_components = s[5];
      if (info->image_height == 0) return pfail(MJH_EUNSUPPORTED, "image height 0 in the frame header: a DNL marker would define it, which is not supported");
      if (info->image_width <= 0 || info->num_components <= 0) return pfail(MJH_EINVAL, "Empty JPEG image (JERR_EMPTY_IMAGE)");
      if (n != 6 + 3 * (size_t)info->num_components) return pfail(MJH_EINVAL, "Bogus marker length (JERR_BAD_LENGTH)");
      if (lossless) {                  // initial_setup (jdinput.c:60-66)
        if (info->data_precision != 8 && info->data_precision != 12 && info->data_precision != 16)
          return pfail(MJH_EINVAL, "Unsupported JPEG data precision %d (JERR_BAD_PRECISION)", info->data_precision);
      } else
      if (info->data_precision != 8) return pfail(MJH_EUNSUPPORTED, "%d-bit source file: only 8-bit samples", info->data_precision);
      if (lossless && info->num_components == 4)
        return pfail(MJH_EUNSUPPORTED, "4 components in a lossless source file: 1 or 3 are supported (four components are decoded from DCT files only)");
      if (info->num_components != 1 && info->num_components != 3 && info->num_components != 4)
        return pfail(MJH_EUNSUPPORTED, "%d components in the source file: 1, 3 or 4 are supported", info->num_components);
      for (int c = 0; c < info->num_components; c++) {
        info->component_id[c] = s[6 + 3 * c];
        info->h_samp_factor[c] = s[7 + 3 * c] >> 4;
        info->v_samp_factor[c] = s[7 + 3 * c] & 15;
        info->quant_tbl_no[c] = s[8 + 3 * c];
        if (info->h_samp_factor[c] < 1 || info->h_samp_factor[c] > 4 || info->v_samp_factor[c] < 1 || info->v_samp_factor[c] > 4)
          return pfail(MJH_EINVAL, "Bogus sampling factors (JERR_BAD_SAMPLING)");
        if (info->quant_tbl_no[c] > 3) return pfail(MJH_EINVAL, "Quantization table 0x%02x was not defined (JERR_NO_QUANT_TABLE)", info->quant_tbl_no[c]);
      }
      if (lossless)
        for (int c = 0; c < info->num_components; c++)
          if (info->h_samp_factor[c] != 1 || info->v_samp_factor[c] != 1)
            return pfail(MJH_EUNSUPPORTED, "subsampled components in a lossless source file (component %d is sampled %dx%d): only 1x1 is decoded", c, info->h_samp_factor[c], info->v_samp_factor[c]);
      saw_sof = true;
      break;
    }
    case 0xC4: {          // DHT (get_dht jdmarker.c:455-533): any number of tables
      size_t o = 0;
      while (o < n) {
        if (n - o < 17) return pfail(MJH_EINVAL, "Bogus marker length (JERR_BAD_LENGTH)");
        const int idx = s[o];
        int count = 0;
        for (int i = 1; i <= 16; i++) count += s[o + i];
        if (count > 256 || (size_t)count > n - o - 17) return pfail(MJH_EINVAL, "Bogus Huffman table definition (JERR_BAD_HUFF_TABLE)");
        if ((idx & 0xEF) > 3) return pfail(MJH_EINVAL, "Bogus DHT index %d (JERR_DHT_INDEX)", idx);
        const int slot = 2 * (idx & 3) + ((idx & 0x10) ? 1 : 0);
        hbits[slot][0] = 0;
        memcpy(&hbits[slot][1], s + o + 1, 16);
        memset(hvals[slot], 0, 256);
        memcpy(hvals[slot], s + o + 17, (size_t)count);
        hdef |= 1 << slot;
        o += 17 + (size_t)count;
      }
      break;
    }
    case 0xCC: {          // DAC (get_dac jdmarker.c:388-428): any number of (Tc|Tb, value) pairs
      if (!take_arith) return pfail(MJH_EUNSUPPORTED, "arithmetic-coding conditioning (DAC) in the source file");
      if (n & 1) return pfail(MJH_EINVAL, "Bogus marker length (JERR_BAD_LENGTH)");
      for (size_t o = 0; o < n; o += 2) {
        const int idx = s[o], val = s[o + 1];
        if (idx >= 32) return pfail(MJH_EINVAL, "Bogus DAC index %d (JERR_DAC_INDEX)", idx);
        if (idx >= 16) dac_K[idx - 16] = val;
        else {
          dac_L[idx] = val & 15; dac_U[idx] = val >> 4;
          if (dac_L[idx] > dac_U[idx]) return pfail(MJH_EINVAL, "Bogus DAC value 0x%x (JERR_DAC_VALUE)", val);
        }
      }
      break;
    }
    case 0xDB: {          // DQT (get_dqt jdmarker.c:536-620)
      size_t o = 0;
      while (o < n) {
        const int pq = s[o] >> 4, t = s[o] & 15;
        if (t > 3) return pfail(MJH_EINVAL, "Bogus DQT index %d (JERR_DQT_INDEX)", t);
        const size_t need = pq ? 128 : 64;
        if (n - o - 1 < need) return pfail(MJH_EINVAL, "Bogus marker length (JERR_BAD_LENGTH)");
        uint16_t q[64];
        for (int i = 0; i < 64; i++) q[kNatural[i]] = pq ? (uint16_t)((s[o + 1 + 2 * i] << 8) | s[o + 2 + 2 * i]) : s[o + 1 + i];
        if (info->num_scans + nex > 0 && ((info->quant_defined >> t) & 1) && memcmp(q, info->quantval[t], sizeof(q)) != 0)
          return pfail(MJH_EINVAL, "Cannot transcode due to multiple use of quantization table %d (JERR_MISMATCHED_QUANT_TABLE)", t);
        memcpy(info->quantval[t], q, sizeof(q));
        info->quant_defined |= 1 << t;
        o += 1 + need;
      }
      break;
    }
    case 0xDC: return pfail(MJH_EUNSUPPORTED, "DNL marker in the source file");
    case 0xDD:
      if (n != 2) return pfail(MJH_EINVAL, "Bogus marker length (JERR_BAD_LENGTH)");
      ri = ((unsigned)s[0] << 8) | s[1];
      break;
    case 0xE0:            // get_interesting_appn / examine_app0 (jdmarker.c:623-690)
      if (n >= 14 && s[0] == 0x4A && s[1] == 0x46 && s[2] == 0x49 && s[3] == 0x46 && s[4] == 0) {
        info->saw_JFIF_marker = 1;
        info->JFIF_major_version = s[5];
        info->JFIF_minor_version = s[6];
        info->density_unit = s[7];
        info->X_density = (s[8] << 8) | s[9];
        info->Y_density = (s[10] << 8) | s[11];
      }
      break;
    case 0xEE:            // examine_app14 (jdmarker.c:693-718)
      if (n >= 12 && s[0] == 0x41 && s[1] == 0x64 && s[2] == 0x6F && s[3] == 0x62 && s[4] == 0x65) {
        info->saw_Adobe_marker = 1;
        info->Adobe_transform = s[11];
      }
      break;
    case 0xDA: {          // SOS (get_sos jdmarker.c:312-393) + the entropy-coded segment behind it
      if (!saw_sof) return pfail(MJH_EINVAL, "Invalid JPEG file structure: SOS before SOF (JERR_SOS_NO_SOF)");
      if (n < 1) return pfail(MJH_EINVAL, "Bogus marker length (JERR_BAD_LENGTH)");
      const int nc = s[0];
      if (n != (size_t)(2 * nc + 4) || nc < 1 || nc > MJH_MAX_COMPS) return pfail(MJH_EINVAL, "Bogus marker length (JERR_BAD_LENGTH)");
      if (!prog && !lossless && info->num_scans >= MJH_MAX_FILE_SCANS) return pfail(MJH_EINVAL, "more than %d scans in a sequential file", MJH_MAX_FILE_SCANS);
      // a progressive or lossless file's scan is built in a scratch record and copied into ex[] (mjh_jpeg_scan_ex begins with the fields
      // of mjh_jpeg_scan); scans beyond the room the caller gave are walked and checked all the same, for the count in the refusal
      static thread_local mjh_jpeg_scan scratch;
      const bool to_ex = prog || lossless;
      if (to_ex) memset(&scratch, 0, sizeof(scratch));
      mjh_jpeg_scan *sc = to_ex ? &scratch : &info->scans[info->num_scans];
      const uint8_t *t = s + 1 + 2 * nc;
      const int Ss = t[0], Se = t[1], Ah = t[2] >> 4, Al = t[2] & 15;
      if (prog) {                      // start_pass_phuff_decoder (jdphuff.c:91-121)
        bool bad = false;
        if (Ss == 0) { if (Se != 0) bad = true; }
        else if (Ss > Se || Se >= 64 || nc != 1) bad = true;
        if (Ah != 0 && Al != Ah - 1) bad = true;
        if (Al > 13) bad = true;
        if (bad) return pfail(MJH_EINVAL, "Invalid progressive/lossless parameters Ss=%d Se=%d Ah=%d Al=%d (JERR_BAD_PROGRESSION)", Ss, Se, Ah, Al);
      }
      if (lossless) {                  // start_pass_lossless (jdlossls.c:249-258); start_input_pass (jddiffct.c:104-110), every MCU row W MCUs
        if (Ss < 1 || Ss > 7 || Se != 0 || Ah != 0 || Al >= info->data_precision)
          return pfail(MJH_EINVAL, "Invalid progressive/lossless parameters Ss=%d Se=%d Ah=%d Al=%d (JERR_BAD_PROGRESSION)", Ss, Se, Ah, Al);
        if (ri % (unsigned)info->image_width != 0)
          return pfail(MJH_EINVAL, "Invalid restart interval %u; must be an integer multiple of the number of MCUs in an MCU row (%d) (JERR_BAD_RESTART)", ri, info->image_width);
      }
      sc->comps_in_scan = nc;
      for (int i = 0; i < nc; i++) {
        const int id = s[1 + 2 * i];
        int ci = -1;
        for (int c = 0; c < info->num_components; c++) if (info->component_id[c] == id) { ci = c; break; }
        if (ci < 0) return pfail(MJH_EINVAL, "Invalid component ID %d in SOS (JERR_BAD_COMPONENT_ID)", id);
        if (i > 0 && ci <= sc->component_index[i - 1]) return pfail(MJH_EINVAL, "Invalid component ID %d in SOS (JERR_BAD_COMPONENT_ID)", id);
        if (comp_scans[ci]++ && !prog) return pfail(MJH_EINVAL, "component %d is coded by two scans of a %s file (JERR_BAD_SCAN_SCRIPT)", ci, lossless ? "lossless" : "sequential");
        sc->component_index[i] = ci;
        sc->dc_tbl_no[i] = s[2 + 2 * i] >> 4;
        sc->ac_tbl_no[i] = s[2 + 2 * i] & 15;
        if (arith) {       // conditioning tables 0..3 are decoded: the one a scan of this kind uses (a DC refinement: none)
          const bool use_dc = !prog || (Ss == 0 && Ah == 0), use_ac = !prog || Ss != 0;
          if (use_dc && sc->dc_tbl_no[i] > 3)
            return pfail(MJH_EUNSUPPORTED, "arithmetic conditioning table %d (DC) in an SOS: tables 0..3 are decoded", sc->dc_tbl_no[i]);
          if (use_ac && sc->ac_tbl_no[i] > 3)
            return pfail(MJH_EUNSUPPORTED, "arithmetic conditioning table %d (AC) in an SOS: tables 0..3 are decoded", sc->ac_tbl_no[i]);
        }
        if (prog) {
          // jdphuff.c:126-144: where the reference warns, the file is refused
          if (Ss != 0 && coef_bits[ci][0] < 0)
            return pfail(MJH_EUNSUPPORTED, "Inconsistent progression sequence for component %d coefficient %d (JWRN_BOGUS_PROGRESSION): an AC scan before the component's DC scan", ci, 0);
          for (int k = Ss; k <= Se; k++) {
            const int expected = coef_bits[ci][k] < 0 ? 0 : coef_bits[ci][k];
            if (Ah != expected || (Ah == 0 && coef_bits[ci][k] >= 0))
              return pfail(MJH_EUNSUPPORTED, "Inconsistent progression sequence for component %d coefficient %d (JWRN_BOGUS_PROGRESSION): %s", ci, k,
                           Ah == 0 ? "a first scan of a coefficient already coded" : coef_bits[ci][k] < 0 ? "a refinement of a coefficient not yet coded" : "a refinement whose Ah is not the Al before it");
            coef_bits[ci][k] = Al;
          }
          // only the table the scan decodes with (jdphuff.c:159-176): DC first its DC table, an AC scan its AC table, DC refinement none
          const bool need_dc = !arith && Ss == 0 && Ah == 0, need_ac = !arith && Ss != 0;
          if ((need_dc && (sc->dc_tbl_no[i] > 3 || !((hdef >> (2 * sc->dc_tbl_no[i])) & 1))) || (need_ac && (sc->ac_tbl_no[i] > 3 || !((hdef >> (2 * sc->ac_tbl_no[i] + 1)) & 1))))
            return pfail(MJH_EINVAL, "Huffman table 0x%02x was not defined (JERR_NO_HUFF_TABLE)", s[2 + 2 * i]);
        } else if (lossless) {         // the DC table alone (jdlhuff.c start_pass_lhuff_decoder); a lossless frame has no quantization tables
          if (sc->dc_tbl_no[i] > 3 || !((hdef >> (2 * sc->dc_tbl_no[i])) & 1))
            return pfail(MJH_EINVAL, "Huffman table 0x%02x was not defined (JERR_NO_HUFF_TABLE)", s[2 + 2 * i]);
          continue;
        } else
        if (!arith && (sc->dc_tbl_no[i] > 3 || sc->ac_tbl_no[i] > 3 || !((hdef >> (2 * sc->dc_tbl_no[i])) & 1) || !((hdef >> (2 * sc->ac_tbl_no[i] + 1)) & 1)))
          return pfail(MJH_EINVAL, "Huffman table 0x%02x was not defined (JERR_NO_HUFF_TABLE)", s[2 + 2 * i]);
        if (!((info->quant_defined >> info->quant_tbl_no[ci]) & 1))
          return pfail(MJH_EINVAL, "Quantization table 0x%02x was not defined (JERR_NO_QUANT_TABLE)", info->quant_tbl_no[ci]);
      }
      if (!to_ex && arith && (t[0] != 0 || t[1] != 63 || t[2] != 0))
        return pfail(MJH_EUNSUPPORTED, "a scan with Ss=%d Se=%d Ah=%d Al=%d in a sequential arithmetic-coded file (the reference warns JWRN_NOT_SEQUENTIAL and decodes whole blocks): only Ss=0 Se=63 Ah=Al=0 is decoded", t[0], t[1], t[2] >> 4, t[2] & 15);
      if (!to_ex && (t[0] != 0 || t[1] != 63 || t[2] != 0))
        return pfail(MJH_EINVAL, "Invalid progressive parameters Ss=%d Se=%d Ah=%d Al=%d in a sequential file (JERR_BAD_PROGRESSION)", t[0], t[1], t[2] >> 4, t[2] & 15);
      sc->restart_interval = ri;
      sc->huff_defined = arith ? 0 : hdef;
      if (!arith) {
        memcpy(sc->huff_bits, hbits, sizeof(hbits));
        memcpy(sc->huff_vals, hvals, sizeof(hvals));
      } else if (!to_ex) { memset(sc->huff_bits, 0, sizeof(sc->huff_bits)); memset(sc->huff_vals, 0, sizeof(sc->huff_vals)); }
      if (cond) {
        MjhArithCond ac;
        for (int tb = 0; tb < 4; tb++) { ac.dc_L[tb] = dac_L[tb]; ac.dc_U[tb] = dac_U[tb]; ac.ac_K[tb] = dac_K[tb]; }
        cond->push_back(ac);
      }
      sc->data_offset = pos;
      // the segment ends at the first 0xFF that is followed by neither 0x00 nor RSTn (fill bytes 0xFF 0xFF belong to that marker)
      size_t q = pos;
      unsigned nrst = 0;
      for (;;) {
        const uint8_t *f = q < size ? (const uint8_t *)memchr(d + q, 0xFF, size - q) : nullptr;
        if (!f || (size_t)(f - d) + 1 >= size) return pfail(MJH_EINVAL, "Premature end of JPEG file (JWRN_JPEG_EOF)");
        q = (size_t)(f - d);
        const int c = d[q + 1];
        if (c == 0) { q += 2; continue; }
        if (c >= 0xD0 && c <= 0xD7) { nrst++; q += 2; continue; }
        if (c == 0xFF) {                                   // fill bytes: they belong to the marker behind them
          size_t r = q + 1;
          while (r < size && d[r] == 0xFF) r++;
          if (r < size && d[r] >= 0xD0 && d[r] <= 0xD7) { nrst++; q = r + 1; continue; }
        }
        break;
      }
      sc->data_size = q - pos;
      sc->restart_markers = nrst;
      pos = q;
      if (!to_ex) info->num_scans++;
      else {
        if (nex < cap) {
          mjh_jpeg_scan_ex *xs = &ex[nex];
          memcpy(xs, sc, sizeof(*sc));
          xs->Ss = Ss; xs->Se = Se; xs->Ah = Ah; xs->Al = Al;
        }
        nex++;
      }
      break;
    }
    default:              // APPn, COM and the rest: nothing to learn from them (a copy mode lists them above)
      break;
    }
  }
  if (!saw_sof) return pfail(MJH_EINVAL, "Invalid JPEG file structure: missing SOF marker (JERR_NO_IMAGE)");
  if (info->num_scans + nex == 0) return pfail(MJH_EINVAL, "JPEG datastream contains no image (JERR_NO_IMAGE)");
  for (int c = 0; c < info->num_components; c++)
    if (!comp_scans[c]) return pfail(MJH_EINVAL, "component %d of the source file is in no scan (JERR_MISSING_DATA)", c);
  if (nex > cap) return pfail(MJH_EUNSUPPORTED, "%d scans in a progressive file: at most %d are decoded (MJH_MAX_SRC_SCANS = %d)", nex, cap, MJH_MAX_SRC_SCANS);
  if (num_ex) *num_ex = nex;
  // default_decompress_parms (jdapimin.c:130-205)
  if (info->num_components == 1) info->jpeg_color_space = MJH_CS_GRAYSCALE;
  else if (info->num_components == 4) {
    // :183-201: the Adobe transform alone decides, a JFIF marker says nothing; where the reference warns (JWRN_ADOBE_XFORM) and
    // assumes YCCK, the file is refused
    if (info->saw_Adobe_marker && info->Adobe_transform != 0 && info->Adobe_transform != 2)
      return pfail(MJH_EUNSUPPORTED, "Unknown Adobe color transform code %d (JWRN_ADOBE_XFORM) in a four-component file: 0 (CMYK) and 2 (YCCK) are decoded", info->Adobe_transform);
    info->jpeg_color_space = info->saw_Adobe_marker && info->Adobe_transform == 2 ? MJH_CS_YCCK : MJH_CS_CMYK;
  }
  else if (info->saw_JFIF_marker) info->jpeg_color_space = MJH_CS_YCbCr;
  else if (info->saw_Adobe_marker) info->jpeg_color_space = info->Adobe_transform == 0 ? MJH_CS_RGB : MJH_CS_YCbCr;
  else info->jpeg_color_space = (info->component_id[0] == 82 && info->component_id[1] == 71 && info->component_id[2] == 66) ? MJH_CS_RGB : MJH_CS_YCbCr;
  if (lossless) {
    // (a three-component lossless file without a marker is RGB: jdapimin.c:157-181 guesses RGB for every lossless file)
    if (info->num_components == 3 && !info->saw_JFIF_marker && !info->saw_Adobe_marker) info->jpeg_color_space = MJH_CS_RGB;
    if (nex > 0 && cap > 0) { info->lossless_psv = ex[0].Ss; info->lossless_pt = ex[0].Al; }
  }
  return MJH_OK;
}

extern "C" int mjh_jpeg_probe(const void *jpeg, size_t size, mjh_jpeg_info *info)
{
  if (!jpeg || !info) return pfail(MJH_EINVAL, "bad arguments");
  return probe_walk(jpeg, size, 0u, info, nullptr, 0, nullptr);
}

extern "C" int mjh_jpeg_probe_ex(const void *jpeg, size_t size, unsigned accept, mjh_jpeg_info *info, mjh_jpeg_scan_ex *scans, int cap, int *num_scans)
{
  if (!jpeg || !info) return pfail(MJH_EINVAL, "bad arguments");
  if (accept & ~MJH_SRC_ALL) return pfail(MJH_EINVAL, "unknown source kinds 0x%x (MJH_SRC_PROGRESSIVE | MJH_SRC_LOSSLESS | MJH_SRC_ARITHMETIC)", accept);
  if (!accept) { if (num_scans) *num_scans = 0; return probe_walk(jpeg, size, 0u, info, nullptr, 0, nullptr); }
  if (!scans || !num_scans || cap < 1) return pfail(MJH_EINVAL, "bad arguments: MJH_SRC_PROGRESSIVE, MJH_SRC_LOSSLESS and MJH_SRC_ARITHMETIC need room for the scans");
  return probe_walk(jpeg, size, accept, info, scans, cap < MJH_MAX_SRC_SCANS ? cap : MJH_MAX_SRC_SCANS, num_scans);
}

// mjh_jpeg_probe / mjh_jpeg_probe_ex and the marker list of one copy mode in the same walk (mjh_encoder.cpp: a transcode call
// with a copy mode reads every file once)
int mjh_probe_markers(const void *jpeg, size_t size, unsigned accept, mjh_jpeg_info *info, mjh_jpeg_scan_ex *scans, int cap, int *num_scans,
                      int copy_mode, std::vector<mjh_jpeg_marker> *saved, std::vector<MjhArithCond> *cond)
{
  if (saved) saved->clear();
  if (!accept) { if (num_scans) *num_scans = 0; return probe_walk(jpeg, size, 0u, info, nullptr, 0, nullptr, copy_mode, saved, cond); }
  return probe_walk(jpeg, size, accept, info, scans, cap < MJH_MAX_SRC_SCANS ? cap : MJH_MAX_SRC_SCANS, num_scans, copy_mode, saved, cond);
}

extern "C" int mjh_jpeg_arith_cond(const void *jpeg, size_t size, unsigned accept, struct mjh_jpeg_arith_cond *list, int cap, int *count)
{
  if (count) *count = 0;
  if (!jpeg || cap < 0 || (cap > 0 && !list)) return pfail(MJH_EINVAL, "bad arguments");
  if (accept & ~MJH_SRC_ALL) return pfail(MJH_EINVAL, "unknown source kinds 0x%x (MJH_SRC_PROGRESSIVE | MJH_SRC_LOSSLESS | MJH_SRC_ARITHMETIC)", accept);
  static thread_local mjh_jpeg_info info;
  static thread_local std::vector<mjh_jpeg_scan_ex> room;
  static thread_local std::vector<MjhArithCond> conds;
  if (accept) room.resize(MJH_MAX_SRC_SCANS);
  int ns = 0;
  const int rc = mjh_probe_markers(jpeg, size, accept, &info, accept ? room.data() : nullptr, MJH_MAX_SRC_SCANS, &ns, MJH_COPY_NONE, nullptr, &conds);
  if (rc) return rc;
  if (count) *count = (int)conds.size();
  if (conds.size() > (size_t)cap) return pfail(MJH_EINVAL, "%zu scans in the file, room for %d", conds.size(), cap);
  for (size_t i = 0; i < conds.size(); i++) list[i] = conds[i];
  return MJH_OK;
}

extern "C" int mjh_jpeg_markers(const void *jpeg, size_t size, unsigned accept, int copy_mode, mjh_jpeg_marker *list, int cap, int *count)
{
  if (count) *count = 0;
  if (!jpeg || cap < 0 || (cap > 0 && !list)) return pfail(MJH_EINVAL, "bad arguments");
  if (accept & ~MJH_SRC_ALL) return pfail(MJH_EINVAL, "unknown source kinds 0x%x (MJH_SRC_PROGRESSIVE | MJH_SRC_LOSSLESS | MJH_SRC_ARITHMETIC)", accept);
  if (copy_mode < MJH_COPY_NONE || copy_mode > MJH_COPY_ICC) return pfail(MJH_EINVAL, "unknown copy mode %d (MJH_COPY_NONE .. MJH_COPY_ICC)", copy_mode);
  static thread_local mjh_jpeg_info info;
  static thread_local std::vector<mjh_jpeg_scan_ex> room;
  static thread_local std::vector<mjh_jpeg_marker> saved;
  if (accept) room.resize(MJH_MAX_SRC_SCANS);
  int ns = 0;
  const int rc = mjh_probe_markers(jpeg, size, accept, &info, accept ? room.data() : nullptr, MJH_MAX_SRC_SCANS, &ns, copy_mode, &saved, nullptr);
  if (rc) return rc;
  if (count) *count = (int)saved.size();
  if (saved.size() > (size_t)cap) return pfail(MJH_EINVAL, "%zu markers in the file, room for %d", saved.size(), cap);
  for (size_t i = 0; i < saved.size(); i++) list[i] = saved[i];
  return MJH_OK;
}

extern "C" int mjh_params_from_jpeg(const mjh_jpeg_info *info, int compress_profile, mjh_params *p)
{
  if (!info || !p) return pfail(MJH_EINVAL, "bad arguments");
  const int nc = info->num_components;
  if (nc != 1 && nc != 3 && nc != 4) return pfail(MJH_EUNSUPPORTED, "%d components", nc);
  if (nc == 4) {
    // A CMYK / YCCK file: the parameters of an encoder that owns the geometry and the tables of decode calls on such files and
    // writes nothing -- jpeg_set_colorspace(JCS_CMYK / JCS_YCCK)'s table numbers (jcparam.c:624-645), the file's own ids, factors
    // and quantization tables, a sequential script whatever the profile (no scan script exists for four components here)
    if (info->sof_type == 3) return pfail(MJH_EUNSUPPORTED, "4 components in a lossless source file");
    if (info->jpeg_color_space != MJH_CS_CMYK && info->jpeg_color_space != MJH_CS_YCCK) return pfail(MJH_EINVAL, "a four-component file whose colour space is %d (MJH_CS_CMYK or MJH_CS_YCCK)", info->jpeg_color_space);
    int rc = mjh_params_defaults(p, info->image_width, info->image_height, 3, 0, compress_profile, 1, 1);
    if (rc) return rc;
    const bool ycck = info->jpeg_color_space == MJH_CS_YCCK;
    p->trellis_quant = 0;
    p->data_precision = info->data_precision;
    p->input_components = 4;
    p->input_pixel_size = 4;
    p->num_components = 4;
    p->color_transform = ycck ? MJH_COLOR_YCCK : MJH_COLOR_CMYK;
    p->write_JFIF_header = 0;
    for (int t = 0; t < 4; t++)
      if ((info->quant_defined >> t) & 1) memcpy(p->quantval[t], info->quantval[t], sizeof(p->quantval[t]));
    for (int c = 0; c < 4; c++) {
      p->component_id[c] = info->component_id[c];
      p->h_samp_factor[c] = info->h_samp_factor[c];
      p->v_samp_factor[c] = info->v_samp_factor[c];
      p->quant_tbl_no[c] = info->quant_tbl_no[c];
      p->dc_tbl_no[c] = p->ac_tbl_no[c] = ycck && (c == 1 || c == 2);
      if (p->quant_tbl_no[c] < 0 || p->quant_tbl_no[c] > 3 || !((info->quant_defined >> p->quant_tbl_no[c]) & 1))
        return pfail(MJH_EINVAL, "Quantization table 0x%02x was not defined (JERR_NO_QUANT_TABLE)", p->quant_tbl_no[c]);
    }
    return MJH_OK;
  }
  if (info->sof_type == 3) {
    // A lossless file (mjh_jpeg_probe_ex with MJH_SRC_LOSSLESS): the parameters of an encoder that writes such files and owns the
    // geometry its decode calls need -- jpeg_enable_lossless(predictor, point transform) of the file's first scan as a script of one
    // scan, the file's precision and components, no colour conversion (gray as gray, RGB as RGB)
    if (nc == 3 && info->jpeg_color_space != MJH_CS_RGB)
      return pfail(MJH_EUNSUPPORTED, "a three-component lossless file that is not RGB: its colour conversion is not built");
    int rc = mjh_params_defaults(p, info->image_width, info->image_height, nc == 1 ? 1 : 3, nc == 1, compress_profile, 2, 2);
    if (rc) return rc;
    p->trellis_quant = 0;
    p->data_precision = info->data_precision;
    p->num_components = nc;
    p->num_scans = 1;
    p->optimize_scans = 0;
    memset(&p->scan_info[0], 0, sizeof(p->scan_info[0]));
    p->scan_info[0].comps_in_scan = nc;
    for (int c = 0; c < nc; c++) p->scan_info[0].component_index[c] = c;
    p->scan_info[0].Ss = info->lossless_psv; p->scan_info[0].Al = info->lossless_pt;
    if (nc == 3) { p->color_transform = MJH_COLOR_NONE; p->write_JFIF_header = 0; }
    for (int c = 0; c < nc; c++) {
      p->component_id[c] = info->component_id[c];
      p->h_samp_factor[c] = p->v_samp_factor[c] = 1;
      p->quant_tbl_no[c] = p->dc_tbl_no[c] = p->ac_tbl_no[c] = 0;
    }
    return MJH_OK;
  }
  // jpeg_set_defaults + jpeg_set_colorspace(srcinfo->jpeg_color_space)
  int rc = mjh_params_defaults(p, info->image_width, info->image_height, nc == 1 ? 1 : 3, nc == 1, compress_profile, 2, 2);
  if (rc) return rc;
  p->trellis_quant = 0;                                   // jctrans.c:102
  p->data_precision = info->data_precision;
  if (info->jpeg_color_space == MJH_CS_RGB) {             // jcparam.c:604-619: no JFIF, Adobe marker, every component on tables 0
    p->color_transform = MJH_COLOR_NONE;
    p->write_JFIF_header = 0;
    for (int c = 0; c < 3; c++) p->dc_tbl_no[c] = p->ac_tbl_no[c] = 0;
  }
  for (int t = 0; t < 4; t++)
    if ((info->quant_defined >> t) & 1) memcpy(p->quantval[t], info->quantval[t], sizeof(p->quantval[t]));
  for (int c = 0; c < nc; c++) {
    p->component_id[c] = info->component_id[c];
    p->h_samp_factor[c] = info->h_samp_factor[c];
    p->v_samp_factor[c] = info->v_samp_factor[c];
    p->quant_tbl_no[c] = info->quant_tbl_no[c];
    // a single component is always written 1x1, whatever the source's frame header says ("some decoders choke on grayscale images
    // with other sampling factors", jtransform_adjust_parameters transupp.c:2072-2079); its non-interleaved scan is laid out alike
    if (nc == 1) p->h_samp_factor[c] = p->v_samp_factor[c] = 1;
    if (p->quant_tbl_no[c] < 0 || p->quant_tbl_no[c] > 3 || !((info->quant_defined >> p->quant_tbl_no[c]) & 1))
      return pfail(MJH_EINVAL, "Quantization table 0x%02x was not defined (JERR_NO_QUANT_TABLE)", p->quant_tbl_no[c]);
  }
  if (p->compress_profile == MJH_PROFILE_MAX_COMPRESSION) return mjh_params_search_progression(p);   // what jpeg_set_defaults selects there (jcparam.c:497-503)
  return MJH_OK;
}

// ---- lossless transforms (transupp.c as jpegtran.c drives it) ---------------------------------------------------------------------
// jtransform_parse_crop_spec (transupp.c:1395-1450): [W[f|r]][xH[f|r]][{+-}X[{+-}Y]], every part optional, nothing behind it
static bool crop_number(const char *&s, unsigned *v)
{
  const char *b = s;
  unsigned x = 0;
  while (*s >= '0' && *s <= '9') x = x * 10u + (unsigned)(*s++ - '0');
  *v = x;
  return s != b;
}
static int crop_suffix(const char *&s)
{
  if (*s == 'f' || *s == 'F') { s++; return MJH_CROP_FORCE; }
  if (*s == 'r' || *s == 'R') { s++; return MJH_CROP_REFLECT; }
  return MJH_CROP_POS;
}

extern "C" int mjh_transform_parse_crop(mjh_transform *t, const char *spec)
{
  if (!t || !spec) return pfail(MJH_EINVAL, "bad arguments");
  const char *s = spec;
  t->crop = 0;
  t->crop_width_set = t->crop_height_set = t->crop_xoffset_set = t->crop_yoffset_set = MJH_CROP_UNSET;
  t->crop_width = t->crop_height = t->crop_xoffset = t->crop_yoffset = 0;
  bool ok = true;
  if (*s >= '0' && *s <= '9') { ok = crop_number(s, &t->crop_width); t->crop_width_set = crop_suffix(s); }
  if (ok && (*s == 'x' || *s == 'X')) { s++; ok = crop_number(s, &t->crop_height); if (ok) t->crop_height_set = crop_suffix(s); }
  if (ok && (*s == '+' || *s == '-')) { t->crop_xoffset_set = *s++ == '-' ? MJH_CROP_NEG : MJH_CROP_POS; ok = crop_number(s, &t->crop_xoffset); }
  if (ok && (*s == '+' || *s == '-')) { t->crop_yoffset_set = *s++ == '-' ? MJH_CROP_NEG : MJH_CROP_POS; ok = crop_number(s, &t->crop_yoffset); }
  if (!ok || *s) return pfail(MJH_EINVAL, "bogus -crop argument '%s'", spec);
  t->crop = 1;
  return MJH_OK;
}

// one axis of the crop request (transupp.c:1585-1716): the size after cropping and the offset in iMCUs
static int crop_axis(int transform, unsigned full, unsigned imcu, unsigned size, int size_set, unsigned off, int off_set, unsigned *out, unsigned *off_imcu)
{
  if (off_set == MJH_CROP_UNSET) off = 0;
  if (size_set == MJH_CROP_UNSET) {
    if (off >= full) return pfail(MJH_EINVAL, "Invalid crop request (JERR_BAD_CROP_SPEC)");
    size = full - off;
  } else if (size > full) {
    if (transform != MJH_XFORM_NONE || off >= size || off > size - full) return pfail(MJH_EINVAL, "Invalid crop request (JERR_BAD_CROP_SPEC)");
    return pfail(MJH_EUNSUPPORTED, "crop extension: a crop of %u on an image of %u (do_crop_ext_* of transupp.c is not built)", size, full);
  } else if (off >= full || size == 0 || off > full - size) return pfail(MJH_EINVAL, "Invalid crop request (JERR_BAD_CROP_SPEC)");
  const unsigned o = off_set == MJH_CROP_NEG ? full - size - off : off;
  *out = size + o % imcu;
  *off_imcu = o / imcu;
  return MJH_OK;
}

int mjh_transform_plan(const mjh_jpeg_info *f, const mjh_transform *t, MjhXformPlan *g)
{
  memset(g, 0, sizeof(*g));
  g->num_components = f->num_components;
  g->out_w = f->image_width; g->out_h = f->image_height;
  if (!t) return MJH_OK;
  if (t->transform < MJH_XFORM_NONE || t->transform > MJH_XFORM_ROT_270)
    return pfail(t->transform == 8 || t->transform == 9 ? MJH_EUNSUPPORTED : MJH_EINVAL, "transform %d (MJH_XFORM_NONE .. MJH_XFORM_ROT_270; -wipe and -drop are not built)", t->transform);
  if (t->transform == MJH_XFORM_NONE && !t->crop && !t->grayscale) return MJH_OK;      // (-trim / -perfect alone change nothing)
  const int nc = f->num_components;
  if (nc == 4) return pfail(MJH_EUNSUPPORTED, "four-component files (CMYK, YCCK) are decoded, not written: no lossless transform of them");
  if (nc != 1 && nc != 3) return pfail(MJH_EUNSUPPORTED, "%d components", nc);
  if (t->crop)
    for (int s : { t->crop_width_set, t->crop_height_set })
      if (s == MJH_CROP_FORCE || s == MJH_CROP_REFLECT)
        return pfail(MJH_EUNSUPPORTED, "the f / r suffixes of a crop specification (crop extension, do_crop_ext_* of transupp.c is not built)");
  g->active = 1;
  int maxh = 1, maxv = 1;
  for (int c = 0; c < nc; c++) { if (f->h_samp_factor[c] > maxh) maxh = f->h_samp_factor[c]; if (f->v_samp_factor[c] > maxv) maxv = f->v_samp_factor[c]; }
  g->num_components = (t->grayscale && f->jpeg_color_space == MJH_CS_YCbCr && nc == 3) ? 1 : nc;
  unsigned imw = g->num_components == 1 ? 8u : (unsigned)maxh * 8u, imh = g->num_components == 1 ? 8u : (unsigned)maxv * 8u;
  unsigned W = (unsigned)f->image_width, H = (unsigned)f->image_height;
  const int x = t->transform;
  if (t->perfect) {
    const bool need_w = x == MJH_XFORM_FLIP_H || x == MJH_XFORM_ROT_270 || x == MJH_XFORM_TRANSVERSE || x == MJH_XFORM_ROT_180;
    const bool need_h = x == MJH_XFORM_FLIP_V || x == MJH_XFORM_ROT_90 || x == MJH_XFORM_TRANSVERSE || x == MJH_XFORM_ROT_180;
    if ((need_w && W % imw) || (need_h && H % imh)) return pfail(MJH_EINVAL, "transformation is not perfect (%ux%u, iMCU %ux%u)", W, H, imw, imh);
  }
  g->transpose = x == MJH_XFORM_TRANSPOSE || x == MJH_XFORM_TRANSVERSE || x == MJH_XFORM_ROT_90 || x == MJH_XFORM_ROT_270;
  g->mirror_x = x == MJH_XFORM_FLIP_H || x == MJH_XFORM_ROT_90 || x == MJH_XFORM_ROT_180 || x == MJH_XFORM_TRANSVERSE;
  g->mirror_y = x == MJH_XFORM_FLIP_V || x == MJH_XFORM_ROT_270 || x == MJH_XFORM_ROT_180 || x == MJH_XFORM_TRANSVERSE;
  if (g->transpose) { unsigned s = W; W = H; H = s; s = imw; imw = imh; imh = s; }
  // W x H, imw x imh: the uncropped destination and its iMCU from here on
  unsigned ow = W, oh = H, xc = 0, yc = 0;
  if (t->crop) {
    int rc = crop_axis(x, W, imw, t->crop_width, t->crop_width_set, t->crop_xoffset, t->crop_xoffset_set, &ow, &xc);
    if (rc == MJH_OK) rc = crop_axis(x, H, imh, t->crop_height, t->crop_height_set, t->crop_yoffset, t->crop_yoffset_set, &oh, &yc);
    if (rc) return rc;
  }
  // trim_right_edge / trim_bottom_edge (transupp.c:1455-1475): only a destination that reaches the partial iMCU loses it
  if (t->trim && g->mirror_x) { const unsigned m = ow / imw; if (m > 0 && xc + m == W / imw) ow = m * imw; }
  if (t->trim && g->mirror_y) { const unsigned m = oh / imh; if (m > 0 && yc + m == H / imh) oh = m * imh; }
  g->out_w = (int)ow; g->out_h = (int)oh;
  g->x_crop = (int)xc; g->y_crop = (int)yc;
  g->mir_cols = (int)(W / imw); g->mir_rows = (int)(H / imh);
  return MJH_OK;
}

extern "C" int mjh_params_from_jpeg_transform(const mjh_jpeg_info *info, const mjh_transform *t, int compress_profile, mjh_params *p)
{
  if (!info || !p) return pfail(MJH_EINVAL, "bad arguments");
  MjhXformPlan g;
  int rc = mjh_transform_plan(info, t, &g);
  if (rc) return rc;
  if (!g.active) return mjh_params_from_jpeg(info, compress_profile, p);
  static thread_local mjh_jpeg_info d;       // the frame jtransform_adjust_parameters leaves (transupp.c:2048-2079)
  d = *info;
  if (t->grayscale) {
    int maxh = 1, maxv = 1;
    for (int c = 0; c < info->num_components; c++) { if (info->h_samp_factor[c] > maxh) maxh = info->h_samp_factor[c]; if (info->v_samp_factor[c] > maxv) maxv = info->v_samp_factor[c]; }
    const bool known = (info->jpeg_color_space == MJH_CS_YCbCr && info->num_components == 3) || (info->jpeg_color_space == MJH_CS_GRAYSCALE && info->num_components == 1);
    if (!known || info->h_samp_factor[0] != maxh || info->v_samp_factor[0] != maxv)
      return pfail(MJH_EUNSUPPORTED, "Unsupported color conversion request (JERR_CONVERSION_NOTIMPL): grayscale needs a YCbCr or gray file whose first component is sampled at the maximum");
    d.num_components = 1;                    // jpeg_set_colorspace(JCS_GRAYSCALE): id 1, its quantization table number kept
    d.jpeg_color_space = MJH_CS_GRAYSCALE;
    d.component_id[0] = 1;
  }
  if (g.num_components == 1) d.h_samp_factor[0] = d.v_samp_factor[0] = 1;
  d.image_width = g.out_w; d.image_height = g.out_h;
  if (g.transpose) {                          // transpose_critical_parameters (transupp.c:1831-1872)
    for (int c = 0; c < d.num_components; c++) { const int s = d.h_samp_factor[c]; d.h_samp_factor[c] = d.v_samp_factor[c]; d.v_samp_factor[c] = s; }
  }
  rc = mjh_params_from_jpeg(&d, compress_profile, p);
  if (rc) return rc;
  if (g.transpose)                            // every table of the destination object, the profile's defaults included
    for (int tb = 0; tb < 4; tb++)
      for (int i = 0; i < 8; i++)
        for (int j = 0; j < i; j++) { const uint16_t s = p->quantval[tb][i * 8 + j]; p->quantval[tb][i * 8 + j] = p->quantval[tb][j * 8 + i]; p->quantval[tb][j * 8 + i] = s; }
  return MJH_OK;
}
