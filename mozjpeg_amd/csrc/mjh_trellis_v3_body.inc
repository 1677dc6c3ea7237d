// Body of k_trellis_ac_v3 and k_trellis_ac_v3_cf (mjh_trellis.hip): included once in each, so that the plain kernel keeps its name,
// its argument list and its machine code.  The including kernel defines CF (count the final AC symbols of the blocks it finishes),
// fin_tabs and fin_slot_of_comp (CF only: where the counts go) in front of the #include.
  static_assert(QN >= 16 && QN <= 63 && NPASS >= 1 && NPASS <= 8 && (FD || !CF), "queue capacity / passes");
  constexpr int FWORDS = 33;
  __shared__ unsigned fhist[CF ? FWORDS : 1];      // CF: 66 bins of 16 bits, bin b = half b & 1 of word b >> 1
  constexpr int TILE = 64 * NPASS;
  __shared__ uint2 col[QN + 1][64];      // tile sort scratch; per pass: queue records (record r in slot r) -> live entries {azd, acc} (entry e in slot e; 0 = the virtual start) -> value column
  // live entry e at [e]: position | back entry << 6 | magnitude (< 16) << 12 (the signs: one bit per position in a register).
  // SLIM (up to 16 records): the word keeps the position only -- ONE byte -- and the back entry (< 16) and the magnitude (< 16) of
  // entry e are nibble e - 1 of two 64-bit registers.  17 slots of 9 instead of 10 bytes per lane + the rate rows = 10 048 bytes:
  // 16 waves per CU instead of 14 (the kernel follows its occupancy, profiles/r06g_occupancy.md: T(w) ~ 0.52 + 13.3 / w), and the
  // scan loop loses the two masks of its position fields.  Same operations on the same values per lane: the files do not change.
  constexpr bool SLIM = QN <= 16;
  typedef typename std::conditional<SLIM, unsigned char, unsigned short>::type info_t;
  __shared__ info_t info[QN + 1][64];
  __shared__ float4 rate_rows[16];
  typedef unsigned __attribute__((may_alias)) u_alias;
  typedef unsigned short __attribute__((may_alias)) us_alias;
  const int img = blockIdx.y + img0, tl = blockIdx.x, lane = threadIdx.x;      // (img0: first image of this launch's range of the batch)
  auto fh_add = [&](int bin, unsigned n) { atomicAdd(&fhist[bin >> 1], n << (16 * (bin & 1))); };
  auto fh_get = [&](int bin) -> unsigned { return (fhist[bin >> 1] >> (16 * (bin & 1))) & 0xFFFFu; };
  const int comp = tl >= tile0_of_comp.w ? 3 : tl >= tile0_of_comp.z ? 2 : tl >= tile0_of_comp.y ? 1 : 0;
  const int t0 = comp == 0 ? 0 : comp == 1 ? tile0_of_comp.y : comp == 2 ? tile0_of_comp.z : tile0_of_comp.w;
  const MjhComp cc = C.c[comp];
  const int tile_base = (tl - t0) * TILE;
  const int slot = comp == 0 ? ac_slot_of_comp.x : comp == 1 ? ac_slot_of_comp.y : comp == 2 ? ac_slot_of_comp.z : ac_slot_of_comp.w;
  const MjhHuffTable *T = tabs + (size_t)img * slots_per_image + slot;
  const size_t gblk0 = (size_t)img * C.total_real_blocks + cc.blk_off;
  if (lane < 16) rate_rows[lane] = rate_row(reinterpret_cast<const uint4 *>(T->ehufsi)[lane]);
  const int si_f0 = (int)T->ehufsi[0xF0], si_eob = (int)T->ehufsi[0];
  const float f0f = si_f0 ? (float)si_f0 : 3e38f, eobf = (float)si_eob;
  const int dq_lane = Q->dq8[cc.qtbl][lane];                    // lane k holds the row entry of position k (ds_bpermute lookups)
  const float lt_lane = Q->lambda_tbl[cc.qtbl][lane];

  // ---- tile sort: descending key; perm entry = index in tile | key << 9 ----
  unsigned long long mine0 = 0ull, mine1 = 0ull;
  {
    u_alias *hist = reinterpret_cast<u_alias *>(&col[0][0]);              // [64]
    us_alias *perm = reinterpret_cast<us_alias *>(&col[0][0]) + 128;      // [TILE], behind the histogram
    hist[lane] = 0u;
    if (CF) for (int b = lane; b < FWORDS; b += 64) fhist[b] = 0u;
    __syncthreads();
    unsigned key[NPASS], rank[NPASS];
#pragma unroll
    for (int j = 0; j < NPASS; j++) {
      const int b = tile_base + j * 64 + lane;
      unsigned k = b < cc.nblk ? (unsigned)nq8[gblk0 + b] : 0u;
      key[j] = k > 63u ? 63u : k;
      rank[j] = atomicAdd(&hist[key[j]], 1u);
    }
    __syncthreads();
    const unsigned h = hist[63 - lane];     // lane L: blocks with key 63-L; blocks with a larger key come first
    unsigned inc = h;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned n = __shfl_up(inc, o, 64);
      if (lane >= o) inc += n;
    }
    __syncthreads();
    hist[63 - lane] = inc - h;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NPASS; j++) perm[hist[key[j]] + rank[j]] = (unsigned short)((unsigned)(j * 64 + lane) | (key[j] << 9));
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NPASS; j++) {
      const unsigned long long v = perm[j * 64 + lane];
      if (j < 4) mine0 |= v << (16 * j); else mine1 |= v << (16 * (j - 4));
    }
    __syncthreads();
  }

  us_alias *colh = reinterpret_cast<us_alias *>(&col[0][0]);   // value of slot s: row s>>2, half-word s&3 of the lane's uint2
#pragma unroll 1
  for (int pass = 0; pass < NPASS; pass++) {
    const unsigned pe = (unsigned)(((pass < 4 ? mine0 : mine1) >> (16 * (pass & 3))) & 0xFFFFull);
    const int blk = tile_base + (int)(pe & 511u);
    const bool inside = blk < cc.nblk;
    const size_t gblk = gblk0 + (inside ? blk : 0);
    if (__builtin_amdgcn_ballot_w64(inside && (pe >> 9) != 0u) == 0ull) {   // nothing quantizes to non-zero: all-zero blocks
      if (inside) nzmask[gblk] = 0ull;
      if (CF) {      // every block of the pass is all zero: one EOB each
        const unsigned nz = (unsigned)__popcll(__builtin_amdgcn_ballot_w64(inside));
        if (lane == 0 && nz) fh_add(MJH_FH_EOB, nz);
      }
      continue;
    }
    const float lambda = lambda_in[gblk0 + (inside ? blk : cc.nblk - 1)];
    int nq = 0, qmax = 0;
    float azd63;
    {
      const int16_t *uq = coef_uq + (size_t)img * C.coefs_per_image + cc.coef_off + (inside ? blk : cc.nblk - 1);
      short xs[64];
#pragma unroll
      for (int k = 1; k < 64; k++) xs[k] = uq[(size_t)k * cc.kstride];
      // (the rows' wave-uniform constants: fetched for eight positions at a time, outside the per-position branch -- one scalar-memory
      // round trip per eight positions instead of two per position; see dct_quant_body)
      constexpr int QCH = 8;
      int dq_c[QCH], sdiv_c[QCH];
      unsigned mdiv_c[QCH];
      float lt_c[QCH], rcp_c[QCH], thr_c[QCH];
      float azd = 0.0f;
#pragma unroll
      for (int k = 1; k < 64; k++) {
        if (k == 1 || (k % QCH) == 0) {
#pragma unroll
          for (int j = 0; j < QCH; j++) {
            const int kk = (k / QCH) * QCH + j;
            dq_c[j] = Q->dq8[cc.qtbl][kk];
            lt_c[j] = Q->lambda_tbl[cc.qtbl][kk];
            thr_c[j] = Q->thr8[cc.qtbl][kk];
            if (FD) { sdiv_c[j] = Q->sdiv[cc.qtbl][kk]; mdiv_c[j] = Q->mdiv[cc.qtbl][kk]; }
            else rcp_c[j] = Q->rcp8q[cc.qtbl][kk];
          }
        }
        // The position's share of the all-zero distortion needs x^2 only: from the SIGNED coefficient converted to float -- xf * xf is
        // the correctly rounded x^2, which is what (float)(x * x) is (one rounding of the same exact integer either way) -- and
        // "quantizes to non-zero" is a compare of |xf| (a source modifier) with the table's float threshold: six VALU instructions per
        // position instead of nine; |x| as an integer exists only inside the branch few positions take.
        const int xsg = xs[k];
        const float xf = (float)xsg;
        float t = (xf * xf) * lambda;
        t = t * lt_c[k % QCH];
        const float azd_cur = t + azd;
        if (__builtin_fabsf(xf) >= thr_c[k % QCH]) {
          const int x = (int)__builtin_fabsf(xf);      // (one conversion with a source modifier)
          const int dq = dq_c[k % QCH];
          int qval = FD ? udiv_mh(x + (dq >> 1), sdiv_c[k % QCH], mdiv_c[k % QCH]) : udiv_exact(x + (dq >> 1), dq, rcp_c[k % QCH]);
          if (qval >= 1024) qval = 1023;
          qmax = qval > qmax ? qval : qmax;
          // (a block with more than QN records is deferred: what its surplus records overwrite in the last slot is never read)
          col[nq < QN ? nq : QN - 1][lane] = make_uint2((unsigned)k | ((__float_as_uint(xf) >> 25) & 64u) | ((unsigned)qval << 7) | ((unsigned)x << 17), __float_as_uint(azd));      // (the sign: the float's)
          nq++;
        }
        azd = azd_cur;
      }
      azd63 = azd;
      defer_blocks(inside && (nq > QN || qmax >= 16), worklist, (unsigned)img, ((unsigned)comp << 28) | (unsigned)blk, 0u, xs, dense, dense_cap, true, lane);
      // (the whole batch's counts: the first range's header.  A large batch counts in every (count_mask + 1)-th tile only -- the host
      // scales: three more atomics per pass on the line of the work-list counter, which one word's ~88 operations per microsecond make
      // ~1.3 % of the kernel, profiles/r06g_occupancy.md)
      if ((tl & count_mask) == 0) count_heavy(counts, inside, nq, lane);
    }
    const bool work = inside && nq <= QN && qmax < 16;

    // ---- the walk: every lane consumes its own records, one record per round; the next record is always one load ahead ----
    int nlive = 1, qi = 0, last = 0;
    unsigned long long neg = 0ull;          // positions whose coefficient is negative (of the entries created so far)
    bool act = work && nq > 0;
    int i = 0, x = 0, qval = 0, ncd = 0, sgn = 0, e = 0, beste = -1, bestk = 0;
    float azd_prev = 0.0f, azd_cur = 0.0f, d0 = 0.0f, d1 = 0.0f, d2 = 0.0f, d3 = 0.0f, best = 1e38f;
    float end_best = azd63 + eobf;
    uint2 rec_n = col[0][lane];
    col[0][lane] = make_uint2(0u, 0u);     // record 0 is in registers: its slot becomes entry 0, the virtual start (position 0, azd 0, cost 0)
    info[0][lane] = (info_t)0;
    unsigned long long back4 = 0ull, mag4 = 0ull;      // SLIM: nibble e - 1 = back entry / magnitude of live entry e
    // quantizer constants of the NEXT record's position: lane k holds entry k of the component's rows, fetched with ds_bpermute
    // at a point where every lane of the wave is enabled (a disabled source lane would read as 0)
    int dq_n = 1;
    float lt_n = 0.0f;
    auto lookup = [&]() {
      const int a = (int)(rec_n.x & 63u) << 2;
      dq_n = __builtin_amdgcn_ds_bpermute(a, dq_lane) & 0x3FFFF;      // 8q <= 8 * 32767: tells the compiler the 24-bit multiplies are exact
      lt_n = __int_as_float(__builtin_amdgcn_ds_bpermute(a, __float_as_int(lt_lane)));
    };
    lookup();
    // `wide`: some lane of the round has a record with more than two candidates (quantized magnitude >= 4); without one, the
    // round's steps evaluate two candidates and the distortions of the other two are not computed
    auto setup = [&](bool wide) {
      const uint2 rec = rec_n;
      qi++;
      rec_n = col[qi][lane];      // qi <= nq <= QN: slot QN exists (a slot is overwritten only after its record was consumed: entry e lives in slot e <= qi - 1 when it is written, and record qi - 1 is in registers by then)
      i = (int)(rec.x & 63u); sgn = (int)((rec.x >> 6) & 1u); qval = (int)((rec.x >> 7) & 1023u); x = (int)(rec.x >> 17);
      azd_prev = __uint_as_float(rec.y);
      const int dq = dq_n;
      const float lti = lt_n;
      float t = squaref(x) * lambda;      // ((float)x * (float)x == (float)(x * x): one rounding of the same exact integer)
      t = t * lti;
      azd_cur = t + azd_prev;
      ncd = bitlen((unsigned)qval);
      float dd[4] = { 3e38f, 3e38f, 3e38f, 3e38f };
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if (k >= 2 && !wide) break;      // uniform
        const int cand = (k < ncd - 1) ? (2 << k) - 1 : qval;
        const int delta = mul24(cand, dq) - x;
        const float d = squaref(delta) * lambda;      // (|delta| <= x < 2^15)
        dd[k] = k < ncd ? d * lti : 3e38f;
      }
      d0 = dd[0]; d1 = dd[1]; d2 = dd[2]; d3 = dd[3];
      e = nlive; best = 1e38f; beste = -1; bestk = 0;
    };
    auto next_wide = [&]() { return __builtin_amdgcn_ballot_w64(act && qi < nq && ((rec_n.x >> 7) & 1023u) >= 4u) != 0ull; };   // of the records about to be set up
    bool wide = next_wide();
    if (act) setup(wide);
    // One ROUND per queue record.  A round is the scan of the lane's live entries for its current record (pair steps, run
    // until the last lane's scan has ended) and then, at a point where the wave is whole again, the commit of the new entry and
    // the setup of the next record for every working lane at once.  (Until round 5 a lane committed and set up as soon as its own
    // scan ended: with 64 lanes some lane nearly always did, so those ~100 instructions were issued in almost every iteration
    // for a handful of lanes -- tools/model_sched.py: 0.74 of the issued instructions this way.)  The same operations per lane
    // in the same order: the files do not change.  Every working lane is at record `qi` of its queue in the same round.
    while (__builtin_amdgcn_ballot_w64(act) != 0ull) {
      if (act) {
        // (a plain divergent loop: lanes whose scan has ended wait masked until the last one is done.  Written as
        // `while (ballot(scan)) if (scan) {..}` until late in round 5, the loop carried its state through a bypass block: eight
        // register copies plus a flag materialised and re-tested per pair step, 10 of its ~75 instructions)
        if (!wide) v3_scan<QN, 2, info_t>(col, info, rate_rows, lane, e, i - 1, azd_prev, f0f, d0, d1, d2, d3, best, beste, bestk);
        else v3_scan<QN, 4, info_t>(col, info, rate_rows, lane, e, i - 1, azd_prev, f0f, d0, d1, d2, d3, best, beste, bestk);
      }
      lookup();
      const bool wide_n = next_wide();
      if (act) {
        if (beste >= 0) {
          const int mag = (bestk < ncd - 1) ? (2 << bestk) - 1 : qval;
          col[nlive][lane] = make_uint2(__float_as_uint(azd_cur), __float_as_uint(best));     // live entry nlive
          if (SLIM) {
            info[nlive][lane] = (info_t)i;
            const int sh = 4 * (nlive - 1);      // (nlive >= 1; beste < nlive <= 16)
            back4 |= (unsigned long long)(unsigned)beste << sh;
            mag4 |= (unsigned long long)(unsigned)mag << sh;
          } else
          info[nlive][lane] = (info_t)((unsigned)i | ((unsigned)beste << 6) | ((unsigned)mag << 12));
          neg |= (unsigned long long)sgn << i;
          // end-of-block choice (jcdctmgr.c:1187-1207): entries appear in position order, strict '<' keeps the first minimum
          float c = best + azd63;
          c = c - azd_cur;
          if (i < 63) c = c + eobf;
          if (c < end_best) { end_best = c; last = nlive; }
          nlive++;
        }
        if (qi >= nq) act = false;
        else setup(wide_n);
      }
      wide = wide_n;
    }

    // ---- back-track (jcdctmgr.c:1211-1222) along the entry indices; values in visiting (descending position) order ----
    unsigned long long pmask = 0ull;
    int cnt = 0, e2 = work ? last : 0;
    if (CF) {
      // the same walk; the symbol of a visited entry is (zeros down to the entry the path came from, size of its magnitude): the
      // info word of that entry -- entry 0 is position 0 -- is the next iteration's, loaded one iteration early
      unsigned inf = info[e2][lane];
      {      // EOB unless the path ends at position 63; an empty path (entry 0) is an all-zero block
        const unsigned ne = (unsigned)__popcll(__builtin_amdgcn_ballot_w64(work && (SLIM ? inf : inf & 63u) < 63u));
        if (lane == 0 && ne) fh_add(MJH_FH_EOB, ne);
      }
      while (__builtin_amdgcn_ballot_w64(e2 > 0) != 0ull) {
        if (e2 > 0) {
          const int sh = 4 * (e2 - 1);
          const int mag = SLIM ? (int)((mag4 >> sh) & 15ull) : (int)(inf >> 12), pos = SLIM ? (int)inf : (int)(inf & 63u);
          const int v = ((neg >> pos) & 1ull) ? -mag : mag;
          colh[((cnt >> 2) * 64 + lane) * 4 + (cnt & 3)] = (unsigned short)v;
          pmask |= 1ull << pos;
          cnt++;
          e2 = SLIM ? (int)((back4 >> sh) & 15ull) : (int)((inf >> 6) & 63u);
          inf = info[e2][lane];
          const int run = pos - (int)(SLIM ? inf : inf & 63u) - 1;
          if (run > 15) fh_add(MJH_FH_ZRL, (unsigned)(run >> 4));
          fh_add(((run & 15) << 2) + bitlen((unsigned)mag) - 1, 1u);
        }
      }
    } else
    while (__builtin_amdgcn_ballot_w64(e2 > 0) != 0ull) {
      if (e2 > 0) {
        const unsigned inf = info[e2][lane];
        const int sh = 4 * (e2 - 1);
        const int mag = SLIM ? (int)((mag4 >> sh) & 15ull) : (int)(inf >> 12), pos = SLIM ? (int)inf : (int)(inf & 63u);
        const int v = ((neg >> pos) & 1ull) ? -mag : mag;
        colh[((cnt >> 2) * 64 + lane) * 4 + (cnt & 3)] = (unsigned short)v;
        pmask |= 1ull << pos;
        cnt++;
        e2 = SLIM ? (int)((back4 >> sh) & 15ull) : (int)((inf >> 6) & 63u);
      }
    }
    if (work) nzmask[gblk] = pmask;
    {
      int16_t *qo = coef_q + (size_t)img * C.coefs_per_image + cc.coef_off + blk;
      // plane i+1 <- the i-th non-zero in position order = slot cnt-1-i; a plane is stored only while some block has a value for it
#pragma unroll
      for (int i2 = 0; i2 < QN; i2++) {
        if (__builtin_amdgcn_ballot_w64(i2 < cnt) == 0ull) break;
        if (i2 < cnt) {
          const int s2 = cnt - 1 - i2;
          qo[(size_t)(i2 + 1) * cc.kstride] = (int16_t)colh[((s2 >> 2) * 64 + lane) * 4 + (s2 & 3)];
        }
      }
    }
    __syncthreads();
  }
  if (CF) {
    // flush once per tile: lane b owns bin b = (run & 15) * 4 + size - 1, lanes 0 and 1 also EOB and ZRL; the dummy blocks of the
    // interleaved scan (one EOB each, as k_stats_ac_compact adds them) come with the component's first tile
    __syncthreads();
    const int fslot = comp == 0 ? fin_slot_of_comp.x : comp == 1 ? fin_slot_of_comp.y : comp == 2 ? fin_slot_of_comp.z : fin_slot_of_comp.w;
    unsigned *dst = (fin_tabs + (size_t)img * slots_per_image + fslot)->counts;
    const unsigned sb = fh_get(lane);
    if (sb) atomicAdd(&dst[((lane >> 2) << 4) + (lane & 3) + 1], sb);
    if (lane < 2) {
      unsigned sx = fh_get(64 + lane);
      if (lane == 0 && tl == t0) sx += (unsigned)(cc.wpad * cc.hpad - cc.nblk);
      if (sx) atomicAdd(&dst[lane == 0 ? 0 : 0xF0], sx);
    }
  }
