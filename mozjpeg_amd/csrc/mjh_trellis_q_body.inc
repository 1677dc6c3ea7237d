// Body of k_trellis_ac_q and k_trellis_ac_q_cf (mjh_trellis.hip): included once in each, so that the plain kernel keeps its name,
// its argument list and its machine code.  The including kernel defines CF (count the final AC symbols of the blocks it finishes),
// fin_tabs and fin_slot_of_comp (CF only: where the counts go) in front of the #include.
  static_assert(QN >= 16 && QN <= 63, "queue capacity");
  static_assert(!CF || COMPACT, "the final symbols are counted from compact records");
  __shared__ uint2 col[QN][64];                  // queue records, then live entries {azd, acc}, then the value column
  __shared__ unsigned short e_pk[QN + 1][64];    // back position | magnitude << 6 of live entry e
  __shared__ uint4 si_rows[16];
  __shared__ float4 rate_rows[16];
  __shared__ int dqT[1][64];
  __shared__ float ltT[1][64];
  // flattened grid: blockIdx.x counts the waves of all components of one image (wave0_of_comp = first wave of each)
  const int img = blockIdx.y;
  const int wv = blockIdx.x;
  const int comp = wv >= wave0_of_comp.w ? 3 : wv >= wave0_of_comp.z ? 2 : wv >= wave0_of_comp.y ? 1 : 0;
  const int w0 = comp == 0 ? 0 : comp == 1 ? wave0_of_comp.y : comp == 2 ? wave0_of_comp.z : wave0_of_comp.w;
  const MjhComp cc = C.c[comp];
  const int lane = threadIdx.x;
  const int slot = comp == 0 ? ac_slot_of_comp.x : comp == 1 ? ac_slot_of_comp.y : comp == 2 ? ac_slot_of_comp.z : ac_slot_of_comp.w;
  const MjhHuffTable *T = tabs + (size_t)img * slots_per_image + slot;
  const int blk = (wv - w0) * 64 + lane;
  const bool inside = blk < cc.nblk;
  const float lambda = lambda_in[(size_t)img * C.total_real_blocks + cc.blk_off + (inside ? blk : cc.nblk - 1)];
  if (lane < 16) {
    const uint4 r = reinterpret_cast<const uint4 *>(T->ehufsi)[lane];
    si_rows[lane] = r;
    rate_rows[lane] = rate_row(r);
  }
  if (EXT) Q += (size_t)img * ext.qstride;
  dqT[0][lane] = Q->dq8[cc.qtbl][lane];
  ltT[0][lane] = Q->lambda_tbl[cc.qtbl][lane];
  int nq;
  float azd63;
  {
    // all 63 raw coefficients at once (coalesced lines, one burst); they are dead after phase 1 / the dense copy
    const int16_t *uq = coef_uq + (size_t)img * C.coefs_per_image + cc.coef_off + (inside ? blk : cc.nblk - 1);
    short xs[64];
#pragma unroll
    for (int k = 1; k < 64; k++) xs[k] = uq[(size_t)k * cc.kstride];
    nq = trellis_q_phase1<QN, EXT>(xs, Q->dq8[cc.qtbl], Q->rcp8q[cc.qtbl], Q->lambda_tbl[cc.qtbl], lambda, col, lane, azd63, ext.Ss, ext.Se);
    defer_blocks(inside && nq > QN, worklist, (unsigned)img, ((unsigned)comp << 28) | (unsigned)blk, 0u, xs, dense, dense_cap, true, lane);
    if (!EXT) count_heavy(worklist, inside, nq, lane);
  }
  __syncthreads();
  int16_t *qo = coef_q + (size_t)img * C.coefs_per_image + cc.coef_off + blk;
  const size_t gblk = (size_t)img * C.total_real_blocks + cc.blk_off + (inside ? blk : 0);
  if (CF) {
    unsigned long long rmask = 0ull;
    int rcnt = -1;      // stays -1: outside the component, or handed on to the work list
    trellis_q_walk<QN, true, EXT, COMPACT, true>(si_rows, rate_rows, dqT, ltT, 0, nq, azd63, lambda, inside, qo, cc.kstride, col, e_pk, lane,
                                                 ext.Ss, ext.Se, nullptr, nullptr, ext.nzmask + gblk, nullptr, nullptr, &rmask, &rcnt);
    typedef unsigned __attribute__((may_alias)) u_alias;
    const int fslot = comp == 0 ? fin_slot_of_comp.x : comp == 1 ? fin_slot_of_comp.y : comp == 2 ? fin_slot_of_comp.z : fin_slot_of_comp.w;
    const unsigned key = (unsigned)img * (unsigned)slots_per_image + (unsigned)fslot;
    count_final_records(rcnt >= 0, rmask, rcnt, col, reinterpret_cast<u_alias *>(&e_pk[0][0]), fin_tabs, key, lane);
    // the dummy blocks of the interleaved scan: one EOB each, once per image and component
    if (wv == w0 && lane == 0 && cc.wpad * cc.hpad > cc.nblk) atomicAdd(&(fin_tabs + key)->counts[0], (unsigned)(cc.wpad * cc.hpad - cc.nblk));
    return;
  }
  trellis_q_walk<QN, true, EXT, COMPACT>(si_rows, rate_rows, dqT, ltT, 0, nq, azd63, lambda, inside, qo, cc.kstride, col, e_pk, lane,
                                         ext.Ss, ext.Se, EXT && ext.eob_cost ? ext.eob_cost + gblk : nullptr, EXT && ext.eob_cost ? ext.eob_has + gblk : nullptr,
                                         COMPACT ? ext.nzmask + gblk : nullptr);
