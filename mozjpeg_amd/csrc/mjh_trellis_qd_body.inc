// Body of k_trellis_ac_qd and k_trellis_ac_qd_cf (mjh_trellis.hip): included once in each, so that the plain kernel keeps its name,
// its argument list and its machine code.  The including kernel defines CF (count the final AC symbols of the blocks it finishes),
// fin_tabs and fin_slot_of_comp (CF only: where the counts go) in front of the #include.
  static_assert(!CF || COMPACT, "the final symbols are counted from compact records");
  __shared__ uint2 col[QN2][64];
  __shared__ unsigned short e_pk[QN2 + 1][64];
  __shared__ int dqT[4][64];
  __shared__ float ltT[4][64];
  const int lane = threadIdx.x;
#pragma unroll
  for (int t = 0; t < 4; t++) { dqT[t][lane] = Q->dq8[t][lane]; ltT[t][lane] = Q->lambda_tbl[t][lane]; }
  __syncthreads();
  const unsigned count = worklist[0];
  for (unsigned base = blockIdx.x * 64; base < count; base += gridDim.x * 64) {   // wave-uniform trip count
    const unsigned it = base + lane;
    const bool active = it < count;
    const unsigned ii = active ? it : count - 1;
    const int img = (int)worklist[4 + 3 * (size_t)ii];
    const unsigned w = worklist[5 + 3 * (size_t)ii];
    const unsigned ds = worklist[6 + 3 * (size_t)ii];
    const int comp = (int)(w >> 28);
    const MjhComp cc = C.c[comp];
    const int blk = (int)(w & 0x0FFFFFFFu);
    const int slot = comp == 0 ? ac_slot_of_comp.x : comp == 1 ? ac_slot_of_comp.y : comp == 2 ? ac_slot_of_comp.z : ac_slot_of_comp.w;
    const MjhHuffTable *T = tabs + (size_t)img * slots_per_image + slot;
    const float lambda = lambda_in[(size_t)img * C.total_real_blocks + cc.blk_off + blk];
    int nq;
    float azd63;
    {
      short xs[64];
      if (ds < dense_cap) {
        const uint4 *d = reinterpret_cast<const uint4 *>(dense + (size_t)ds * 64);
#pragma unroll
        for (int v = 0; v < 8; v++) {
          const uint4 q4 = d[v];
          const unsigned ww[4] = { q4.x, q4.y, q4.z, q4.w };
#pragma unroll
          for (int j = 0; j < 4; j++) { xs[8 * v + 2 * j] = (short)(ww[j] & 0xFFFFu); xs[8 * v + 2 * j + 1] = (short)(ww[j] >> 16); }
        }
      } else {
        const int16_t *uq = coef_uq + (size_t)img * C.coefs_per_image + cc.coef_off + blk;
#pragma unroll
        for (int k = 1; k < 64; k++) xs[k] = uq[(size_t)k * cc.kstride];
      }
      if (EXT && ext.qstride) {
        const MjhQuant *Qi = Q + (size_t)img * ext.qstride;   // per-lane image: vector loads of its own rows
        nq = trellis_q_phase1<QN2, EXT>(xs, Qi->dq8[cc.qtbl], Qi->rcp8q[cc.qtbl], Qi->lambda_tbl[cc.qtbl], lambda, col, lane, azd63, ext.Ss, ext.Se);
      } else
      nq = trellis_q_phase1<QN2, EXT>(xs, dqT[cc.qtbl], Q->rcp8q[cc.qtbl], ltT[cc.qtbl], lambda, col, lane, azd63, ext.Ss, ext.Se);
      if (QN2 < 63) defer_blocks(active && nq > QN2, worklist_next, (unsigned)img, w, ds, xs, nullptr, 0u, false, lane);
    }
    int16_t *qo = coef_q + (size_t)img * C.coefs_per_image + cc.coef_off + blk;
    const size_t gblk = (size_t)img * C.total_real_blocks + cc.blk_off + blk;
    if (CF) {
      unsigned long long rmask = 0ull;
      int rcnt = -1;      // stays -1: no block, or handed on to the next list
      trellis_q_walk<QN2, false, EXT, COMPACT, true>(reinterpret_cast<const uint4 *>(T->ehufsi), nullptr, dqT, ltT, cc.qtbl, nq, azd63, lambda, active, qo, cc.kstride,
                                                     col, e_pk, lane, ext.Ss, ext.Se, nullptr, nullptr, ext.nzmask + gblk, nullptr, nullptr, &rmask, &rcnt);
      typedef unsigned __attribute__((may_alias)) u_alias;
      const int fslot = comp == 0 ? fin_slot_of_comp.x : comp == 1 ? fin_slot_of_comp.y : comp == 2 ? fin_slot_of_comp.z : fin_slot_of_comp.w;
      count_final_records(rcnt >= 0, rmask, rcnt, col, reinterpret_cast<u_alias *>(&e_pk[0][0]), fin_tabs,
                          (unsigned)img * (unsigned)slots_per_image + (unsigned)fslot, lane);
    } else
    trellis_q_walk<QN2, false, EXT, COMPACT>(reinterpret_cast<const uint4 *>(T->ehufsi), nullptr, dqT, ltT, cc.qtbl, nq, azd63, lambda, active, qo, cc.kstride,
                                                              col, e_pk, lane, ext.Ss, ext.Se, EXT && ext.eob_cost ? ext.eob_cost + gblk : nullptr,
                                                              EXT && ext.eob_cost ? ext.eob_has + gblk : nullptr, COMPACT ? ext.nzmask + gblk : nullptr,
                                                              EXT && ext.qstride ? (Q + (size_t)img * ext.qstride)->dq8[cc.qtbl] : nullptr,
                                                              EXT && ext.qstride ? (Q + (size_t)img * ext.qstride)->lambda_tbl[cc.qtbl] : nullptr);
    __syncthreads();   // the LDS columns are reused by the next round
  }
