// Fragment of bhg_mlp.hip — #included there INSIDE `namespace bhg { namespace {`, in this order: gemm, outer, scalars, head, wsk,
// (host: launch helpers), recurrence, proj.  Not a header of its own.
// Here: hoisted direction products (k_hoist, k_hoist_reduce) and the projected solvers' kernels (k_proj_scalars / _update / _step).

// ---- hoisted direction products (fused CG solver, BHG_MLP_HOIST) ----------------------------------------------------------
// Half of the R-chain's matrix work does not depend on the chain at all, only on the direction: the forward products
// Gf_l = h_l V_l^T (every MFMA layer) and the backward products Gb_l = delta_l V_l (every layer behind the first).  And
// they are LINEAR in the direction, which the lazy CG direction is a two-term sum of:  p_k = r_k + beta p_{k-1}  =>
//     G(p_k) = G(r_k) + beta * G(p_{k-1})          (batch-sized arrays, kept from iteration to iteration)
// So ONE grouped launch at the top of the iteration (k_hoist) forms every G(r_k) — reading the residual alone: no
// second operand, no mixing in the loaders, and no step of the chain in front of it, not even beta: the blocks behind the
// GEMM tiles of the same launch do k_cg_beta's work — and k_hoist_reduce turns the split-K slabs into G(p_k).  What stays on
// the dependent chain are the products with the constant weights, Rh_{l-1} W_l^T and Rd_l W_l: one operand pair, half the K
// loop, run in the in-workgroup split-K form whose epilogue adds G (no slabs, no reduce launch).  One fill / drain for
// half of the chain's flops instead of five; 9 dependent launches per iteration instead of 12.
struct HoistProb {
  const float* A;      // [Bp][K] batch-sized and iteration-invariant: h_l (forward) / delta_l (backward)
  const float* Bm;     // residual slice of the W_l-shaped state: [N][K] (forward, K-contiguous) / [K][N] (backward)
  float* slabs;        // [splits][Bp][N]  (splits == 1: the product itself)
  int K, N, splits, rc, lda, ldb;
  const float* A2;     // optional second operand pair with the same layouts and leading dimensions (projected CG:
  const float* B2m;    // G(raw) = S Rd + T delta, two B x B Gram matrices times two batch-sized arrays); NULL = one pair
  const float* X;      // fully projected CG: the tiles also emit <X, G(raw)> — raw.raw's share of this product (GemmArgs.dotX)
  int a_slabs, a2_slabs, a_slab_stride;   // > 1: A / A2 arrive as K-split slabs (GemmPair.a_slabs)
};
constexpr int kHoistMax = 14;
// Fully projected CG: partials of  r.raw = sum_l <Rd_l, Gf_l(r)> + <Rh_{l-1}, Gb_l(r)>  and  p.raw (the same with G(p)) over the
// MFMA layers' weight slices — the inner products of the N-sized residual / direction with the N-sized outer products, from
// batch-sized arrays (see k_proj_scalars).  One float4 per thread, one (r.raw, p.raw) pair of fp64 partials per block.
// (raw.raw has the same form with G(raw) in place of G(r): <raw_l, raw_l> = <Rd_l, Gf_l(raw)> + <Rh_{l-1}, Gb_l(raw)> — the tiles that
//  form G(raw) emit it themselves, GemmArgs.dotX.  Round 3's first form took it from Gram matrices, <S_l, Rd_l Rd_l^T> +
//  2 <E_l^T, T_l> + <D_l, Rh Rh^T>: five more B x B x K products per iteration.)
struct ProjDotProb { const float* Gr; const float* Gp; const float* X; int N; };
// One dot block takes kDotUnroll x 256 float4 of its problem: a quarter of the partials k_proj_step's blocks each sum again.
constexpr int kDotUnroll = 4;
constexpr int dot_blocks_of(int float4s) { return ((float4s + 255) / 256 + kDotUnroll - 1) / kDotUnroll; }
constexpr int kProjDotMax = kHoistMax;
// The small slices' outputs (head weight, biases) with their fused CG epilogue, as block classes of k_hoist (fully projected CG:
// they are all that is left of k_outer_all).  Compact twin of BiasArgs (the hoisted forms take at most 8 layers).
constexpr int kSmallL = kHoistMax / 2 + 1;
struct BiasArgsC {
  const float* rd[kSmallL]; const float* c[kSmallL]; float* out[kSmallL];
  int n[kSmallL]; int blk0[kSmallL + 1]; int L, B; float rho2; int64_t foff[kSmallL];
  const float* d0; const float* d1;   // see BiasArgs
};
struct SmallOutArgs {
  HeadOuterArgs head; FuseArgs hf; int head_gx, head_blocks, head_has_rh;
  BiasArgsC ba; FuseArgs bf; int bias_blocks;
};
struct HoistArgs {
  HoistProb p[kHoistMax];
  int blk0[kHoistMax + 1];
  int n, Bp, gemm_blocks, do_beta;
  BetaArgs beta;
  int beta_blocks;               // blocks [gemm_blocks, gemm_blocks + beta_blocks): k_cg_beta's work (do_beta)
  int dot_blocks, nd, B;         // then dot_blocks blocks of the projected inner products (fully projected CG)
  ProjDotProb dp[kProjDotMax];
  int dblk0[kProjDotMax + 1];
  double* part_dot;              // [2][dot_blocks]: r.raw, p.raw
  double* part_raw;              // [gemm_blocks]: raw.raw, one partial per G(raw) tile (HoistProb.X)
  int small_blocks;              // then the small slices' output blocks (head_blocks + bias_blocks)
  SmallOutArgs so;
  int do_alpha; AlphaArgs alpha; // the step length is computed HERE, by every small block for itself (round 4: no launch of its own)
};

static_assert(sizeof(HoistArgs) <= 3800, "kernel arguments of k_hoist must fit the kernarg segment");
constexpr int kHoistLds = GemmLds<LAYOUT_KC, LAYOUT_KC, 32>::FLOATS > GemmLds<LAYOUT_KC, LAYOUT_RC, 32>::FLOATS
                              ? GemmLds<LAYOUT_KC, LAYOUT_KC, 32>::FLOATS : GemmLds<LAYOUT_KC, LAYOUT_RC, 32>::FLOATS;
template <int SMODE>   // epilogue of the small slices' output blocks: FUSE_CG / FUSE_NEUMANN
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_hoist(HoistArgs ha) {
  __shared__ __attribute__((aligned(16))) float smem[kHoistLds];
  const int b = blockIdx.x;
  if (b >= ha.gemm_blocks) {
    const int e = b - ha.gemm_blocks;
    if (e < ha.beta_blocks) {   // the scalar work between two iterations rides behind the tiles (cg.py:51-53, see k_cg_beta)
      if (ha.do_beta) beta_body(ha.beta, e);
      return;
    }
    // projected inner products: block d of product i
    const int d = e - ha.beta_blocks;
    if (d >= ha.dot_blocks) {   // small slices' outputs, CG epilogue (r' = r - alpha Hp on their slices + partials)
      const int sb = d - ha.dot_blocks;
      FuseArgs hf = ha.so.hf, bf = ha.so.bf;
      if (SMODE == FUSE_CG && ha.do_alpha) {   // (workgroup-uniform) the same partials, the same order, the same alpha in every block
        const float al = alpha_compute(ha.alpha, sb == 0);
        hf.alpha_ready = 1; hf.alpha = al;
        bf.alpha_ready = 1; bf.alpha = al;
      }
      if (sb < ha.so.head_blocks) {
        if (ha.so.head_has_rh) head_outer_body<true, SMODE>(ha.so.head, hf, sb % ha.so.head_gx, sb / ha.so.head_gx, ha.so.head_gx, smem);
        else head_outer_body<false, SMODE>(ha.so.head, hf, sb % ha.so.head_gx, sb / ha.so.head_gx, ha.so.head_gx, smem);
      } else {
        bias_body<SMODE>(ha.so.ba, bf, sb - ha.so.head_blocks, smem);
      }
      return;
    }
    int i = 0;
    while (i + 1 < ha.nd && d >= ha.dblk0[i + 1]) ++i;
    const ProjDotProb q = ha.dp[i];
    const int nv = q.N / 4;
    double ar = 0.0, ap = 0.0;
#pragma unroll
    for (int u = 0; u < kDotUnroll; ++u) {
    const int64_t idx = ((int64_t)(d - ha.dblk0[i]) * kDotUnroll + u) * 256 + threadIdx.x;
    if (idx < (int64_t)ha.Bp * nv && (int)(idx / nv) < ha.B) {
      const float4 gr = ld16(q.Gr + idx * 4);
      const float4 xv = ld16(q.X + idx * 4), gp = ld16(q.Gp + idx * 4);
      ar += (double)xv.x * gr.x + (double)xv.y * gr.y + (double)xv.z * gr.z + (double)xv.w * gr.w;
      ap += (double)xv.x * gp.x + (double)xv.y * gp.y + (double)xv.z * gp.z + (double)xv.w * gp.w;
    }
    }
    double* red = reinterpret_cast<double*>(smem);
    const double sr = block_sum(ar, red);
    const double sp = block_sum(ap, red);
    if (threadIdx.x == 0) { ha.part_dot[d] = sr; ha.part_dot[ha.dot_blocks + d] = sp; }
    return;
  }
  int i = 0;
  while (i + 1 < ha.n && b >= ha.blk0[i + 1]) ++i;
  const int t = b - ha.blk0[i];
  GemmArgs a{};
  a.pr[0].A = ha.p[i].A; a.pr[0].B = ha.p[i].Bm; a.pr[0].lda = ha.p[i].lda; a.pr[0].ldb = ha.p[i].ldb;
  a.pairs = 1;
  if (ha.p[i].A2) {
    a.pr[1].A = ha.p[i].A2; a.pr[1].B = ha.p[i].B2m; a.pr[1].lda = ha.p[i].lda; a.pr[1].ldb = ha.p[i].ldb; a.pairs = 2;
    if (ha.p[i].splits == 2) a.pair_split = 1;   // one workgroup per operand pair: two slabs, half the K loop each
  }
  a.M = ha.Bp; a.N = ha.p[i].N; a.K = ha.p[i].K; a.splits = ha.p[i].splits;
  a.out = ha.p[i].slabs; a.ldo = a.N; a.out_rows = ha.Bp; a.nt_out = 1; a.xpose_out = 1;
  if (ha.p[i].X && ha.part_raw) { a.dotX = ha.p[i].X; a.dot_out = ha.part_raw + b; }
  const int ntn = a.N / 32, ntm = ha.Bp / kTM;
  const int bx = t % ntn, by = (t / ntn) % ntm, bz = t / (ntn * ntm);
  a.pr[0].a_slabs = ha.p[i].a_slabs; a.pr[1].a_slabs = ha.p[i].a2_slabs;
  a.pr[0].a_slab_stride = a.pr[1].a_slab_stride = ha.p[i].a_slab_stride;
  if (ha.p[i].rc) {
    if (ha.p[i].a_slabs > 1 || ha.p[i].a2_slabs > 1) gemm_body<LAYOUT_KC, LAYOUT_RC, 32, true, false, true>(a, bx, by, bz, smem);
    else gemm_body<LAYOUT_KC, LAYOUT_RC, 32, true, false>(a, bx, by, bz, smem);
  } else gemm_body<LAYOUT_KC, LAYOUT_KC, 32, true, false>(a, bx, by, bz, smem);
}

// G(p_k)[m][n] = sum_s slabs[s][m][n] + beta * G(p_{k-1})[m][n]   (rows >= B zero; first iteration: no second term), and for
// the first layer's forward product also Rh_0 = mask_0 * (G + c_0).  One float4 per thread; fixed summation order.
struct HoistRedProb {
  const float* slabs; float* G; int N, splits;
  const float* bias; const float* mask; float* out;   // out != NULL: out = mask * (G + bias)
  float* G2;                                          // projected CG, first iteration: G(r_0) = G(p_0), kept separately
  float* outp;                                        // packed copy of out ([N / 16][Bp][16], wskp.inc) or NULL
  float* Gp_wr;                                       // != NULL: G(p') is written here, not over G(p) (a product whose old G(p) is read by
                                                      // other workgroups of the same launch: k_wskpl)
};
struct HoistRedArgs {
  HoistRedProb p[kHoistMax];
  int blk0[kHoistMax + 1];
  int n, Bp, B, first;
  const double* scal;
};
__global__ __launch_bounds__(256) void k_hoist_reduce(HoistRedArgs ra) {
  const int b = blockIdx.x;
  int i = 0;
  while (i + 1 < ra.n && b >= ra.blk0[i + 1]) ++i;
  const HoistRedProb pr = ra.p[i];
  const int nv = pr.N / 4;
  const int64_t total = (int64_t)ra.Bp * nv;
  const int64_t idx = (int64_t)(b - ra.blk0[i]) * 256 + threadIdx.x;
  if (idx >= total) return;
  const int m = (int)(idx / nv), n = (int)(idx - (int64_t)m * nv) * 4;
  const int64_t slab = (int64_t)ra.Bp * pr.N;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (m < ra.B) {
    constexpr int NB = 8;
    const float* p0 = pr.slabs + idx * 4;
    float4 gp = make_float4(0.f, 0.f, 0.f, 0.f), bv = gp, mv = make_float4(1.f, 1.f, 1.f, 1.f);
    if (!ra.first) gp = ld16(pr.G + idx * 4);
    if (pr.out) { if (pr.bias) bv = ld16(pr.bias + n); if (pr.mask) mv = ld16(pr.mask + idx * 4); }
    for (int s0 = 0; s0 < pr.splits; s0 += NB) {
      float4 t[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) t[u] = ld16(p0 + (int64_t)(s0 + u < pr.splits ? s0 + u : pr.splits - 1) * slab);
#pragma unroll
      for (int u = 0; u < NB; ++u)
        if (s0 + u < pr.splits) { v.x += t[u].x; v.y += t[u].y; v.z += t[u].z; v.w += t[u].w; }
    }
    if (!ra.first) {   // the two roundings of p = r + (beta * p_old), applied to the products instead of the operands
      const float beta = (float)ra.scal[S_BETA];
      v.x = add_rn(v.x, mul_rn(beta, gp.x)); v.y = add_rn(v.y, mul_rn(beta, gp.y));
      v.z = add_rn(v.z, mul_rn(beta, gp.z)); v.w = add_rn(v.w, mul_rn(beta, gp.w));
    }
    *reinterpret_cast<float4*>(pr.G + idx * 4) = v;
    if (pr.G2) *reinterpret_cast<float4*>(pr.G2 + idx * 4) = v;
    if (pr.out) {
      float4 o;
      o.x = (v.x + bv.x) * mv.x; o.y = (v.y + bv.y) * mv.y; o.z = (v.z + bv.z) * mv.z; o.w = (v.w + bv.w) * mv.w;
      *reinterpret_cast<float4*>(pr.out + idx * 4) = o;
      if (pr.outp) *reinterpret_cast<float4*>(pr.outp + ((int64_t)(n >> 4) * ra.Bp + m) * 16 + (n & 15)) = o;
    }
  } else {
    *reinterpret_cast<float4*>(pr.G + idx * 4) = v;
    if (pr.G2) *reinterpret_cast<float4*>(pr.G2 + idx * 4) = v;
    if (pr.out) *reinterpret_cast<float4*>(pr.out + idx * 4) = v;
    if (pr.outp) *reinterpret_cast<float4*>(pr.outp + ((int64_t)(n >> 4) * ra.Bp + m) * 16 + (n & 15)) = v;
  }
}

// ---- fully projected CG: the scalars of an iteration without an N-sized residual ------------------------------------------
// With G(r), G(p) projected, the solve needs the N-sized residual and direction for ONE thing only: the dots r'.r' (-> beta,
// next alpha) and p.p (-> the shift's share of p.Hp).  They follow from the recurrences as well — on the MFMA layers' slices
//     r'.r' = r.r - 2 a r.Hp + a^2 Hp.Hp,   Hp = raw + shift p
//     r.Hp  = r.raw + shift r.p          p.Hp = p.raw + shift p.p          Hp.Hp = raw.raw + 2 shift p.raw + shift^2 p.p
//     r.raw = sum_l <Rd_l, Gf_l(r)> + <Rh_{l-1}, Gb_l(r)>     (p.raw alike: the dot blocks of k_hoist)
//     raw.raw = sum_l <Rd_l Rd_l^T, S_l> + 2 <E_l^T, T_l> + <D_l, Rh_{l-1} Rh_{l-1}^T>     (B x B Gram matrices, k_wsk_group)
//     r'.p = r.p - a p.Hp ;  next:  r.p <- r'.r' + b r'.p ,  p.p <- r'.r' + 2 b r'.p + b^2 p.p
// in fp64, while the small slices (biases, head weight) stay explicit: their epilogues (k_outer_all's head / bias blocks) emit
// their share of r'.r', r'.p, p.p as before.  So after iteration 0 NO kernel reads or writes an N-sized state vector: what
// is left of an iteration is the R-chain through the constant weights and batch-sized work.  (CPU emulation in fp32 against
// the reference's fp64 run at full size: 1e-7 ... 2e-6 on the well-conditioned variant, r.r falling smoothly through
// twenty orders of magnitude; GPU: tests/test_cfg2_goldens.py.)  One workgroup.
struct ProjScalArgs {
  const double* part_dot; int dot_blocks;                        // [2][dot_blocks]: r.raw, p.raw (k_hoist's dot blocks)
  const double* part_raw; int raw_blocks;                        // raw.raw: one partial per tile of the G(raw) launch
  const double* part; int part_stride; int off0, n0, off1, n1;   // the small slices' epilogue partials [3][stride]
  const float* r_small; float* p_small;                          // flat r / p (small slices only)
  int64_t soff[BHG_MLP_MAX_LAYERS + 1]; int slen[BHG_MLP_MAX_LAYERS + 1]; int snt;
  double* scal; double* pscal;   // pscal: {rr_big, rp_big, pp_big} x 2, ping-pong by iteration parity
  float shift; int first, kpar;
};
// A few blocks (one thread per element of the small slices); every block recomputes the same scalars from the same partials in
// the same order, block 0 publishes them (like k_cg_beta).  The previous iteration's {rr, rp, pp} are read from the OTHER
// parity slot of pscal, so no block can see block 0's new values.
// (bias 0 of the direction may be read at p0_rd and written at p0_wr instead of in place: k_proj_step)
// Two phases: proj_scalars_load() only ISSUES this thread's loads (its element of the small slices, the scalars, its strided
// shares of the partial arrays); proj_scalars_finish() sums, publishes and applies.  k_proj_step issues the operand loads of the
// recurrences BETWEEN the two: loads return in order, so the wait for the partials does not wait for the operands behind them,
// and both round trips to the Infinity Cache overlap.
struct ProjScalRegs {
  int64_t eoff; int etensor, eidx; bool alt0 /* write at p0_wr (proj_scalars_finish's argument) */, fits;
  float* alt_wr;   // != NULL: this thread's element of the direction is written HERE (a slotted bias slice), not in place
  float rv, pv;
  double rr_old, al, pin0, pin1, pin2;
  StridedRegs<4> d0, d1, d2;
  double q0[2], q1[2], q2[2];
};
// (i) this thread's element of the small slices (small blocks only) — (ii) proj_scalars_load: scalars and partials
__device__ __forceinline__ void proj_small_elem(const ProjScalArgs& a, const int bx, const bool small,
                                                const float* __restrict__ p0_rd, ProjScalRegs& R) {
  const int t = threadIdx.x;
  // this thread's element of the small slices: loads first (independent of the sums)
  const int gi = bx * kThreads + t;
  int64_t eoff = -1;
  int etensor = -1, eidx = 0;
  if (small) {
    int base = 0;
    for (int tt = 0; tt < a.snt; ++tt) {
      if (eoff < 0 && gi < base + a.slen[tt]) { eoff = a.soff[tt] + (gi - base); etensor = tt; eidx = gi - base; }
      base += a.slen[tt];
    }
  }
  const bool alt0 = etensor == 0 && p0_rd != nullptr;
  float rv = 0.f, pv = 0.f;
  if (eoff >= 0) { rv = a.r_small[eoff]; pv = alt0 ? p0_rd[eidx] : a.p_small[eoff]; }
  R.eoff = eoff; R.etensor = etensor; R.eidx = eidx; R.alt_wr = nullptr; R.alt0 = alt0; R.rv = rv; R.pv = pv;
}
template <class SA>   // ProjScalArgs, or k_pstep's copy of its scalar fields (no arrays: nothing left for the stack)
__device__ __forceinline__ void proj_scalars_load(const SA& a, ProjScalRegs& R) {
  const int t = threadIdx.x;
  // the scalars thread 0 needs AFTER the sums are requested BEFORE them (uniform addresses: scalar loads) — one round trip to
  // the Infinity Cache for the whole scalar phase instead of two (stamps: 5 us of the launch's 7 were this phase)
  R.rr_old = a.scal[S_RR_OLD];          // r.r of this iteration (k_cg_alpha)
  R.al = a.scal[S_ALPHA_RING + a.kpar];
  R.pin0 = a.pscal[4 * (a.kpar ^ 1)]; R.pin1 = a.pscal[4 * (a.kpar ^ 1) + 1]; R.pin2 = a.pscal[4 * (a.kpar ^ 1) + 2];
  // partial sums: every array's loads are issued before the first add (one round trip, see strided_load)
  const int ns = a.n0 + a.n1;
  R.fits = a.dot_blocks <= 4 * kThreads && a.raw_blocks <= 4 * kThreads && ns <= 2 * kThreads;   // (uniform)
  if (R.fits) {
    strided_load(R.d0, a.part_dot, a.dot_blocks, t, kThreads, a.scal);
    strided_load(R.d1, a.part_dot + a.dot_blocks, a.dot_blocks, t, kThreads, a.scal);
    strided_load(R.d2, a.part_raw, a.raw_blocks, t, kThreads, a.scal);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = t + u * kThreads;
      const int ic = i < ns ? i : 0;
      const int j = ic < a.n0 ? a.off0 + ic : a.off1 + (ic - a.n0);
      R.q0[u] = a.part[j]; R.q1[u] = a.part[a.part_stride + j]; R.q2[u] = a.part[2 * (int64_t)a.part_stride + j];
    }
  }
}
// gran (publishing block only, may be NULL): beta is also left in 64 replicated granules for the workgroups of the SAME launch that
// poll for it (k_wskpl, poll_beta).
template <class SA>
__device__ __forceinline__ float proj_scalars_finish(const SA& a, const ProjScalRegs& R, const bool publish,
                                                     const float* __restrict__ p0_rd, float* __restrict__ p0_wr,
                                                     unsigned long long* __restrict__ gran = nullptr) {
  __shared__ double red[6][kWaves];
  __shared__ float s_beta;
  const int t = threadIdx.x;
  const int64_t eoff = R.eoff;
  const int eidx = R.eidx;
  const bool alt0 = R.alt0;
  const float rv = R.rv, pv = R.pv;
  const double rr_old_pre = R.rr_old, al_pre = R.al, pin0 = R.pin0, pin1 = R.pin1, pin2 = R.pin2;
  double ar = 0.0, ap = 0.0, ag = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
  const int ns = a.n0 + a.n1;
  if (R.fits) {
    ar = strided_sum(R.d0, a.dot_blocks, t, kThreads);
    ap = strided_sum(R.d1, a.dot_blocks, t, kThreads);
    ag = strided_sum(R.d2, a.raw_blocks, t, kThreads);
#pragma unroll
    for (int u = 0; u < 2; ++u)
      if (t + u * kThreads < ns) { s0 += R.q0[u]; s1 += R.q1[u]; s2 += R.q2[u]; }
  } else {
    for (int i = t; i < a.dot_blocks; i += kThreads) { ar += a.part_dot[i]; ap += a.part_dot[a.dot_blocks + i]; }
    for (int i = t; i < a.raw_blocks; i += kThreads) ag += a.part_raw[i];
    for (int i = t; i < ns; i += kThreads) {
      const int j = i < a.n0 ? a.off0 + i : a.off1 + (i - a.n0);
      s0 += a.part[j]; s1 += a.part[a.part_stride + j]; s2 += a.part[2 * (int64_t)a.part_stride + j];
    }
  }
  // six fixed-order sums with ONE barrier (wave sums, then the waves in order: block_sum's order, value for value)
  {
    const double v[6] = {ar, ap, ag, s0, s1, s2};
    const int lane = t & 63, wv = t >> 6;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const double ws = wave_sum(v[q]);
      if (lane == 0) red[q][wv] = ws;
    }
  }
  __syncthreads();
  BHG_STAMP(1, 3);
  if (t == 0) {
    double tot[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      double acc = 0.0;
#pragma unroll
      for (int i = 0; i < kWaves; ++i) acc += red[q][i];
      tot[q] = acc;
    }
    const double r_raw = tot[0], p_raw = tot[1], raw_raw = tot[2], rr_s = tot[3], rp_s = tot[4], pp_s = tot[5];
    const double rr_old = rr_old_pre;
    const double al = al_pre, sh = (double)a.shift;
    double* pout = a.pscal + 4 * a.kpar;
    double rr_b, rp_b, pp_b;
    // first iteration: p = r (bhg_cg_init), so the small slices' share of r.r is their p.p partial of this very iteration
    if (a.first) rr_b = rp_b = pp_b = rr_old - pp_s;
    else { rr_b = pin0; rp_b = pin1; pp_b = pin2; }
    const double rHp = r_raw + sh * rp_b, pHp = p_raw + sh * pp_b, HpHp = raw_raw + 2.0 * sh * p_raw + sh * sh * pp_b;
    const double rr_b1 = rr_b - 2.0 * al * rHp + al * al * HpHp;
    const double rp_b1 = rp_b - al * pHp;              // r'.p over the MFMA layers
    const double rr1 = rr_b1 + rr_s, rp1 = rp_b1 + rp_s, pp = pp_b + pp_s;
    const float beta = (float)rr1 / (float)rr_old;     // fp32 division of the fp32-rounded dots, as the reference (cg.py:51-52)
    const double b = (double)beta;
    if (publish) {
      a.scal[S_RR_NEW] = rr1;
      a.scal[S_BETA] = b;
      a.scal[S_PP] = rr1 + 2.0 * b * rp1 + b * b * pp;
      pout[0] = rr_b1;
      pout[1] = rr_b1 + b * rp_b1;
      pout[2] = rr_b1 + 2.0 * b * rp_b1 + b * b * pp_b;
    }
    s_beta = beta;
  }
  __syncthreads();
  if (publish && gran && t < 64)
    (void)__hip_atomic_exchange(gran + 8 * t, (1ull << 32) | (unsigned long long)__builtin_bit_cast(unsigned, s_beta), __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT);
  // cg.py:53 for the small slices (biases, head weight): p = r' + beta p
  if (eoff >= 0) {
    const float np = add_rn(rv, mul_rn(s_beta, pv));
    if (R.alt_wr) R.alt_wr[eidx] = np; else if (alt0) p0_wr[eidx] = np; else a.p_small[eoff] = np;
  }
  return s_beta;
}
__device__ __forceinline__ float proj_scalars_body(const ProjScalArgs& a, const int bx, const bool publish, const bool small,
                                                   const float* __restrict__ p0_rd, float* __restrict__ p0_wr) {
  ProjScalRegs R;
  proj_small_elem(a, bx, small, p0_rd, R);
  proj_scalars_load(a, R);
  return proj_scalars_finish(a, R, publish, p0_rd, p0_wr);
}
// The scalars as a launch of their own (BHG_PROJ_STEP_ALONE; the default merges them into the next iteration's k_proj_step): it
// runs alone because the chain of the next iteration and k_proj_update (Rh_0 needs the first bias direction) read the slices.
#ifdef BHG_AB   // (round 6: an arm of the measurement build only — key proj_step_alone; no plan of the product reaches it)
__global__ __launch_bounds__(kThreads) void k_proj_scalars(ProjScalArgs a) {
  (void)proj_scalars_body(a, blockIdx.x, blockIdx.x == 0, true, nullptr, nullptr);
}
#endif

// ---- projected CG (BHG_MLP_PROJ, default on): the direction products WITHOUT the N-sized operand ---------------------------
// The products G(.) are linear, and the residual itself obeys r' = r - alpha (raw + shift p) with raw = H p's weight-shaped
// outputs — outer products of batch-sized factors:  raw(W_l) = Rd_l^T h_l + delta_l^T Rh_{l-1}.  So
//     Gf_l(raw) = h_l raw(W_l)^T  = (h_l h_l^T) Rd_l       + (h_l Rh_{l-1}^T) delta_l   = S_l Rd_l + T_l delta_l
//     Gb_l(raw) = delta_l raw(W_l) = (delta_l Rd_l^T) h_l  + (delta_l delta_l^T) Rh_{l-1} = E_l h_l + D_l Rh_{l-1}
// with B x B Gram matrices (S_l, D_l once per solve; T_l, E_l per iteration: k_wsk_group) and batch-deep products
// (k_hoist with two operand pairs, K = batch): ~0.2 GFLOP instead of the 2.75 GFLOP of k_hoist on the residual, and no pass
// over the N-sized state at all.  The recurrences (k_proj_update, at the top of the next iteration):
//     G(r_{k+1}) = G(r_k) - alpha_k (G(raw_k) + shift G(p_k))        G(p_{k+1}) = G(r_{k+1}) + beta_k G(p_k)
// Only iteration 0 reads the N-sized residual (k_hoist on the initial vector).  Checked against the reference's CPU goldens
// on the well-conditioned full-size variant like every other arm (tests/test_cfg2_goldens.py); fp32 emulation on the CPU
// beforehand: 1e-6 from the fp64 truth, the same as the direct form and as the reference itself.
struct ProjProb {
  float* Gr; float* Gp; const float* Graw; const float* Graw2 /* second slab of G(raw) or NULL */; int N;
  const float* bias; const float* mask; float* out;   // out != NULL: out = mask * (Gp + bias)   (first layer: Rh_0)
  float* outp;                                        // packed copy of out ([N / 16][Bp][16], wskp.inc) or NULL
  float* Gp_wr;                                       // != NULL: G(p') is written here, not over G(p) (a product whose old G(p) is read by
                                                      // other workgroups of the same launch: k_wskpl)
};
struct ProjArgs {
  ProjProb p[kHoistMax];
  int blk0[kHoistMax + 1];
  int n, Bp, B, kpar_prev;
  float shift;
  const double* scal;   // CG: alpha_{k-1}, beta_{k-1}.  NULL: Neumann — G(v') = G(v) - alpha (G(raw) + shift G(v)) with the constant
  float alpha;          // step `alpha` (Gr and Gp then name the same array)
};
// b0: bias 0 of the coming direction is formed here, r'_b0 + beta * p_b0_old (k_proj_step; the very roundings of the small slices'
// update), instead of read from pr.bias.
// beta_fn: called by EVERY thread of the block exactly once, after all of this thread's operand loads have been issued — in
// k_proj_step it is the scalar phase (block-wide sums, barriers), whose round trip to the Infinity Cache then overlaps the
// operands'.  All loads are unconditional (clamped element, dummy array) for the same reason as in k_graw.
struct ProjCommon { int Bp, B, kpar_prev; float shift, alpha; const double* scal; float* rb0_copy /* != NULL: r|b0 is copied there (k_graw reads it while its bias blocks update the slice) */; };
template <int U, class PreFn, class BetaFn>
__device__ __forceinline__ void proj_update_one(const ProjProb& pr, const ProjCommon& pa, const int lb, const PreFn& pre_fn,
                                                const BetaFn& beta_fn, const float* __restrict__ r_b0, const float* __restrict__ p_b0_old);
template <class PreFn, class BetaFn>
__device__ __forceinline__ void proj_update_body(const ProjArgs& pa, const int b, const PreFn& pre_fn, const BetaFn& beta_fn,
                                                 const float* __restrict__ r_b0, const float* __restrict__ p_b0_old) {
  int i = 0;
  while (i + 1 < pa.n && b >= pa.blk0[i + 1]) ++i;
  const ProjProb pr = pa.p[i];
  const ProjCommon c{pa.Bp, pa.B, pa.kpar_prev, pa.shift, pa.alpha, pa.scal, nullptr};
  proj_update_one<1>(pr, c, b - pa.blk0[i], pre_fn, beta_fn, r_b0, p_b0_old);
}
template <int U, class PreFn, class BetaFn>
__device__ __forceinline__ void proj_update_one(const ProjProb& pr, const ProjCommon& pa, const int lb, const PreFn& pre_fn,
                                                const BetaFn& beta_fn, const float* __restrict__ r_b0, const float* __restrict__ p_b0_old) {
  pre_fn();   // (the scalar phase's loads go out FIRST: loads return in order)
  // U float4 per thread (block lb owns float4s [lb * 256 U, (lb + 1) * 256 U), thread t every 256th of them): every block repeats
  // the scalar phase — ~12 KB of partials out of L2 per block — so FEWER, fatter blocks repeat it less often (k_pstep: U = 4)
  // (row = index / nv without an integer division — ~200 VALU instructions each in 64 bits, and inside k_wskpl these waves share
  //  their SIMDs with an MFMA-dense K loop: the launch's longest chain was this block's ADDRESS arithmetic, 6.8 us before its last
  //  load was requested; stamps of round 4.  (index + 0.5) / nv in fp32 is exact for index < 2^20 — the quotient is at least
  //  0.5 / nv away from an integer, the rounding error a few ulp of it; first failure at index 2.0 M — and hoist_plan takes the
  //  projected forms only below that bound.)
  const int nv = pr.N / 4;
  const int total = pa.Bp * nv;
  const float rcp_nv = 1.0f / (float)nv;
  const bool own_b0 = pr.out && pr.bias && r_b0;
  const bool has_bq = pr.out && pr.bias && !r_b0;
  int idx[U];
  bool valid[U];
  int m[U], n[U];
  float4 r0[U], p0[U], w0[U], w1[U], mk[U], rb[U], pb[U], bq[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    idx[u] = (lb * U + u) * 256 + (int)threadIdx.x;
    valid[u] = idx[u] < total;
    m[u] = valid[u] ? (int)(((float)idx[u] + 0.5f) * rcp_nv) : 0;
    n[u] = valid[u] ? (idx[u] - m[u] * nv) * 4 : 0;
    const bool live = valid[u] && m[u] < pa.B;
    const int ci = live ? idx[u] : 0;   // (a padding row / a thread past the end reads element 0 and discards it)
    r0[u] = ld16(pr.Gr + ci * 4); p0[u] = ld16(pr.Gp + ci * 4);
    // (Graw == NULL: G(r) already holds r' — k_graw applied the step itself; element 0 of G(r) is read instead and discarded)
    w0[u] = ld16((pr.Graw ? pr.Graw : pr.Gr) + (pr.Graw ? ci * 4 : 0));
    w1[u] = ld16((pr.Graw2 ? pr.Graw2 : pr.Gr) + (pr.Graw2 ? ci * 4 : 0));
    mk[u] = ld16((pr.out && pr.mask ? pr.mask : pr.Gr) + ci * 4);
    rb[u] = ld16((own_b0 ? r_b0 : pr.Gr) + (own_b0 ? n[u] : 0)); pb[u] = ld16((own_b0 ? p_b0_old : pr.Gr) + (own_b0 ? n[u] : 0));
    bq[u] = ld16((has_bq ? pr.bias : pr.Gr) + (has_bq ? n[u] : 0));
  }
  const float alpha = pa.scal ? (float)pa.scal[S_ALPHA_RING + pa.kpar_prev] : pa.alpha;
  BHG_STAMP(1, 2);
  const float beta = beta_fn();
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (!valid[u]) continue;
    if (own_b0 && pa.rb0_copy && m[u] == 0) *reinterpret_cast<float4*>(pa.rb0_copy + n[u]) = rb[u];
    float4 gr = make_float4(0.f, 0.f, 0.f, 0.f), gp = gr;
    if (m[u] < pa.B) {
      float4 wv = w0[u];
      if (pr.Graw2) { wv.x += w1[u].x; wv.y += w1[u].y; wv.z += w1[u].z; wv.w += w1[u].w; }
      float4 bv = make_float4(0.f, 0.f, 0.f, 0.f), mv = make_float4(1.f, 1.f, 1.f, 1.f);
      if (pr.out) {
        if (own_b0) {
          bv.x = add_rn(rb[u].x, mul_rn(beta, pb[u].x)); bv.y = add_rn(rb[u].y, mul_rn(beta, pb[u].y));
          bv.z = add_rn(rb[u].z, mul_rn(beta, pb[u].z)); bv.w = add_rn(rb[u].w, mul_rn(beta, pb[u].w));
        } else if (pr.bias) {
          bv = bq[u];
        }
        if (pr.mask) mv = mk[u];
      }
      // the rounding sequence of the N-sized recurrences (fuse_elem): Hp = raw + shift p; r' = r - alpha Hp; p' = r' + beta p
#define BHG_PROJ1(c)                                                                  \
      {                                                                               \
        float hv = wv.c;                                                              \
        if (pa.shift != 0.f) hv = add_rn(hv, mul_rn(pa.shift, p0[u].c));              \
        gr.c = pr.Graw ? sub_rn(r0[u].c, mul_rn(alpha, hv)) : r0[u].c;                \
        gp.c = pa.scal ? add_rn(gr.c, mul_rn(beta, p0[u].c)) : gr.c;                  \
      }
      BHG_PROJ1(x) BHG_PROJ1(y) BHG_PROJ1(z) BHG_PROJ1(w)
#undef BHG_PROJ1
      if (pr.Graw) *reinterpret_cast<float4*>(pr.Gr + idx[u] * 4) = gr;
      *reinterpret_cast<float4*>((pr.Gp_wr ? pr.Gp_wr : pr.Gp) + idx[u] * 4) = gp;
      if (pr.out) {
        float4 o;
        o.x = (gp.x + bv.x) * mv.x; o.y = (gp.y + bv.y) * mv.y; o.z = (gp.z + bv.z) * mv.z; o.w = (gp.w + bv.w) * mv.w;
        *reinterpret_cast<float4*>(pr.out + idx[u] * 4) = o;
        if (pr.outp) *reinterpret_cast<float4*>(pr.outp + ((int64_t)(n[u] >> 4) * pa.Bp + m[u]) * 16 + (n[u] & 15)) = o;
      }
    } else if (pr.out) {
      *reinterpret_cast<float4*>(pr.out + idx[u] * 4) = gr;
      if (pr.outp) *reinterpret_cast<float4*>(pr.outp + ((int64_t)(n[u] >> 4) * pa.Bp + m[u]) * 16 + (n[u] & 15)) = gr;
    }
  }
}
__global__ __launch_bounds__(256) void k_proj_update(ProjArgs pa) {
  proj_update_body(pa, blockIdx.x, []() {}, [&]() { return pa.scal ? (float)pa.scal[S_BETA] : 0.f; }, nullptr, nullptr);
}

// Fully projected CG, default: the scalars of iteration k-1 and the recurrences of iteration k in ONE launch (one dependent
// launch less per iteration).  Every block sums the same partials in the same order to the same beta (a few KB out of L2);
// the blocks behind the update blocks own the small slices' direction update and the first of them publishes the scalars.
// Nothing in this launch reads what another block of it writes: the update blocks of the first layer need the coming first
// bias direction — they form it themselves from r'_b0 and the OLD p_b0, which the small blocks leave alone (the new one goes to
// the other of two slots, p0_wr; every later reader of that slice is pointed at the slot of its iteration's parity).
struct ProjStepArgs {
  ProjArgs pa; ProjScalArgs sa;
  int update_blocks;
  const float* r_b0; const float* p0_rd; float* p0_wr;
};
static_assert(sizeof(ProjStepArgs) <= 3800, "kernel arguments of k_proj_step must fit the kernarg segment");
#ifdef BHG_AB   // (round 6: the product's plans all take k_pstep — the same work with its arguments laid out for two round trips; key pstep_v2 = 0)
__global__ __launch_bounds__(256) void k_proj_step(ProjStepArgs g) {
  const int b = blockIdx.x;
  kernarg_warm<sizeof(ProjStepArgs)>();
  BHG_STAMP(1, 0);
  const bool small = b >= g.update_blocks;
  const int sb = small ? b - g.update_blocks : 0;
  if (small) {
    (void)proj_scalars_body(g.sa, sb, sb == 0, true, g.p0_rd, g.p0_wr);
  } else {   // the operands of the recurrences are in flight while the block sums the partials to beta
    ProjScalRegs R;
    proj_update_body(g.pa, b, [&]() { proj_small_elem(g.sa, 0, false, g.p0_rd, R); proj_scalars_load(g.sa, R); },
                     [&]() { const float be = proj_scalars_finish(g.sa, R, false, g.p0_rd, g.p0_wr); BHG_STAMP(1, 1); return be; },
                     g.r_b0, g.p0_rd);
  }
  BHG_STAMP(1, 4);
}
#endif
