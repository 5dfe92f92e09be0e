// Fragment of bhg_mlp.hip — #included there INSIDE `namespace bhg { namespace {`, after check_mlp (it uses every launch helper of the
// translation unit).  Not a header of its own.
// Here (round 6): the FACTOR-EXCHANGE form of the global-batch CG solver — the fully projected solver (DESIGN 3.5-3.6) run on
// SAMPLE-PARTITIONED data, `world` ranks, one process per GPU.  Oracle: the reference's cg (betty/hypergradient/cg.py:8-70) in ONE
// process on the concatenated batch; protocol restated in ATen in tests/proj_global_ref.py (north_star: "all-reduce partitioned across
// the 8 GPUs ... overlapped with the next CG matvec"; SURVEY.md 8(e)(2)).
//
// A Krylov vector u is known to rank g through its products with rank g's batch only,
//     Gf_l(u) = h_l U_l^T   [Bp x d_{l+1}]          Gb_l(u) = delta_l U_l   [Bp x d_l]          (wide layers l <= L-2),
// and since (H_g' v)(W_l) = Rd_l^T h_l + delta_l^T Rh_{l-1} is an outer product of BATCH-SIZED factors of rank g',
//     Gf_l^(g)(H v) = 1/G sum_g' [ (h_l^(g) h_l^(g')T) Rd_l^(g') + (h_l^(g) Rh_{l-1}^(g')T) delta_l^(g') ]  =  1/G [S_l | T_l] [Rd_l ; delta_l]
//     Gb_l^(g)(H v) = 1/G sum_g' [ (delta_l^(g) Rd_l^(g')T) h_l^(g') + (delta_l^(g) delta_l^(g')T) Rh_{l-1}^(g') ]  =  1/G [E_l | D_l] [h_l ; Rh_{l-1}]
// with RECTANGULAR Gram blocks [Bp x G Bp] (this rank's rows against every rank's samples).  Per iteration the ranks exchange
//     ONE all-gather of the factor slab   Rd_0..Rd_{L-1}, Rh_0..Rh_{L-2}   (Bp x sum of widths floats per rank: 4.07 MB at cfg 2 / Bp = 128,
//                                                                            against the 40.1 MB residual of the one-pass form)
//     ONE all-gather of 3 x ndot fp64 partials (this rank's shares of r.raw, p.raw, raw.raw on the wide layers; 22 KB at cfg 2) — summed by every
//                                          rank in rank order, so the scalars are bit-identical everywhere without relying on the collective's
//                                          reduction order
// and h_l, delta_l of all ranks once per solve.  The narrow slices (biases, head weight) stay explicit and REPLICATED: their outputs are
// sums over all samples of the gathered factors, computed redundantly (identical bits: same data, same code).  Nothing N-sized is read
// after the projections of the right-hand side in iteration 0.
//
// Every matrix product runs on the kernels the one-rank solver already has: the chain through the constant weights (k_wskpc, the head
// kernel) and, for the rectangular Gram and G(raw) products, the generic packed product k_wskp — its `outp` store IS the packed M-side
// operand of the product that consumes it ([K / 16][Bp][16] with K = the gathered samples), and two operand pairs are ONE product over
// the concatenated K ([S | T] against [Rd ; delta]: in the packed layout concatenation along K is concatenation in memory).
// New here: the pack of the gathered factors with the narrow slices' outputs riding in it (k_fx_pack), the step between two iterations —
// scalars, element-wise recurrences, Rz(x) — as ONE launch (k_fx_step); the inner products of the wide layers are emitted by the tiles of
// the G(raw) launch (k_wskpd, wskp.inc: WskpDots).
//
// Phases (bhg_mlp_cg_fx_phase; the caller does the collectives between them, all on one stream):
//     BEGIN (k = 0)   h_l, delta_l of this rank -> its slot of the constant slab                      -> all-gather the constant slab
//     CHAIN (k)       k = 0: constants packed, S_l / D_l, projections of the right-hand side (the only N-sized pass);
//                     k > 0: scalars of iteration k-1 (alpha, beta), recurrences G(r), G(p), Rh_0(p), Rz(x) += alpha Rz(p);
//                     then the R-chain on this rank's batch -> Rd_l, Rh_l in this rank's slot of the factor slab -> all-gather the factor slab
//     GRAM (k)        gathered factors packed (+ narrow outputs); T_l, E_l; G(raw) with the inner-product partials -> all-gather the partials
//     END             scalars of iteration K-1, Rz(x) complete (bhg_mlp_cg_mixed_coeff reads it).  Neumann (bhg_mlp_neumann_fx_phase): no scalars, no partials' gather; CHAIN (K) = the closing half pass, END (K): Rz(v_K) joins the sum
constexpr int kFxL = kHoistMax / 2 + 1;   // deepest net the hoist plan takes (8 layers)
constexpr int kFxKsMax = 4;                // K split of a per-iteration Gram product (FxPlan.ks)
constexpr int kFxPackMax = (2 + 2 * kFxKsMax) * kFxL + 2;
enum : int { FX_RR = 0, FX_RRW = 1, FX_RPW = 2, FX_PPW = 3, FX_ALPHA = 4, FX_BETA = 5, FX_RRNEW = 6, FX_NSCAL = 8 };

// ---- the narrow slices' outputs from the GATHERED factors (replicated: every rank computes the same bits) ---------------------------------
//   rawn|b_l = 1/G colsum over ALL ranks' samples of Rd_l          rawn|V = 1/G (Rd_{L-1}^T h_{L-1} + delta_{L-1}^T Rh_{L-2}) over all samples
// They need nothing but the gathered slabs, so they ride in the launch that packs them (k_fx_pack), off the critical path of the
// Gram -> G(raw) -> inner-products chain.  64 columns x 4 row groups per workgroup, eight rows' operands in flight per trip.
struct FxSmallArgs {
  int B, G; long long sstride, cstride;       // floats between two ranks' factor slabs / constant slabs
  const float* rd[kFxL]; int bn[kFxL]; int bblk0[kFxL + 1]; int boff[kFxL]; int L;   // rank 0's Rd_l; width; bias blocks; offset in rawn
  const float* rdL; const float* hL; const float* dL; const float* rhL; int NL, C, hoff, head_gx, head_blocks;
  float* rawn; float invG;
  const float* rn; const float* pn; float shift; double* npart; int nsb;   // this block's shares of p.raw, p.p, r.r, r.h, h.h (h = raw + shift p)
};
__device__ __forceinline__ void fx_small_body(const FxSmallArgs& a, const int sb, float (*redf)[64]) {
  const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
  float acc = 0.f;
  int64_t out_idx = -1;
  if (sb < a.head_blocks) {   // head weight: class c, 64 features
    const int c = sb / a.head_gx, n = (sb - c * a.head_gx) * 64 + col;
    const int nc = n < a.NL ? n : a.NL - 1;
    for (int g = 0; g < a.G; ++g) {
      const float* rd = a.rdL + (int64_t)g * a.sstride; const float* rh = a.rhL + (int64_t)g * a.sstride;
      const float* h = a.hL + (int64_t)g * a.cstride; const float* d = a.dL + (int64_t)g * a.cstride;
      for (int r0 = grp; r0 < a.B; r0 += 32) {
        float v0[8], v1[8], v2[8], v3[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int r = r0 + 4 * u < a.B ? r0 + 4 * u : a.B - 1;
          v0[u] = rd[(int64_t)r * a.C + c]; v1[u] = h[(int64_t)r * a.NL + nc];
          v2[u] = d[(int64_t)r * a.C + c]; v3[u] = rh[(int64_t)r * a.NL + nc];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (r0 + 4 * u < a.B) { acc = fmaf(v0[u], v1[u], acc); acc = fmaf(v2[u], v3[u], acc); }
      }
    }
    if (n < a.NL) out_idx = a.hoff + (int64_t)c * a.NL + n;
  } else {                    // biases: layer l, 64 columns
    const int bb = sb - a.head_blocks;
    int l = 0;
    while (l + 1 < a.L && bb >= a.bblk0[l + 1]) ++l;
    const int n = (bb - a.bblk0[l]) * 64 + col;
    const int W = a.bn[l];
    const int nc = n < W ? n : W - 1;
    for (int g = 0; g < a.G; ++g) {
      const float* rd = a.rd[l] + (int64_t)g * a.sstride;
      for (int r0 = grp; r0 < a.B; r0 += 32) {
        float v0[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v0[u] = rd[(int64_t)(r0 + 4 * u < a.B ? r0 + 4 * u : a.B - 1) * W + nc];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (r0 + 4 * u < a.B) acc += v0[u];
      }
    }
    if (n < W) out_idx = a.boff[l] + n;
  }
  const int64_t oc = out_idx >= 0 ? out_idx : 0;
  const float rv = a.rn[oc], pv = a.pn[oc];
  redf[grp][col] = acc;
  __syncthreads();
  if (grp == 0) {   // (one wave: the five inner products of the block's 64 outputs with the narrow state, fixed order)
    double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0, q4 = 0.0;
    if (out_idx >= 0) {
      const float v = mul_rn(a.invG, (redf[0][col] + redf[1][col]) + (redf[2][col] + redf[3][col]));
      a.rawn[out_idx] = v;
      const double hv = (double)v + (double)a.shift * (double)pv;
      q0 = (double)pv * (double)v; q1 = (double)pv * (double)pv; q2 = (double)rv * (double)rv; q3 = (double)rv * hv; q4 = hv * hv;
    }
    q0 = wave_sum(q0); q1 = wave_sum(q1); q2 = wave_sum(q2); q3 = wave_sum(q3); q4 = wave_sum(q4);
    if (col == 0) {
      a.npart[sb] = q0; a.npart[a.nsb + sb] = q1; a.npart[2 * a.nsb + sb] = q2; a.npart[3 * a.nsb + sb] = q3; a.npart[4 * a.nsb + sb] = q4;
    }
  }
}

// ---- k_fx_pack: gathered row-major factors -> the packed operands of the rectangular products ----------------------------------------
// src: rank 0's [Bp][W] array inside its slab, rank g's at src + g * stride.
//   kind 0: the N-side operand of a Gram product, [W / 16][G Bp][16]   (K = the feature index, rows = every rank's samples) — 32 x 32 tiles,
//           128-B rows in, each of the tile's two 16-feature planes 2 KB contiguous out
//   kind 1: the N-side operand of a G(raw) product, [G Bp / 16][W][16] (K = the gathered samples, rows = the feature index) —
//           a 32-sample x 32-column tile per workgroup through LDS: 128-B rows in, 2 KB contiguous out
struct FxPackProb { const float* src; float* dst; int W, kind; };
struct FxPackArgs { FxPackProb p[kFxPackMax]; int blk0[kFxPackMax + 1]; int n, G, Bp; long long stride; int small_blocks; };
static_assert(sizeof(FxPackArgs) + sizeof(FxSmallArgs) <= 3800, "kernel arguments of k_fx_pack must fit the kernarg segment");
inline int fx_pack_blocks(const FxPackProb& q, int GB) { return (GB / 32) * (q.W / 32); }   // one 32-sample x 32-column tile per workgroup
__global__ __launch_bounds__(256) void k_fx_pack(FxPackArgs g, FxSmallArgs sm) {
  __shared__ float tile[32][33];
  if ((int)blockIdx.x < g.small_blocks) {   // (dispatched first: their row loops are the launch's longest chains)
    fx_small_body(sm, blockIdx.x, reinterpret_cast<float (*)[64]>(&tile[0][0]));
    return;
  }
  const int blk = blockIdx.x - g.small_blocks;
  int i = 0;
  while (i + 1 < g.n && blk >= g.blk0[i + 1]) ++i;
  const FxPackProb q = g.p[i];
  const int lb = blk - g.blk0[i];
  const int GB = g.G * g.Bp;
  const int ntc = q.W / 32;
  const int ts = lb / ntc, tc = lb - ts * ntc;   // sample tile (32 samples: inside one rank, Bp % 32 == 0), column tile
  const int s0 = 32 * ts, j0 = 32 * tc;
  const int gr = s0 / g.Bp, b0 = s0 - gr * g.Bp;
  {
    const int s = threadIdx.x >> 3, cg = threadIdx.x & 7;   // 128-B rows in
    const f32x4 v = *reinterpret_cast<const f32x4*>(q.src + (int64_t)gr * g.stride + (int64_t)(b0 + s) * q.W + j0 + 4 * cg);
    if (q.kind == 0) {   // no transposition: the tile's two 16-feature planes leave as 2 KB contiguous each (32 rows x 64 B)
      const int j = j0 + 4 * cg;
      *reinterpret_cast<f32x4*>(q.dst + ((int64_t)(j >> 4) * GB + s0 + s) * 16 + (j & 15)) = v;
      return;
    }
    tile[s][4 * cg + 0] = v[0]; tile[s][4 * cg + 1] = v[1]; tile[s][4 * cg + 2] = v[2]; tile[s][4 * cg + 3] = v[3];
  }
  __syncthreads();
  {
    const int sbl = threadIdx.x >> 7, j = (threadIdx.x & 127) >> 2, c4 = threadIdx.x & 3;
    f32x4 v;
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = tile[16 * sbl + 4 * c4 + u][j];
    *reinterpret_cast<f32x4*>(q.dst + ((int64_t)(s0 / 16 + sbl) * q.W + j0 + j) * 16 + 4 * c4) = v;
  }
}

// ---- r.r of the (replicated) right-hand side over the WIDE weights (the narrow slices' share comes from the small-output blocks): blocks in
// proportion to the tensors' sizes, one fp64 partial each, summed in block order by k_fx_init ------------------------------------------------
constexpr int kFxRrBlocks = 1024;
struct FxRrArgs { const float* t[kFxL]; int64_t n4[kFxL]; int blk0[kFxL + 1]; int nt; double* part; };
__global__ __launch_bounds__(kThreads) void k_fx_rr(FxRrArgs a) {
  __shared__ double red[kWaves];
  int ti = 0;
  while (ti + 1 < a.nt && (int)blockIdx.x >= a.blk0[ti + 1]) ++ti;
  const int b = blockIdx.x - a.blk0[ti], nb = a.blk0[ti + 1] - a.blk0[ti];
  const float* __restrict__ x = a.t[ti];
  double acc = 0.0;
  for (int64_t i0 = (int64_t)b * kThreads + threadIdx.x; i0 < a.n4[ti]; i0 += (int64_t)4 * nb * kThreads) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { const int64_t i = i0 + (int64_t)u * nb * kThreads; v[u] = ld16(x + 4 * (i < a.n4[ti] ? i : 0)); }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i0 + (int64_t)u * nb * kThreads < a.n4[ti])
        acc += (double)v[u].x * v[u].x + (double)v[u].y * v[u].y + (double)v[u].z * v[u].z + (double)v[u].w * v[u].w;
  }
  const double s = block_sum(acc, red);
  if (threadIdx.x == 0) a.part[blockIdx.x] = s;
}
// One workgroup: the wide layers' scalars of iteration 0 (r = p = right-hand side) and the narrow slices' state (copies of the right-hand
// side's biases and head weight: rn = pn, parity slot 0; every slice starts on a 16-byte boundary, the padding and rawn are cleared).
struct FxInitArgs {
  const double* part; int npart;
  const float* src[kFxL + 1]; int off[kFxL + 1], len[kFxL + 1]; int ns, Nn;   // narrow tensors: the biases, then the head weight
  float* rn; float* pn; float* rawn; double* sc;
};
__global__ __launch_bounds__(kThreads) void k_fx_init(FxInitArgs a) {   // one element of the narrow state per thread; block 0: the scalars
  __shared__ double red[kWaves];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < a.Nn) {
    float v = 0.f;
    for (int s = 0; s < a.ns; ++s)
      if (i >= a.off[s] && i < a.off[s] + a.len[s]) v = a.src[s][i - a.off[s]];
    a.rn[i] = v; a.pn[i] = v; a.rawn[i] = 0.f;
  }
  if (blockIdx.x != 0) return;
  const double rr_w = block_sum(sum_strided<4>(a.part, a.npart, threadIdx.x, kThreads), red);
  if (threadIdx.x == 0) {
    a.sc[FX_RR] = rr_w; a.sc[FX_RRW] = rr_w; a.sc[FX_RPW] = rr_w; a.sc[FX_PPW] = rr_w;   // (parity slot 0; FX_RR: diagnostic)
    a.sc[FX_ALPHA] = 0.0; a.sc[FX_BETA] = 0.0; a.sc[FX_RRNEW] = 0.0;
  }
}
// Several device-to-device copies in one launch (BEGIN: this rank's h_l, delta_l into its slot of the constant slab).
struct FxCopyArgs { const float* src[2 * kFxL]; float* dst[2 * kFxL]; int64_t n4[2 * kFxL]; int n; };
__global__ __launch_bounds__(256) void k_fx_copy(FxCopyArgs a) {
  const int i = blockIdx.y;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < a.n4[i]; j += (int64_t)gridDim.x * 256)
    reinterpret_cast<float4*>(a.dst[i])[j] = reinterpret_cast<const float4*>(a.src[i])[j];
}

// ---- the step between two iterations: scalars, element-wise recurrences, Rz(x) — ONE launch (k_fx_step) -------------------------------------
// Scalars (cg.py:42-53 on batch-sized quantities).  Wide layers: the recurrences of DESIGN 3.6 in fp64 from the gathered partials
// scal_all [G][3][ndot] (every rank's shares of r.raw, p.raw, raw.raw over ITS samples, emitted by the G(raw) tiles: k_wskpd; summed in rank order).  Narrow slices
// (biases, head weight; explicit and replicated): five fp64 partials per small-output block (fx_small_body), all independent of the step
// length — p.raw, p.p, r.r, r.h, h.h with h = raw + shift p — so that r'.r' = r.r - 2 alpha r.h + alpha^2 h.h needs no second pass:
//   alpha = rr / (cg_alpha (p.raw + shift p.p))   (fp32 division of the fp32-rounded dots, as cg.py:45-47 on fp32 tensors and as k_cg_alpha)
//   beta  = rr' / rr
// EVERY workgroup of the launch sums the same partials in the same order to the same alpha and beta (a few KB out of L2, three
// barriers: like k_pstep of the one-rank solver) and applies them to its share:
//   [rz blocks]      Rz(x) += alpha Rz(p)                                              (fp64, as k_cg_alpha)
//   [narrow blocks]  rn' = rn - alpha (rawn + shift pn);  pn' = rn' + beta pn          (the rounding sequence of fuse_elem)
//   [update blocks]  G(r') = G(r) - alpha (G(raw) / G + shift G(p));  G(p') = G(r') + beta G(p);  first layer:
//                    Rh_0(p') = m_0 * (Gf_0(p') + p'|b0), row-major into this rank's slot of the factor slab and packed for the chain
// Nothing in the launch reads what another block of it writes: the narrow state and the scalars live in TWO slots by iteration parity
// (read old, write new); the first layer's blocks form p'|b0 themselves from the OLD slot with the narrow blocks' very operations.
// (First version: a one-workgroup scalar kernel + an update launch — 7.7 us + a launch boundary per iteration at cfg 2.)
struct FxStepHdr {
  const double* scal_all; int G, ndot; long long stride;   // doubles between two ranks' partials
  const double* npart; int nsb;                             // [5][nsb]: the narrow slices' partials (this iteration's small-output blocks)
  const double* sc_old; double* sc_new;
  float cg_alpha, shift, invG; int last;
  int neumann;   // 1: neumann.py:61-66 instead of cg.py:42-53 — no scalars at all: v' = v - alpha (H v + shift v) with the CONSTANT alpha = cg_alpha
                 // (the direction lives in the p slots; the r slots are carried along), Rz(x) = sum_k Rz(v_k)
  const float* rn_old; const float* pn_old; const float* rawn; float* rn_new; float* pn_new; int Nn;
  const float* rz; double* rzx; int nrz, rz_first, rz_blocks, narrow_blocks;
  int n, Bp, B, rh0_prod, boff0;
  const float* mask0; float* rh0; float* rh0p;
};
struct FxUpdProb { float* Gr; float* Gp; const float* Graw; int N; };
struct FxStepArgs { FxStepHdr h; FxUpdProb p[kHoistMax]; int blk0[kHoistMax + 1]; };
static_assert(sizeof(FxStepArgs) <= 3800, "kernel arguments of k_fx_step must fit the kernarg segment");
constexpr int kFxUpdU = 4;   // float4s per thread of an update block
__global__ __launch_bounds__(256) void k_fx_step(FxStepArgs a) {
  __shared__ double red[3 * kWaves];
  const FxStepHdr& h = a.h;
  const int t = threadIdx.x, b = blockIdx.x;
  // ---- this block's operands (requested before the scalar phase: loads return in order, the sums below do not wait for them twice)
  const bool is_rz = b < h.rz_blocks;
  const bool is_narrow = !is_rz && b < h.rz_blocks + h.narrow_blocks;
  const int ub = b - h.rz_blocks - h.narrow_blocks;
  int pi = 0;
  if (!is_rz && !is_narrow) while (pi + 1 < h.n && ub >= a.blk0[pi + 1]) ++pi;
  const FxUpdProb q = a.p[pi];
  const int nv = q.N / 4, total = h.Bp * nv;
  const bool first_layer = !is_rz && !is_narrow && pi == h.rh0_prod;
  float4 r0[kFxUpdU], p0[kFxUpdU], w0[kFxUpdU], mk[kFxUpdU], rb[kFxUpdU], pb[kFxUpdU], wb[kFxUpdU];
  int idx[kFxUpdU], m[kFxUpdU], n[kFxUpdU];
  bool valid[kFxUpdU];
  if (!is_rz && !is_narrow) {
#pragma unroll
    for (int u = 0; u < kFxUpdU; ++u) {
      idx[u] = ((ub - a.blk0[pi]) * kFxUpdU + u) * 256 + t;
      valid[u] = idx[u] < total;
      m[u] = valid[u] ? idx[u] / nv : 0;
      n[u] = valid[u] ? (idx[u] - m[u] * nv) * 4 : 0;
      const int ci = (valid[u] && m[u] < h.B) ? idx[u] : 0;
      r0[u] = ld16(q.Gr + (int64_t)ci * 4); p0[u] = ld16(q.Gp + (int64_t)ci * 4); w0[u] = ld16(q.Graw + (int64_t)ci * 4);
      mk[u] = ld16((first_layer ? h.mask0 : q.Gr) + (int64_t)ci * 4);
      const int nb = first_layer ? h.boff0 + n[u] : 0;
      rb[u] = ld16(h.rn_old + nb); pb[u] = ld16(h.pn_old + nb); wb[u] = ld16(h.rawn + nb);
    }
  }
  const int ne = (b - h.rz_blocks) * 256 + t;                 // narrow blocks: this thread's element
  const int nec = (is_narrow && ne < h.Nn) ? ne : 0;
  const float e_r = h.rn_old[nec], e_p = h.pn_old[nec], e_w = h.rawn[nec];
  const int ri = b * 256 + t;                                  // rz blocks: this thread's element
  const int ric = (is_rz && ri < h.nrz) ? ri : 0;
  const float e_rz = h.rz[ric];
  const double e_rzx = h.rz_first ? 0.0 : h.rzx[ric];
  // ---- the scalar phase: the same bits in every block
  const double rr_w = h.sc_old[FX_RRW], rp_w = h.sc_old[FX_RPW], pp_w = h.sc_old[FX_PPW];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  double d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0, d4 = 0.0, dz = 0.0;
  if (!h.neumann) {   // (workgroup-uniform)
    for (int g = 0; g < h.G; ++g) {   // (rank order, then index order: the same sum in every block of every rank)
      const double* p = h.scal_all + (int64_t)g * h.stride;
      for (int i = t; i < h.ndot; i += 256) { s0 += p[i]; s1 += p[h.ndot + i]; s2 += p[2 * h.ndot + i]; }
    }
    for (int i = t; i < h.nsb; i += 256) {
      d0 += h.npart[i]; d1 += h.npart[h.nsb + i]; d2 += h.npart[2 * h.nsb + i]; d3 += h.npart[3 * h.nsb + i]; d4 += h.npart[4 * h.nsb + i];
    }
    block_sum3(s0, s1, s2, red);
    block_sum3(d0, d1, d2, red);
    block_sum3(d3, d4, dz, red);
  }
  const double invG = 1.0 / (double)h.G;
  const double r_raw = s0 * invG, p_raw = s1 * invG, raw_raw = s2 * invG * invG;
  const double shift = (double)h.shift;
  const double rr = rr_w + d2;                                  // r.r = wide (recurrence) + narrow (explicit)
  const double pp = pp_w + d1;
  const double den = (double)h.cg_alpha * ((p_raw + d0) + shift * pp);
  const float alpha = h.neumann ? h.cg_alpha : (float)rr / (float)den;
  const double al = (double)alpha;
  const double rHp = r_raw + shift * rp_w, pHp = p_raw + shift * pp_w, HpHp = raw_raw + 2.0 * shift * p_raw + shift * shift * pp_w;
  const double rr_w1 = rr_w - 2.0 * al * rHp + al * al * HpHp;
  const double rp_w1 = rp_w - al * pHp;
  const double rr_n1 = d2 - 2.0 * al * d3 + al * al * d4;
  const double rr_new = rr_w1 + rr_n1;
  const float beta = (h.last || h.neumann) ? 0.f : (float)rr_new / (float)rr;
  if (b == 0 && t == 0 && !h.neumann) {
    const double bb = (double)beta;
    h.sc_new[FX_ALPHA] = al; h.sc_new[FX_BETA] = bb; h.sc_new[FX_RRNEW] = rr_new; h.sc_new[FX_RR] = rr;
    h.sc_new[FX_PPW] = rr_w1 + 2.0 * bb * rp_w1 + bb * bb * pp_w;
    h.sc_new[FX_RPW] = rr_w1 + bb * rp_w1;
    h.sc_new[FX_RRW] = rr_w1;
  }
  // ---- this block's share
  if (is_rz) {
    if (ri < h.nrz) h.rzx[ri] = e_rzx + (h.neumann ? 1.0 : al) * (double)e_rz;   // (Neumann: the plain sum of Rz(v_k))
    return;
  }
  auto narrow = [&](const float rv, const float pv, const float wv, float& rnew, float& pnew) {
    float hv = wv;
    if (h.shift != 0.f) hv = add_rn(hv, mul_rn(h.shift, pv));
    rnew = add_rn(h.neumann ? pv : rv, -mul_rn(alpha, hv));
    pnew = h.neumann ? rnew : add_rn(rnew, mul_rn(beta, pv));
  };
  if (is_narrow) {
    if (ne < h.Nn) {
      float rnew, pnew;
      narrow(e_r, e_p, e_w, rnew, pnew);
      h.rn_new[ne] = rnew; h.pn_new[ne] = pnew;
    }
    return;
  }
#pragma unroll
  for (int u = 0; u < kFxUpdU; ++u) {
    if (!valid[u]) continue;
    float4 gr = make_float4(0.f, 0.f, 0.f, 0.f), gp = gr, o = gr;
    if (m[u] < h.B) {
#define BHG_FX1(c)                                                          \
      {                                                                     \
        float hv = mul_rn(h.invG, w0[u].c);                                 \
        if (h.shift != 0.f) hv = add_rn(hv, mul_rn(h.shift, p0[u].c));      \
        gr.c = add_rn(h.neumann ? p0[u].c : r0[u].c, -mul_rn(alpha, hv));   \
        gp.c = h.neumann ? gr.c : add_rn(gr.c, mul_rn(beta, p0[u].c));      \
      }
      BHG_FX1(x) BHG_FX1(y) BHG_FX1(z) BHG_FX1(w)
#undef BHG_FX1
      if (first_layer) {
        float4 bv, rdummy;
        narrow(rb[u].x, pb[u].x, wb[u].x, rdummy.x, bv.x); narrow(rb[u].y, pb[u].y, wb[u].y, rdummy.y, bv.y);
        narrow(rb[u].z, pb[u].z, wb[u].z, rdummy.z, bv.z); narrow(rb[u].w, pb[u].w, wb[u].w, rdummy.w, bv.w);
        o.x = (gp.x + bv.x) * mk[u].x; o.y = (gp.y + bv.y) * mk[u].y; o.z = (gp.z + bv.z) * mk[u].z; o.w = (gp.w + bv.w) * mk[u].w;
      }
    }
    *reinterpret_cast<float4*>(q.Gr + (int64_t)idx[u] * 4) = gr;
    *reinterpret_cast<float4*>(q.Gp + (int64_t)idx[u] * 4) = gp;
    if (first_layer) {
      *reinterpret_cast<float4*>(h.rh0 + (int64_t)idx[u] * 4) = o;
      *reinterpret_cast<float4*>(h.rh0p + ((int64_t)(n[u] >> 4) * h.Bp + m[u]) * 16 + (n[u] & 15)) = o;
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
// Layout of the slabs the ranks exchange (floats per rank) and of the solver's own workspace (a function of the shapes and the world size).
struct FxPlan {
  bool ok;
  int L, Bp, G, GB, C;
  int ks;                                                // K split of the per-iteration Gram products T_l, E_l (see fx_gram)
  HoistPlan hp;
  size_t c_h[kFxL + 1], c_d[kFxL + 1], const_floats;     // constant slab: h_0 .. h_{L-1}, delta_1 .. delta_{L-1}
  size_t s_rd[kFxL + 1], s_rh[kFxL + 1], slab_floats;    // factor slab: Rd_0 .. Rd_{L-1}, Rh_0 .. Rh_{L-2}
  int ndot; size_t scal_doubles;                         // [3][ndot] fp64 partials per rank
  int Nn, boff[kFxL + 1], hoff;                          // narrow state: biases b_0 .. b_{L-1}, then the head weight
};
struct FxWs {
  float* Af[kFxL]; float* Ab[kFxL];      // packed M-side operands of G(raw): [S_l | T_l slabs] (l = 0: S_0), [E_l slabs | D_l]
  float* Bf[kFxL]; float* Bb[kFxL];      // packed N-side operands of G(raw): [Rd_l^T ; ks x delta_l^T] (l = 0: Rd_0^T), [ks x h_l^T ; Rh_{l-1}^T]
  float* RdP[kFxL]; float* RhP[kFxL];    // packed N-side operands of E_l (Rd_l, l >= 1) and T_{l+1} (Rh_l, l <= L-3): per iteration
  float* hP[kFxL]; float* dP[kFxL];      // ... of S_l (h_l) and D_l (delta_l): once per solve
  float* rmS[kFxL]; float* rmD[kFxL]; float* rmT[kFxL]; float* rmE[kFxL];   // row-major copies the product kernel always stores
  float* rn[2]; float* pn[2]; float* rawn;   // narrow state: two slots by iteration parity (k_fx_step reads one, writes the other)
  double* sc[2]; double* npart; double* rrpart;
  int nsb;                                     // small-output blocks (head weight + biases) = narrow partials per quantity
  size_t bytes;
};
void fx_plan(const bhg_mlp* m, int world, FxPlan* fp) {
  memset(fp, 0, sizeof(*fp));
  if (!m || world < 1 || m->L < 3 || m->L > kFxL || !use_head(m)) return;
  hoist_plan(m, &fp->hp);
  if (!fp->hp.ok || !fp->hp.proj_ok) return;
  const int L = m->L;
  fp->L = L; fp->Bp = m->Bp; fp->G = world; fp->GB = world * m->Bp; fp->C = m->dims[L];
  // K split of the per-iteration Gram products T_l, E_l.  They have (Bp / 32) (G Bp / 32) tiles each — 64 workgroups for the four of cfg 2
  // at G = 1, a quarter of the chip for 11.8 us.  Split over ks workgroups the slabs are never summed: the product that consumes them runs
  // over the concatenated K ([S | T_0 | .. | T_{ks-1}] against [Rd ; delta ; .. ; delta]: the repeated N-side blocks are CONSTANTS of the
  // solve, delta_l^T and h_l^T, packed ks times once).  MEASURED at cfg 2, G = 1 (same box, measurement build, key fx_ksplit): ks = 1 / 2 / 4:
  // 551-552 / 563-564 / 560 steps/s — the Gram launch gains (11.8 -> 7.4 us at ks = 4) what the G(raw) launch loses to its longer reduction
  // (11.8 -> 16.5 us: 944 tiles re-read 2.5 x the operands out of L2); ks = 2 is the better trade.  The tiles multiply with G, so the split is
  // taken only while the Gram launch leaves three quarters of the chip idle (G = 1 at cfg 2); key fx_ksplit = 1 / 2 / 4 overrides.
  {
    const int tiles = (m->Bp / 32) * (fp->GB / 32) * 2 * (L - 2);
    const int ks = dbg(DBG_fx_ksplit, tiles * 4 <= chip_cus() ? 2 : 1);
    fp->ks = ks == 2 ? 2 : (ks == 4 ? 4 : 1);
  }
  size_t off = 0;
  for (int l = 0; l < L; ++l) { fp->c_h[l] = off; off += (size_t)m->Bp * m->dims[l]; }
  for (int l = 1; l < L; ++l) { fp->c_d[l] = off; off += (size_t)m->Bp * m->dims[l + 1]; }
  fp->const_floats = (off + 63) & ~(size_t)63;
  off = 0;
  for (int l = 0; l < L; ++l) { fp->s_rd[l] = off; off += (size_t)m->Bp * m->dims[l + 1]; off = (off + 3) & ~(size_t)3; }
  for (int l = 0; l + 1 < L; ++l) { fp->s_rh[l] = off; off += (size_t)m->Bp * m->dims[l + 1]; }
  fp->slab_floats = (off + 63) & ~(size_t)63;
  int nd = 0;   // one partial triple per block of the G(raw) launch (block tables are rounded up to multiples of 8: the padding slots stay zero)
  for (int i = 0; i < fp->hp.n; ++i) nd += ((m->Bp / 32) * (fp->hp.N[i] / 32) + 7) & ~7;
  fp->ndot = nd;
  fp->scal_doubles = ((size_t)3 * nd + 7) & ~(size_t)7;
  int o = 0;
  for (int l = 0; l < L; ++l) { fp->boff[l] = o; o += (m->dims[l + 1] + 3) & ~3; }   // (16-byte aligned slices: the update reads b_0 as float4)
  fp->hoff = o; o += (m->dims[L] * m->dims[L - 1] + 3) & ~3;
  fp->Nn = o;
  fp->ok = true;
}
void fx_carve(const bhg_mlp* m, const FxPlan& fp, void* base, FxWs* w) {
  memset(w, 0, sizeof(*w));
  size_t off = 0;
  auto take = [&](size_t bytes) { void* p = base ? static_cast<char*>(base) + off : nullptr; off += (bytes + 255) & ~(size_t)255; return p; };
  auto takef = [&](size_t n) { return static_cast<float*>(take(sizeof(float) * n)); };
  const int L = fp.L;
  const size_t Bp = (size_t)fp.Bp, GB = (size_t)fp.GB;
  for (int l = 0; l + 1 < L; ++l) {
    w->Af[l] = takef((l >= 1 ? 1 + fp.ks : 1) * Bp * GB);
    w->Bf[l] = takef((l >= 1 ? 1 + fp.ks : 1) * GB * m->dims[l + 1]);
    w->hP[l] = takef(GB * m->dims[l]);
    w->rmS[l] = takef(Bp * GB);
    if (l >= 1) {
      w->Ab[l] = takef((1 + fp.ks) * Bp * GB);
      w->Bb[l] = takef((1 + fp.ks) * GB * m->dims[l]);
      w->RdP[l] = takef(GB * m->dims[l + 1]);
      w->RhP[l - 1] = takef(GB * m->dims[l]);
      w->dP[l] = takef(GB * m->dims[l + 1]);
      w->rmD[l] = takef(Bp * GB); w->rmT[l] = takef(fp.ks * Bp * GB); w->rmE[l] = takef(fp.ks * Bp * GB);
    }
  }
  for (int i = 0; i < 2; ++i) { w->rn[i] = takef(fp.Nn); w->pn[i] = takef(fp.Nn); w->sc[i] = static_cast<double*>(take(sizeof(double) * FX_NSCAL)); }
  w->rawn = takef(fp.Nn);
  w->nsb = ((m->dims[L - 1] + 63) / 64) * m->dims[L];
  for (int l = 0; l < L; ++l) w->nsb += (m->dims[l + 1] + 63) / 64;
  w->npart = static_cast<double*>(take(sizeof(double) * 5 * w->nsb));
  w->rrpart = static_cast<double*>(take(sizeof(double) * kFxRrBlocks));
  w->bytes = off;
}

// this rank's descriptor with Rd_l / Rh_l living inside its slot of the factor slab (what the chain writes is what the ranks gather)
inline bhg_mlp fx_local(const bhg_mlp* m, const FxPlan& fp, float* slab_all, int rank) {
  bhg_mlp d = *m;
  float* mine = slab_all + (size_t)rank * fp.slab_floats;
  for (int l = 0; l < fp.L; ++l) d.Rd[l] = mine + fp.s_rd[l];
  for (int l = 0; l + 1 < fp.L; ++l) d.Rh[l] = mine + fp.s_rh[l];
  return d;
}

int fx_launch_pack(const FxPackArgs& g_in, int blk, hipStream_t st, const FxSmallArgs* sm = nullptr, int small_blocks = 0) {
  FxPackArgs g = g_in;
  g.blk0[g.n] = blk;
  g.small_blocks = small_blocks;
  FxSmallArgs none{};
  if (blk + small_blocks > 0) hipLaunchKernelGGL(k_fx_pack, dim3(small_blocks + blk), dim3(256), 0, st, g, sm ? *sm : none);
  BHG_HIP_CHECK(hipGetLastError());
  return BHG_OK;
}

// BEGIN: this rank's h_l, delta_l into its slot of the constant slab (device-to-device copies, once per solve)
int fx_begin(const bhg_mlp* m, const FxPlan& fp, float* const_all, int rank, hipStream_t st) {
  float* mine = const_all + (size_t)rank * fp.const_floats;
  FxCopyArgs ca{};
  for (int l = 0; l < fp.L; ++l) { ca.src[ca.n] = m->h[l]; ca.dst[ca.n] = mine + fp.c_h[l]; ca.n4[ca.n++] = (int64_t)m->Bp * m->dims[l] / 4; }
  for (int l = 1; l < fp.L; ++l) { ca.src[ca.n] = m->delta[l]; ca.dst[ca.n] = mine + fp.c_d[l]; ca.n4[ca.n++] = (int64_t)m->Bp * m->dims[l + 1] / 4; }
  hipLaunchKernelGGL(k_fx_copy, dim3(64, ca.n), dim3(256), 0, st, ca);
  BHG_HIP_CHECK(hipGetLastError());
  return BHG_OK;
}

// The R-chain of this rank on its G(p) arrays: forward through W_1 .. W_{L-2}, the head, backward — the packed products of the
// one-rank solver without riders (the Gram products need the OTHER ranks' factors: they run after the exchange).
int fx_chain(const bhg_mlp* m /* fx_local */, const FxPlan& fp, const FusedWs& w, const FxWs& x, int par, hipStream_t st,
             bool stop_after_head = false) {
  const float* pn = x.pn[par];   // the direction's narrow slices of THIS iteration
  const HoistPlan* hp = &fp.hp;
  const int L = m->L, Bp = m->Bp, B = m->B;
  float* hbase = w.hoist;
  const int tn = skinny_tile_n();
  HeadFuse head_fuse{};
  for (int l = 1; l + 1 < L; ++l) {
    const int K = m->dims[l], N = m->dims[l + 1];
    const float* c = pn + fp.boff[l];
    const float* Gf = hbase + hp->g_off[hp->gf[l]];
    WskpBuilder wb;
    WskpProb q{};
    q.Ap = w.Rhp[l - 1]; q.Bq = w.Wf[l]; q.RA = Bp; q.RB = N; q.K = K; q.B = B; q.nsplit = 1;
    if (l == L - 2) {   // raw K-split slabs: the head kernel combines them (adds Gf and c_l, applies the mask)
      const int tiles_l = (Bp / 32) * (N / 32);
      int sp = chip_cus() / tiles_l;
      const int cap = pick_splits((N + tn - 1) / tn, K, 1);   // what m->partial was sized for
      if (sp > cap) sp = cap;
      if (sp > K / 64) sp = K / 64;
      if (sp < 1) sp = 1;
      q.nsplit = sp; q.raw = 1; q.out = m->partial;
      head_fuse = {m->partial, sp, Bp * N, c, m->mask[l], m->Rh[l], Gf};
    } else {
      q.bias = c; q.mask = m->mask[l]; q.addend = Gf; q.out = m->Rh[l]; q.outp = w.Rhp[l];
    }
    wb.add(q);
    wb.launch(st);
  }
  {
    const int l = L - 1, K = m->dims[l], N = m->dims[l + 1];
    launch_head_forward(st, Bp, (const float*)m->Rh[l - 1], m->h[l], m->W[l], pn + fp.hoff, pn + fp.boff[l], m->prob, m->sd, m->Rd[l], K, N, B,
                        HEAD_JVP, nullptr, nullptr, (const float*)m->delta[l], (const float*)m->mask[l - 1], m->Rd[l - 1], &head_fuse, nullptr,
                        nullptr, w.rz, nullptr, 0, w.Rdp[l - 1]);
  }
  for (int l = L - 2; l >= 1 && !stop_after_head; --l) {   // (stop_after_head: Neumann's closing half pass only needs Rz(v_K))
    const int K = m->dims[l + 1], N = m->dims[l];
    WskpBuilder wb;
    WskpProb q{};
    q.Ap = w.Rdp[l]; q.Bq = w.Wb[l]; q.RA = Bp; q.RB = N; q.K = K; q.B = B; q.nsplit = 1;
    q.mask = m->mask[l - 1]; q.addend = hbase + hp->g_off[hp->gb[l]]; q.out = m->Rd[l - 1];
    q.outp = l >= 2 ? w.Rdp[l - 1] : nullptr;
    wb.add(q);
    wb.launch(st);
  }
  BHG_HIP_CHECK(hipGetLastError());
  return BHG_OK;
}

// CHAIN, k = 0: everything that happens once per solve, then the first chain.
int fx_first(const bhg_mlp* m, const bhg_mlp* ml, const FxPlan& fp, const FusedWs& w, const FxWs& x, const void* const* rhs,
             const float* const_all, int rank, hipStream_t st, bool neumann = false) {
  const HoistPlan* hp = &fp.hp;
  const int L = m->L, Bp = m->Bp, B = m->B, G = fp.G, GB = fp.GB;
  float* hbase = w.hoist;
  if (!m->prepacked)
    if (int rc = pack_operands(m, w, st)) return rc;
  {   // gathered constants -> packed operands
    FxPackArgs g{};
    int blk = 0;
    auto add = [&](const float* src, float* dst, int W, int kind) {
      g.p[g.n] = {src, dst, W, kind};
      g.blk0[g.n] = blk;
      blk += fx_pack_blocks(g.p[g.n], GB);
      ++g.n;
    };
    g.G = G; g.Bp = Bp; g.stride = (long long)fp.const_floats;
    for (int l = 0; l + 1 < L; ++l) {
      add(const_all + fp.c_h[l], x.hP[l], m->dims[l], 0);
      if (l >= 1) {
        for (int j = 0; j < fp.ks; ++j)   // h_l^T against every K slab of E_l: [ks x h_l^T ; Rh_{l-1}^T]
          add(const_all + fp.c_h[l], x.Bb[l] + (size_t)j * GB * m->dims[l], m->dims[l], 1);
        add(const_all + fp.c_d[l], x.dP[l], m->dims[l + 1], 0);
        for (int j = 0; j < fp.ks; ++j)   // delta_l^T against every K slab of T_l: [Rd_l^T ; ks x delta_l^T]
          add(const_all + fp.c_d[l], x.Bf[l] + (size_t)(1 + j) * GB * m->dims[l + 1], m->dims[l + 1], 1);
      }
    }
    if (int rc = fx_launch_pack(g, blk, st)) return rc;
  }
  {   // S_l = h_l^(g) h_l^T, D_l = delta_l^(g) delta_l^T against every rank's samples: constants of the solve
    WskpBuilder sb;
    for (int l = 0; l + 1 < L; ++l) {
      WskpProb u{};
      u.Ap = w.hpk[l]; u.Bq = x.hP[l]; u.RA = Bp; u.RB = GB; u.K = m->dims[l]; u.B = B; u.raw = 1; u.nsplit = 1;
      u.out = x.rmS[l]; u.outp = x.Af[l];
      if (!sb.add(u)) { sb.launch(st); sb.add(u); }
      if (l >= 1) {
        u.Ap = w.dpk[l]; u.Bq = x.dP[l]; u.K = m->dims[l + 1]; u.out = x.rmD[l]; u.outp = x.Ab[l] + (size_t)fp.ks * Bp * GB;
        if (!sb.add(u)) { sb.launch(st); sb.add(u); }
      }
    }
    sb.launch(st);
  }
  {   // r.r of the right-hand side's wide slices, the scalars and the narrow state of iteration 0
    FxRrArgs ra{};
    ra.nt = L - 1; ra.part = x.rrpart;
    int64_t tot4 = 0;
    for (int l = 0; l + 1 < L; ++l) { ra.t[l] = static_cast<const float*>(rhs[2 * l]); ra.n4[l] = (int64_t)m->dims[l] * m->dims[l + 1] / 4; tot4 += ra.n4[l]; }
    int blk = 0;
    for (int l = 0; l + 1 < L; ++l) {
      int nb = (int)((ra.n4[l] * (kFxRrBlocks - kFxL) + tot4 - 1) / tot4);
      if (nb < 1) nb = 1;
      ra.blk0[l] = blk; blk += nb;
    }
    ra.blk0[L - 1] = blk;
    BHG_REQUIRE(blk <= kFxRrBlocks, "r.r block table overflow");
    if (!neumann) hipLaunchKernelGGL(k_fx_rr, dim3(blk), dim3(kThreads), 0, st, ra);   // (Neumann has no scalars: no r.r)
    FxInitArgs ia{};
    ia.part = x.rrpart; ia.npart = neumann ? 0 : blk;
    for (int l = 0; l < L; ++l) { ia.src[l] = static_cast<const float*>(rhs[2 * l + 1]); ia.off[l] = fp.boff[l]; ia.len[l] = m->dims[l + 1]; }
    ia.src[L] = static_cast<const float*>(rhs[2 * (L - 1)]); ia.off[L] = fp.hoff; ia.len[L] = m->dims[L] * m->dims[L - 1];
    ia.ns = L + 1; ia.Nn = fp.Nn;
    ia.rn = x.rn[0]; ia.pn = x.pn[0]; ia.rawn = x.rawn; ia.sc = x.sc[0];
    hipLaunchKernelGGL(k_fx_init, dim3((fp.Nn + kThreads - 1) / kThreads), dim3(kThreads), 0, st, ia);
  }
  {   // projections of the right-hand side on this rank's batch (the only N-sized reads of the solve): k_hoist + k_hoist_reduce
    HoistArgs ha{};
    HoistRedArgs ra{};
    for (int i = 0; i < hp->n; ++i) {
      const int l = hp->layer[i];
      HoistProb& q = ha.p[i];
      q.A = hp->bwd[i] ? m->delta[l] : m->h[l];
      q.Bm = static_cast<const float*>(rhs[2 * l]);
      q.slabs = hbase + hp->slab_off[i];
      q.K = hp->K[i]; q.N = hp->N[i]; q.splits = hp->splits[i]; q.rc = hp->bwd[i];
      q.lda = hp->K[i]; q.ldb = hp->bwd[i] ? hp->N[i] : hp->K[i];
      ha.blk0[i] = hp->blk0[i];
      HoistRedProb& rq = ra.p[i];
      rq.slabs = q.slabs; rq.G = hbase + hp->g_off[i]; rq.G2 = hbase + hp->gr_off[i]; rq.N = hp->N[i]; rq.splits = hp->splits[i];
      if (!hp->bwd[i] && l == 0) { rq.bias = x.pn[0] + fp.boff[0]; rq.mask = m->mask[0]; rq.out = ml->Rh[0]; rq.outp = w.Rhp[0]; }
    }
    ha.blk0[hp->n] = hp->blk0[hp->n];
    ha.n = hp->n; ha.Bp = Bp; ha.gemm_blocks = hp->blk0[hp->n];
    hipLaunchKernelGGL(k_hoist<FUSE_CG>, dim3(ha.gemm_blocks), dim3(256), 0, st, ha);
    ++g_hoist_launches;
    int rblk = 0;
    for (int i = 0; i < hp->n; ++i) { ra.blk0[i] = rblk; rblk += (Bp * (hp->N[i] / 4) + 255) / 256; }
    ra.blk0[hp->n] = rblk;
    ra.n = hp->n; ra.Bp = Bp; ra.B = B; ra.first = 1; ra.scal = nullptr;
    hipLaunchKernelGGL(k_hoist_reduce, dim3(rblk), dim3(256), 0, st, ra);
  }
  BHG_HIP_CHECK(hipGetLastError());
  (void)rank;
  return BHG_OK;
}

// The step after iteration kprev (CHAIN of iteration kprev + 1; END: last = 1 — only alpha_{K-1} and Rz(x) are needed)
int fx_step(const bhg_mlp* ml, const FxPlan& fp, const FusedWs& w, const FxWs& x, const double* scal_all, int kprev, bool last,
            float cg_alpha, float shift, hipStream_t st, bool neumann = false) {
  const HoistPlan* hp = &fp.hp;
  const int Bp = ml->Bp, B = ml->B;
  float* hbase = w.hoist;
  const int po = kprev & 1, pw = po ^ 1;
  FxStepArgs sa{};
  FxStepHdr& h = sa.h;
  h.scal_all = scal_all; h.G = fp.G; h.ndot = fp.ndot; h.stride = (long long)fp.scal_doubles;
  h.npart = x.npart; h.nsb = x.nsb; h.sc_old = x.sc[po]; h.sc_new = x.sc[pw];
  h.cg_alpha = cg_alpha; h.shift = shift; h.invG = 1.0f / (float)fp.G; h.last = last ? 1 : 0; h.neumann = neumann ? 1 : 0;
  h.rn_old = x.rn[po]; h.pn_old = x.pn[po]; h.rawn = x.rawn; h.rn_new = x.rn[pw]; h.pn_new = x.pn[pw]; h.Nn = fp.Nn;
  h.rz = w.rz; h.rzx = w.rzx; h.nrz = B * fp.C; h.rz_first = kprev == 0 ? 1 : 0; h.rz_blocks = (B * fp.C + 255) / 256;
  h.narrow_blocks = last ? 0 : (fp.Nn + 255) / 256;
  h.n = hp->n; h.Bp = Bp; h.B = B; h.rh0_prod = hp->gf[0]; h.boff0 = fp.boff[0];
  h.mask0 = ml->mask[0]; h.rh0 = ml->Rh[0]; h.rh0p = w.Rhp[0];
  int ublk = 0;
  for (int i = 0; i < hp->n; ++i) {
    sa.p[i] = {hbase + hp->gr_off[i], hbase + hp->g_off[i], hbase + hp->graw_off[i], hp->N[i]};
    sa.blk0[i] = ublk;
    ublk += (Bp * (hp->N[i] / 4) + 256 * kFxUpdU - 1) / (256 * kFxUpdU);
  }
  sa.blk0[hp->n] = ublk;
  const int grid = h.rz_blocks + h.narrow_blocks + (last ? 0 : ublk);
  hipLaunchKernelGGL(k_fx_step, dim3(grid), dim3(256), 0, st, sa);
  ++g_proj_iterations;
  BHG_HIP_CHECK(hipGetLastError());
  return BHG_OK;
}

// GRAM: the gathered factors packed, the rectangular Gram products of this iteration, G(raw), the closing launch
int fx_gram(const bhg_mlp* ml, const FxPlan& fp, const FusedWs& w, const FxWs& x, const float* slab_all, const float* const_all,
            double* scal_mine, int par, float shift, hipStream_t st) {
  const HoistPlan* hp = &fp.hp;
  const int L = ml->L, Bp = ml->Bp, B = ml->B, G = fp.G, GB = fp.GB;
  float* hbase = w.hoist;
  {
    FxPackArgs g{};
    int blk = 0;
    auto add = [&](const float* src, float* dst, int W, int kind) {
      g.p[g.n] = {src, dst, W, kind};
      g.blk0[g.n] = blk;
      blk += fx_pack_blocks(g.p[g.n], GB);
      ++g.n;
    };
    g.G = G; g.Bp = Bp; g.stride = (long long)fp.slab_floats;
    for (int l = 0; l + 1 < L; ++l) {
      add(slab_all + fp.s_rd[l], x.Bf[l], ml->dims[l + 1], 1);                                   // Rd_l^T: first half of [Rd_l^T ; delta_l^T]
      if (l >= 1) {
        add(slab_all + fp.s_rd[l], x.RdP[l], ml->dims[l + 1], 0);                                // Rd_l: N side of E_l
        add(slab_all + fp.s_rh[l - 1], x.RhP[l - 1], ml->dims[l], 0);                            // Rh_{l-1}: N side of T_l
        add(slab_all + fp.s_rh[l - 1], x.Bb[l] + (size_t)fp.ks * GB * ml->dims[l], ml->dims[l], 1);   // Rh_{l-1}^T: the tail of [ks x h_l^T ; Rh_{l-1}^T]
      }
    }
    FxSmallArgs sa{};
    sa.B = B; sa.G = G; sa.sstride = (long long)fp.slab_floats; sa.cstride = (long long)fp.const_floats;
    int bblk = 0;
    for (int l = 0; l < L; ++l) {
      sa.rd[l] = slab_all + fp.s_rd[l]; sa.bn[l] = ml->dims[l + 1]; sa.boff[l] = fp.boff[l];
      sa.bblk0[l] = bblk; bblk += (ml->dims[l + 1] + 63) / 64;
    }
    sa.bblk0[L] = bblk; sa.L = L;
    sa.rdL = slab_all + fp.s_rd[L - 1]; sa.rhL = slab_all + fp.s_rh[L - 2];
    sa.hL = const_all + fp.c_h[L - 1]; sa.dL = const_all + fp.c_d[L - 1];
    sa.NL = ml->dims[L - 1]; sa.C = fp.C; sa.hoff = fp.hoff; sa.head_gx = (sa.NL + 63) / 64; sa.head_blocks = sa.head_gx * sa.C;
    sa.rawn = x.rawn; sa.invG = 1.0f / (float)G;
    sa.rn = x.rn[par]; sa.pn = x.pn[par]; sa.shift = shift; sa.npart = x.npart; sa.nsb = x.nsb;
    BHG_REQUIRE(sa.head_blocks + bblk == x.nsb, "small-output block count of the plan and of the launch disagree");
    if (int rc = fx_launch_pack(g, blk, st, &sa, sa.head_blocks + bblk)) return rc;
  }
  {   // T_l = h_l^(g) Rh_{l-1}^T, E_l = delta_l^(g) Rd_l^T  [Bp x G Bp], stored packed as the second / first half of the M-side operands
    WskpBuilder gb;
    for (int l = 1; l + 1 < L; ++l) {
      WskpProb t{};
      t.Ap = w.hpk[l]; t.Bq = x.RhP[l - 1]; t.RA = Bp; t.RB = GB; t.K = ml->dims[l]; t.B = B; t.raw = 1; t.nsplit = fp.ks;
      t.out = x.rmT[l]; t.outp = x.Af[l] + (size_t)Bp * GB;   // (K slab j: packed at + j Bp GB, contiguous = concatenated along K)
      if (!gb.add(t)) { gb.launch(st); gb.add(t); }
      t.Ap = w.dpk[l]; t.Bq = x.RdP[l]; t.K = ml->dims[l + 1]; t.out = x.rmE[l]; t.outp = x.Ab[l];
      if (!gb.add(t)) { gb.launch(st); gb.add(t); }
    }
    gb.launch(st);
  }
  {   // G(raw) = [S | T slabs] [Rd ; delta ..]  /  [E slabs | D] [h .. ; Rh]: one product over the concatenated K = (1 + ks) G Bp (first layer: G Bp);
      // the tiles emit this rank's shares of r.raw, p.raw, raw.raw on their way (k_wskpd) — no launch of its own for the inner products
    int slot = 0;
    for (int i0 = 0; i0 < hp->n; i0 += kWskpMax) {
      WskpdArgs wa{};
      int blk = 0;
      for (int i = i0; i < hp->n && i < i0 + kWskpMax; ++i) {
        const int l = hp->layer[i];
        WskpProb q{};
        q.RA = Bp; q.RB = hp->N[i]; q.B = B; q.raw = 1; q.nsplit = 1;
        if (!hp->bwd[i]) { q.Ap = x.Af[l]; q.Bq = x.Bf[l]; q.K = (l >= 1 ? 1 + fp.ks : 1) * GB; }
        else { q.Ap = x.Ab[l]; q.Bq = x.Bb[l]; q.K = (1 + fp.ks) * GB; }
        q.out = hbase + hp->graw_off[i];
        wskp_tiling(&q, false);
        const int j = wa.g.n++;
        wa.g.p[j] = q;
        wa.g.blk0[j] = blk;
        wa.d[j] = {hp->bwd[i] ? (const float*)ml->Rh[l - 1] : (const float*)ml->Rd[l], hbase + hp->gr_off[i], hbase + hp->g_off[i], scal_mine,
                   slot + blk, fp.ndot};
        blk += (q.nfull * (q.RB / 32) + 7) & ~7;
      }
      wa.g.blk0[wa.g.n] = blk;
      hipLaunchKernelGGL(k_wskpd<2>, dim3(blk), dim3(64 * kWskpWaves), 0, st, wa);
      slot += blk;
    }
    BHG_REQUIRE(slot == fp.ndot, "tile count of the G(raw) launch and of the plan disagree");
  }
  BHG_HIP_CHECK(hipGetLastError());
  return BHG_OK;
}
