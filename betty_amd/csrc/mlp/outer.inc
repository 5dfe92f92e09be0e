// Fragment of bhg_mlp.hip — #included there INSIDE `namespace bhg { namespace {`, in this order: gemm, outer, scalars, head, wsk,
// (host: launch helpers), recurrence, proj.  Not a header of its own.
// Here: fused CG / Neumann epilogues (fuse_elem), k_outer (weight-shaped outputs), split-K reduce kernels.

// ---- fused recurrence epilogues ("one pass": the weight-shaped HVP output never round-trips through HBM) ------
// Instead of storing H*direction, the kernels that produce it (k_outer, k_head_outer, k_bias_hvp) apply the
// CG / Neumann recurrence to the matching slices of the flat state vectors while the tile is still on chip:
//   FUSE_CG       Hp = raw + shift*p ; r <- r - alpha*Hp ; x <- x + alpha*p [x <- out_scale*x] ; partial r'.r'
//                 (cg.py:47-51; alpha = rr / (cg_alpha * p.Hp) was computed BEFORE these kernels from the batch-sized
//                 factors of the R-chain — see k_cg_alpha — so there is no N-sized H*p vector at all)
//   FUSE_NEUMANN  Hv = raw + shift*v ; v' <- v - alpha*Hv (written to the OTHER direction buffer: the R-backward
//                 GEMMs of this HVP still read v) ; p <- p + v' [p <- out_scale*p]          (neumann.py:62-64,66)
// Same rounding sequence as bhg_vector.hip's recurrence kernels (products rounded before add/sub, never contracted).
enum : int { FUSE_NONE = 0, FUSE_CG = 1, FUSE_NEUMANN = 2 };
struct FuseArgs {
  float* a;          // CG: r (in/out)          Neumann: v_out (out)
  float* b;          // CG: x (in/out)          Neumann: p (in/out)
  float* d;          // the direction slice:    CG: p (in; in/out when lazy)    Neumann: v_in (in)
  const double* scal;  // CG: device scalars, alpha = scal[S_ALPHA], beta = scal[S_BETA]
  double* part;        // CG: per-workgroup partials -> part[q * part_stride + part_base + linear block id],
  int part_base;       //     q = 0: r'.r'   q = 1: r'.p   q = 2: p.p   (p = this iteration's direction)
  int part_stride;
  float alpha;       // Neumann: step length (host constant); CG with alpha_ready: computed by the calling kernel itself
  int alpha_ready;   // 1: `alpha` holds it | 2: it will be at *alpha_lds (LDS) once the body's first barrier has passed (k_graw)
  const float* alpha_lds;
  int kpar;          // CG: iteration parity (alpha of iteration k lives in scal[S_ALPHA_RING + (k & 1)])
  float shift;       // operator = raw HVP + shift * I
  float out_scale;   // applied to x (CG) / p (Neumann) when apply_out != 0: the final scaling + negation of the solve
  int apply_out;
  int x_mode;        // CG, lazy slices only: 0 = x += alpha*p | 1 = leave x alone this iteration | 2 = catch up:
                     // x = (x + alpha_prev*p_old) + alpha*p — the very two roundings of two separate updates, with x read
                     // and written every OTHER iteration only (p_old, last iteration's direction, is loaded anyway)
  int lazy;          // CG: the slice at d still holds the PREVIOUS direction; this iteration's is r + beta * d — formed
                     // here (same roundings as k_cg_pdir) and written back, so no kernel of its own updates it (cg.py:53)
};
struct FuseAcc { double rr, rp, pp; };
// one element: hv = raw HVP value, dv = direction (CG lazy: previous direction), av / bv = the two state values;
// results back in av / bv, the direction actually used back in dv.
template <int MODE>
__device__ __forceinline__ void fuse_elem(const FuseArgs& f, float alpha, float beta, float hv, float& dv, float& av,
                                          float& bv, FuseAcc& acc, float alpha_prev = 0.f) {
  const float d_old = dv;
  if (MODE == FUSE_CG && f.lazy) dv = add_rn(av, mul_rn(beta, dv));
  if (f.shift != 0.f) hv = add_rn(hv, mul_rn(f.shift, dv));
  if (MODE == FUSE_CG) {
    const float nr = sub_rn(av, mul_rn(alpha, hv));
    float nx = bv;
    if (f.x_mode == 2) nx = add_rn(nx, mul_rn(alpha_prev, d_old));
    if (f.x_mode != 1) nx = add_rn(nx, mul_rn(alpha, dv));
    if (f.apply_out) nx = mul_rn(f.out_scale, nx);
    acc.rr += (double)nr * nr;
    acc.rp += (double)nr * dv;
    acc.pp += (double)dv * dv;
    av = nr; bv = nx;
  } else {
    const float nv = sub_rn(dv, mul_rn(alpha, hv));
    // x_mode for Neumann: 1 = leave the accumulator p alone this iteration, 2 = catch up: p = (p + v_in) + v' — v_in is
    // last iteration's v' (the direction just read), so these are the very roundings of two separate p += v' updates
    float np = bv;
    if (f.x_mode == 2) np = add_rn(np, dv);
    if (f.x_mode != 1) np = add_rn(np, nv);
    if (f.apply_out) np = mul_rn(f.out_scale, np);
    av = nv; bv = np;
  }
}
template <int MODE>
__device__ __forceinline__ float fuse_alpha(const FuseArgs& f) {
  if (MODE == FUSE_CG && f.alpha_ready == 2) return *f.alpha_lds;
  return (MODE == FUSE_CG && !f.alpha_ready) ? (float)f.scal[S_ALPHA] : f.alpha;
}
// When the step length of a fused epilogue comes from the calling kernel (k_graw: every small-slice block computes it itself),
// the body drives this functor in two phases — begin<MODE>() by every thread BEFORE its own first operand load (the step length's
// loads are requested first: loads return in order and its chain is the longest), finish<MODE>() after the body's loop.
// Default: the value is read from the arguments / the device scalars (requested at begin, so it lands under the loop).
struct AlphaFromArgs {
  float v;
  template <int MODE>
  __device__ __forceinline__ void begin(const FuseArgs& f) { v = (MODE == FUSE_CG && !f.alpha_ready) ? (float)f.scal[S_ALPHA] : f.alpha; }
  template <int MODE>
  __device__ __forceinline__ float finish(const FuseArgs& f) const { return (MODE == FUSE_CG && f.alpha_ready == 2) ? *f.alpha_lds : v; }
};
template <int MODE>
__device__ __forceinline__ float fuse_beta(const FuseArgs& f) {
  return MODE == FUSE_CG && f.lazy ? (float)f.scal[S_BETA] : 0.f;
}
// block-wide sums of the three partials -> part[q][part_base + idx]   (all threads of the 256-thread block call it)
__device__ __forceinline__ void fuse_store_partials(const FuseArgs& f, const FuseAcc& acc, int idx, double* red) {
  double s0 = acc.rr, s1 = acc.rp, s2 = acc.pp;
  block_sum3(s0, s1, s2, red);   // (`red`: 3 * kWaves doubles)
  if (threadIdx.x == 0) {
    double* p0 = f.part + f.part_base + idx;
    p0[0] = s0;
    p0[f.part_stride] = s1;
    p0[2 * (int64_t)f.part_stride] = s2;
  }
}

// ---- weight-shaped outputs: C[M][N] = sum_pairs A_pair^T B_pair (+ addend), K = batch (<= 128) -----------
// The accumulators are transposed through LDS so C (and the addend) move as coalesced 16-B accesses.
constexpr int kOK = 128;                      // max K of the outer-product kernel
constexpr int kOH = kOK / 2;                  // K rows per pipeline stage (half of a pair)
constexpr int kOA = kOH * kTM / (256 * 4);    // float4 per thread for one [64][128] A stage = 8
constexpr int kOB = kOH * kTN / (256 * 4);    // = 4
constexpr int kCPad = kTN + 4;                // LDS row stride of the C staging tile (16-B aligned rows)

// Each operand pair is cut in two K halves => up to 4 pipeline stages; a stage is ONE round of global
// loads (all in flight together) parked in registers while the previous stage's MFMAs run from the
// single 40-KiB LDS tile, so 3-4 workgroups share a CU and cover each other's load/epilogue phases.
// FAST: all tiles interior and 16-B aligned (checked by the launcher): no ragged path, loads unconditional with
// clamped row index and a 0/1 multiplier (same reasons as k_gemm's FAST instance).
// PRE (fused, FAST only): the last stage re-loads nothing; the first half tile's state slices are requested instead, so
// they travel under that stage's MFMAs, and the second half's are requested before the first half is processed.
template <bool FAST, int MODE, bool PRE = false>
__device__ __forceinline__ void outer_body(const GemmArgs& a, const FuseArgs& fz, const int bx, const int by, const int gx) {
  static_assert(!PRE || (FAST && MODE != FUSE_NONE), "PRE is the fused all-interior epilogue");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ double red_rr[3 * kWaves];
  const int K = a.K;
  const int nsp = a.kstages;                          // stages per pair
  const int Kh = (((K + nsp - 1) / nsp) + 1) & ~1;    // rows per stage, even, <= kOH
  float* sA = smem;                       // [Kh][128]
  float* sB = smem + Kh * kTM;            // [Kh][64]
  const int n0 = bx * kTN;
  const int m0 = by * kTM;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 32;
  const int li = lane & 31, lk = lane >> 5;
  const int t = threadIdx.x;

  f32x16 acc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;

  float4 ra[kOA], rb[kOB];
  // stage s: pair s / nsp, K rows [ (s % nsp)*Kh, min(K, (s % nsp)*Kh + Kh) )
  const GemmPair pr0 = a.pr[0];
  const GemmPair pr1 = a.pr[a.pairs > 1 ? 1 : 0];
  auto gload = [&](int stage) {
    const bool second = stage >= nsp;             // workgroup-uniform
    const GemmPair pr = {second ? pr1.A : pr0.A, second ? pr1.B : pr0.B, second ? pr1.lda : pr0.lda,
                         second ? pr1.ldb : pr0.ldb};
    const int kb = (stage - (second ? nsp : 0)) * Kh;
    const bool fa = FAST || (m0 + kTM <= a.M && (pr.lda & 3) == 0);  // workgroup-uniform
    const bool fb = FAST || (n0 + kTN <= a.N && (pr.ldb & 3) == 0);
#pragma unroll
    for (int i = 0; i < kOA; ++i) {   // A stage: 32 float4 per k-row, 8 k-rows per pass
      const int kl = (t >> 5) + 8 * i;
      const int k = kb + kl;
      const int r = m0 + 4 * (t & 31);
      const bool kok = kl < Kh && k < K;
      const int64_t base = (int64_t)(kok ? k : 0) * pr.lda + r;
      if (fa) {
        const float4 v = ld16(pr.A + base);
        const float mz = kok ? 1.f : 0.f;   // multiplier, not a select: hipcc turns the select into a branch around the load
        ra[i] = make_float4(v.x * mz, v.y * mz, v.z * mz, v.w * mz);
      } else {
        ra[i].x = ld_guard(pr.A, base, kok && r < a.M);
        ra[i].y = ld_guard(pr.A, base + 1, kok && r + 1 < a.M);
        ra[i].z = ld_guard(pr.A, base + 2, kok && r + 2 < a.M);
        ra[i].w = ld_guard(pr.A, base + 3, kok && r + 3 < a.M);
      }
    }
#pragma unroll
    for (int i = 0; i < kOB; ++i) {   // B stage: 16 float4 per k-row, 16 k-rows per pass
      const int kl = (t >> 4) + 16 * i;
      const int k = kb + kl;
      const int r = n0 + 4 * (t & 15);
      const bool kok = kl < Kh && k < K;
      const int64_t base = (int64_t)(kok ? k : 0) * pr.ldb + r;
      if (fb) {
        const float4 v = ld16(pr.B + base);
        const float mz = kok ? 1.f : 0.f;
        rb[i] = make_float4(v.x * mz, v.y * mz, v.z * mz, v.w * mz);
      } else {
        rb[i].x = ld_guard(pr.B, base, kok && r < a.N);
        rb[i].y = ld_guard(pr.B, base + 1, kok && r + 1 < a.N);
        rb[i].z = ld_guard(pr.B, base + 2, kok && r + 2 < a.N);
        rb[i].w = ld_guard(pr.B, base + 3, kok && r + 3 < a.N);
      }
    }
  };
  auto lstore = [&]() {
#pragma unroll
    for (int i = 0; i < kOA; ++i) {
      const int k = (t >> 5) + 8 * i;
      if (k < Kh) *reinterpret_cast<float4*>(sA + k * kTM + 4 * (t & 31)) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < kOB; ++i) {
      const int k = (t >> 4) + 16 * i;
      if (k < Kh) *reinterpret_cast<float4*>(sB + k * kTN + 4 * (t & 15)) = rb[i];
    }
  };
  auto compute = [&](int stage) {
    const int kb = (stage >= nsp ? stage - nsp : stage) * Kh;
    const int kvalid = min(Kh, K - kb);           // rows of this stage that carry data (rest is zero)
    const int nkp = kvalid > 0 ? (kvalid + 1) / 2 : 0;
    int kp = 0;
    for (; kp + 4 <= nkp; kp += 4) {  // 12 LDS reads in flight, then 8 MFMAs
      float b[4], a0[4], a1[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = 2 * (kp + u) + lk;
        b[u] = sB[k * kTN + wn + li];
        a0[u] = sA[k * kTM + wm + li];
        a1[u] = sA[k * kTM + wm + 32 + li];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[u], b[u], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[u], b[u], acc[1], 0, 0, 0);
      }
    }
    for (; kp < nkp; ++kp) {
      const int k = 2 * kp + lk;
      const float b = sB[k * kTN + wn + li];
      const float a0 = sA[k * kTM + wm + li];
      const float a1 = sA[k * kTM + wm + 32 + li];
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc[1], 0, 0, 0);
    }
  };

  const int nstages = nsp * a.pairs;
  const bool use_x = fz.x_mode != 1 || MODE == FUSE_NONE;   // workgroup-uniform
  float4 pdv[4], pav[4], pbv[4];                // PRE: state slices of half tile 0
  auto hload = [&](int hb, float4* dv, float4* av, float4* bv) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = (t >> 4) + 16 * (4 * hb + i);
      const int64_t off = (int64_t)(m0 + row) * a.ldo + n0 + 4 * (t & 15);
      dv[i] = ld16(fz.d + off);
      if (MODE == FUSE_CG) av[i] = ld16(fz.a + off);
      bv[i] = use_x ? ld16(fz.b + off) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  gload(0);
  lstore();
  if (PRE) {
    for (int stage = 0; stage + 1 < nstages; ++stage) {
      gload(stage + 1);                         // in flight during this stage's MFMAs
      __syncthreads();                          // this stage's tile is complete in LDS
      compute(stage);
      __syncthreads();                          // everyone is done reading it
      lstore();
    }
    hload(0, pdv, pav, pbv);
    __syncthreads();
    compute(nstages - 1);
  } else {
    for (int stage = 0; stage < nstages; ++stage) {
      gload(min(stage + 1, nstages - 1));       // in flight during this stage's MFMAs (the last one re-loads itself: unused)
      __syncthreads();                          // this stage's tile is complete in LDS
      compute(stage);
      __syncthreads();                          // everyone is done reading it
      lstore();                                 // (after the last stage: a dead store, overwritten by the C staging below)
    }
  }
  __syncthreads();  // LDS is reused as the C staging tile below

  // ---- epilogue: acc -> LDS [128][kCPad] -> coalesced float4 rows (+ addend) -> global
  float* sC = smem;
#pragma unroll
  for (int tt = 0; tt < 2; ++tt)
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) {
      const int row = wm + 32 * tt + (rg & 3) + 8 * (rg >> 2) + 4 * lk;
      sC[row * kCPad + wn + li] = acc[tt][rg];
    }
  __syncthreads();
  const bool vec_ok = ((a.ldo & 3) == 0);
  if (MODE != FUSE_NONE) {
    // fused recurrence: the tile's slices of the state vectors are read/written at the SAME element offsets as C
    // (the weight tensor W_l occupies flat[start_l + row*ldo + col]); two half-tiles of 4 float4 per thread so the
    // 8-12 state loads of a half are all in flight before the first use.
    const float alpha = fuse_alpha<MODE>(fz);
    const float beta = fuse_beta<MODE>(fz);
    const bool wr_d = MODE == FUSE_CG && fz.lazy;
    const float alpha_prev = (MODE == FUSE_CG && fz.x_mode == 2) ? (float)fz.scal[S_ALPHA_RING + (fz.kpar ^ 1)] : 0.f;
    FuseAcc racc{0.0, 0.0, 0.0};
    if constexpr (PRE) {
      float4 dv1[4], av1[4], bv1[4];
      if (MODE != FUSE_CG) hload(1, dv1, av1, bv1);   // (CG: three state vectors — both halves at once do not fit 128 registers)
#pragma unroll
      for (int hb = 0; hb < 2; ++hb) {
        if (MODE == FUSE_CG && hb == 1) hload(1, dv1, av1, bv1);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = (t >> 4) + 16 * (4 * hb + i);
          const int c4 = 4 * (t & 15);
          const float4 hv = *reinterpret_cast<const float4*>(sC + row * kCPad + c4);
          const int64_t off = (int64_t)(m0 + row) * a.ldo + n0 + c4;
          float4 na = MODE == FUSE_CG ? (hb ? av1[i] : pav[i]) : make_float4(0.f, 0.f, 0.f, 0.f);
          float4 nb = hb ? bv1[i] : pbv[i], nd = hb ? dv1[i] : pdv[i];
          fuse_elem<MODE>(fz, alpha, beta, hv.x, nd.x, na.x, nb.x, racc, alpha_prev);
          fuse_elem<MODE>(fz, alpha, beta, hv.y, nd.y, na.y, nb.y, racc, alpha_prev);
          fuse_elem<MODE>(fz, alpha, beta, hv.z, nd.z, na.z, nb.z, racc, alpha_prev);
          fuse_elem<MODE>(fz, alpha, beta, hv.w, nd.w, na.w, nb.w, racc, alpha_prev);
          *reinterpret_cast<float4*>(fz.a + off) = na;
          if (use_x) *reinterpret_cast<float4*>(fz.b + off) = nb;
          if (wr_d) *reinterpret_cast<float4*>(fz.d + off) = nd;
        }
      }
      if (MODE == FUSE_CG) fuse_store_partials(fz, racc, by * gx + bx, red_rr);
      return;
    }
#pragma unroll
    for (int hb = 0; hb < 2; ++hb) {
      float4 dv[4], av[4], bv[4];
      bool ok[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = (t >> 4) + 16 * (4 * hb + i);
        const int c4 = 4 * (t & 15);
        const int grow = m0 + row, gcol = n0 + c4;
        ok[i] = FAST || (grow < a.M && vec_ok && gcol + 4 <= a.N);
        const int64_t off = ok[i] ? (int64_t)grow * a.ldo + gcol : 0;
        dv[i] = ld16(fz.d + off);
        if (MODE == FUSE_CG) av[i] = ld16(fz.a + off);
        bv[i] = use_x ? ld16(fz.b + off) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = (t >> 4) + 16 * (4 * hb + i);
        const int c4 = 4 * (t & 15);
        const int grow = m0 + row, gcol = n0 + c4;
        const float4 hv = *reinterpret_cast<const float4*>(sC + row * kCPad + c4);
        const int64_t off = (int64_t)grow * a.ldo + gcol;
        if (ok[i]) {
          float4 na = MODE == FUSE_CG ? av[i] : make_float4(0.f, 0.f, 0.f, 0.f), nb = bv[i], nd = dv[i];
          fuse_elem<MODE>(fz, alpha, beta, hv.x, nd.x, na.x, nb.x, racc, alpha_prev);
          fuse_elem<MODE>(fz, alpha, beta, hv.y, nd.y, na.y, nb.y, racc, alpha_prev);
          fuse_elem<MODE>(fz, alpha, beta, hv.z, nd.z, na.z, nb.z, racc, alpha_prev);
          fuse_elem<MODE>(fz, alpha, beta, hv.w, nd.w, na.w, nb.w, racc, alpha_prev);
          *reinterpret_cast<float4*>(fz.a + off) = na;
          if (use_x) *reinterpret_cast<float4*>(fz.b + off) = nb;
          if (wr_d) *reinterpret_cast<float4*>(fz.d + off) = nd;
        } else if (!FAST && grow < a.M) {   // ragged right edge / odd leading dimension: element by element
          const float hh[4] = {hv.x, hv.y, hv.z, hv.w};
          for (int j = 0; j < 4 && gcol + j < a.N; ++j) {
            float na = MODE == FUSE_CG ? fz.a[off + j] : 0.f, nb = use_x ? fz.b[off + j] : 0.f, nd = fz.d[off + j];
            fuse_elem<MODE>(fz, alpha, beta, hh[j], nd, na, nb, racc, alpha_prev);
            fz.a[off + j] = na;
            if (use_x) fz.b[off + j] = nb;
            if (wr_d) fz.d[off + j] = nd;
          }
        }
      }
    }
    if (MODE == FUSE_CG) fuse_store_partials(fz, racc, by * gx + bx, red_rr);
    return;
  }
#pragma unroll
  for (int i = 0; i < kTM * kTN / (256 * 4); ++i) {  // 8 float4 per thread
    const int row = (t >> 4) + 16 * i;
    const int c4 = 4 * (t & 15);
    const int grow = m0 + row, gcol = n0 + c4;
    if (!FAST && (grow >= a.M || gcol >= a.N)) continue;
    float4 v = *reinterpret_cast<const float4*>(sC + row * kCPad + c4);
    float* dst = a.out + (int64_t)grow * a.ldo + gcol;
    if (FAST || (vec_ok && gcol + 4 <= a.N)) {
      if (a.addend) {
        const float4 ad = *reinterpret_cast<const float4*>(a.addend + (int64_t)grow * a.ldo + gcol);
        v.x += a.addend_scale * ad.x; v.y += a.addend_scale * ad.y;
        v.z += a.addend_scale * ad.z; v.w += a.addend_scale * ad.w;
      }
      *reinterpret_cast<float4*>(dst) = v;
    } else {
      const float vv[4] = {v.x, v.y, v.z, v.w};
      for (int j = 0; j < 4 && gcol + j < a.N; ++j) {
        float o = vv[j];
        if (a.addend) o += a.addend_scale * a.addend[(int64_t)grow * a.ldo + gcol + j];
        dst[j] = o;
      }
    }
  }
}

template <bool FAST, int MODE>
__global__ __launch_bounds__(256) void k_outer(GemmArgs a, FuseArgs fz) {
  outer_body<FAST, MODE>(a, fz, blockIdx.x, blockIdx.y, gridDim.x);
}

// ---- split-K epilogues ---------------------------------------------------------------------------------
// out[m][n] = mask[m][n] * (sum_s part[s][m][n] + bias[n]);  rows >= B are written as zero.
// One float4 per thread when N % 4 == 0 (all split loads independent => in flight together);
// fixed summation order over splits => deterministic.
template <int VEC>
__global__ __launch_bounds__(256) void k_reduce_mask(const float* __restrict__ part, int splits, int slab,
                                                     const float* __restrict__ bias, const float* __restrict__ mask,
                                                     float* __restrict__ out, int rows, int N, int B,
                                                     float* __restrict__ relu_mask_out, float* __restrict__ outp = nullptr) {
  // relu_mask_out != NULL: forward-pass mode — out = relu(sum + bias), relu_mask_out = (sum + bias > 0)
  // outp != NULL (VEC == 4): a packed copy of out, [N / 16][rows][16] (wskp.inc), for the product that consumes it
  const int64_t total = (int64_t)rows * N / VEC;
  const int nv = N / VEC;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int m = (int)(i / nv), n = (int)(i - (int64_t)m * nv) * VEC;
    float v[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) v[j] = 0.f;
    if (m < B) {
      if constexpr (VEC == 4) {
        // Batches of 8 slabs: all 8 loads (plus bias and mask) are issued before the first add, so a
        // reduce costs one or two L2 round trips instead of `splits` dependent ones.  Lanes past the
        // last slab re-read it (an L1 hit) and are not added; the summation order stays s = 0, 1, ...
        constexpr int NB = 8;    // (measured: 16 in flight — one round trip for the benchmark's 12-16 slabs — is SLOWER, 5.5-6.1 vs 4.9 us)
        const float* p0 = part + i * VEC;
        float4 bv = make_float4(0.f, 0.f, 0.f, 0.f), mv = make_float4(1.f, 1.f, 1.f, 1.f);
        if (bias) bv = *reinterpret_cast<const float4*>(bias + n);
        if (mask) mv = *reinterpret_cast<const float4*>(mask + i * VEC);
        for (int s0 = 0; s0 < splits; s0 += NB) {
          float4 t[NB];
#pragma unroll
          for (int u = 0; u < NB; ++u) {
            const int s = s0 + u < splits ? s0 + u : splits - 1;
            t[u] = *reinterpret_cast<const float4*>(p0 + (int64_t)s * slab);
          }
#pragma unroll
          for (int u = 0; u < NB; ++u) {
            if (s0 + u < splits) { v[0] += t[u].x; v[1] += t[u].y; v[2] += t[u].z; v[3] += t[u].w; }
          }
        }
        v[0] = (v[0] + bv.x) * mv.x; v[1] = (v[1] + bv.y) * mv.y;
        v[2] = (v[2] + bv.z) * mv.z; v[3] = (v[3] + bv.w) * mv.w;
      } else {
        for (int s = 0; s < splits; ++s) v[0] += part[(int64_t)s * slab + i];
        if (bias) v[0] += bias[n];
        if (mask) v[0] *= mask[i];
      }
    }
    if (relu_mask_out) {
      float mk[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        mk[j] = v[j] > 0.f ? 1.f : 0.f;
        v[j] = v[j] > 0.f ? v[j] : 0.f;
      }
      if constexpr (VEC == 4) *reinterpret_cast<float4*>(relu_mask_out + i * VEC) = make_float4(mk[0], mk[1], mk[2], mk[3]);
      else relu_mask_out[i] = mk[0];
    }
    if constexpr (VEC == 4) {
      *reinterpret_cast<float4*>(out + i * VEC) = make_float4(v[0], v[1], v[2], v[3]);
      if (outp) *reinterpret_cast<float4*>(outp + ((int64_t)(n >> 4) * rows + m) * 16 + (n & 15)) = make_float4(v[0], v[1], v[2], v[3]);
    } else out[i] = v[0];
  }
}
