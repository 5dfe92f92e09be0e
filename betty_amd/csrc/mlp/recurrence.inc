// Fragment of bhg_mlp.hip — #included there INSIDE `namespace bhg { namespace {`, in this order: gemm, outer, scalars, head, wsk,
// (host: launch helpers), recurrence, proj.  Not a header of its own.
// Here: mixed coefficient from Rz(x), direction update kernels (k_cg_pdir, k_cg_beta).

// coeff[b] = scale * (prob_b - onehot(y_b)) . RzX_b / B   (mixed-derivative coefficient from the accumulated Rz(x))
//   add_scale != 0: coeff[b] = that + add_scale * coeff[b]  (the accumulator-free Neumann solve: the last direction's share
//   is already in coeff);  rzx == NULL counts as zero.
__global__ __launch_bounds__(kThreads) void k_coeff_from_rzx(const double* __restrict__ rzx, const float* __restrict__ prob,
                                                             const int64_t* __restrict__ labels, float* __restrict__ coeff,
                                                             int rows, int C, int B, float scale, float add_scale) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= rows) return;
  float out = 0.f;
  if (b < B) {
    const int y = (int)labels[b];
    double acc = 0.0;
    if (rzx)
      for (int c = 0; c < C; ++c) acc += ((double)prob[(int64_t)b * C + c] - (c == y ? 1.0 : 0.0)) * rzx[(int64_t)b * C + c];
    double o = (double)scale * acc / (double)B;
    if (add_scale != 0.f) o += (double)add_scale * (double)coeff[b];
    out = (float)o;
  }
  coeff[b] = out;
}

#ifdef BHG_AB   // (round 6: the eager direction update is an arm of the measurement build only — key cg_eager_p; the product is always lazy)
// cg.py:52-53 after the fused outputs: beta = r'.r' / r.r ; p <- r' + beta * p ; partial p'.p' (next iteration's
// shift term).  12*N bytes (read r', p; write p).  x and r were already updated by the fused epilogues.
__global__ __launch_bounds__(kThreads) void k_cg_pdir(const bhg_chunk* __restrict__ chunks, int n_chunks,
                                                      const float* __restrict__ r, float* __restrict__ p,
                                                      const double* __restrict__ partRR_new, int nRR,
                                                      double* __restrict__ partPP, double* __restrict__ scal) {
  __shared__ double red[kWaves];
  const double rr_new = sum_partials(partRR_new, nRR, red);
  const double rr_old = scal[S_RR_OLD];
  const float beta = (float)rr_new / (float)rr_old;
  double acc = 0.0;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const bhg_chunk ck = chunks[c];
    float4 a[kVecPerThread], q[kVecPerThread];
#pragma unroll
    for (int i = 0; i < kVecPerThread; ++i) {
      const int e = 4 * (threadIdx.x + kThreads * i);
      a[i] = ld4(r + ck.flat_off, e, ck.len);
      q[i] = ld4(p + ck.flat_off, e, ck.len);
    }
#pragma unroll
    for (int i = 0; i < kVecPerThread; ++i) {
      const int e = 4 * (threadIdx.x + kThreads * i);
      float4 np;
      np.x = add_rn(a[i].x, mul_rn(beta, q[i].x)); np.y = add_rn(a[i].y, mul_rn(beta, q[i].y));
      np.z = add_rn(a[i].z, mul_rn(beta, q[i].z)); np.w = add_rn(a[i].w, mul_rn(beta, q[i].w));
      st4(p + ck.flat_off, e, ck.len, np);
      acc += (double)np.x * np.x + (double)np.y * np.y + (double)np.z * np.z + (double)np.w * np.w;
    }
  }
  const double s = block_sum(acc, red);
  if (threadIdx.x == 0) {
    partPP[blockIdx.x] = s;
    if (blockIdx.x == 0) {
      scal[S_RR_NEW] = rr_new;
      scal[S_BETA] = (double)beta;
    }
  }
}
#endif

// Lazy direction (default of the fused CG solver): instead of k_cg_pdir's 12*N-byte pass, the coming iteration forms
// p = r' + beta * p_old wherever it reads the direction (k_gemm<BF> loaders, the fused output epilogue, which also
// writes it back).  This kernel is what remains of cg.py:51-53 between two iterations:
//   rr' = sum partials, beta = rr' / rr (fp32 division of fp32-rounded dots, as the reference), and
//   p.p of the coming direction = rr' + 2 beta r'.p_old + beta^2 p_old.p_old  (only used for the shift * p.p term of
//   the step length; in exact CG r'.p_old = 0, so this is a sum of positives),
// plus the direction update of the SMALL slices (biases, narrow head weights), which the head / reduce kernels read
// directly.  A few blocks; every block recomputes the same scalars from the same partials in the same order.
struct BetaArgs {
  const double* part; int n, stride;     // [3][stride] partials of the previous iteration's epilogues (rr', r'.p, p.p)
  double* scal;
  const float* r; float* p;
  int64_t off[BHG_MLP_MAX_LAYERS + 1]; int len[BHG_MLP_MAX_LAYERS + 1]; int nt;   // small slices (flat element offsets)
};
__device__ __forceinline__ void beta_body(const BetaArgs& a, const int bx) {
  __shared__ double red[3][kWaves];
  __shared__ float s_beta;
  // this thread's element of the small slices: its loads are issued BEFORE the partial sums are reduced (independent)
  const int gi = bx * kThreads + threadIdx.x;
  int64_t eoff = -1;
  {
    int base = 0;
    for (int t = 0; t < a.nt; ++t) {
      if (eoff < 0 && gi < base + a.len[t]) eoff = a.off[t] + (gi - base);
      base += a.len[t];
    }
  }
  float rv = 0.f, pv = 0.f;
  if (eoff >= 0) { rv = a.r[eoff]; pv = a.p[eoff]; }
  double acc[3] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < a.n; i += kThreads) {
    acc[0] += a.part[i];
    acc[1] += a.part[a.stride + i];
    acc[2] += a.part[2 * (int64_t)a.stride + i];
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const double v = wave_sum(acc[q]);
    if (lane == 0) red[q][w] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      double t = 0.0;
#pragma unroll
      for (int i = 0; i < kWaves; ++i) t += red[q][i];
      tot[q] = t;
    }
    const double rr_old = a.scal[S_RR_OLD];
    const float beta = (float)tot[0] / (float)rr_old;
    s_beta = beta;
    if (bx == 0) {
      a.scal[S_RR_NEW] = tot[0];
      a.scal[S_BETA] = (double)beta;
      a.scal[S_PP] = tot[0] + 2.0 * (double)beta * tot[1] + (double)beta * (double)beta * tot[2];
    }
  }
  __syncthreads();
  if (eoff >= 0) a.p[eoff] = add_rn(rv, mul_rn(s_beta, pv));
}
__global__ __launch_bounds__(kThreads) void k_cg_beta(BetaArgs a) { beta_body(a, blockIdx.x); }
