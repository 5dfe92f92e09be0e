// bhg_logreg_solve.hip — the whole CG / Neumann solve of L2-regularised logistic regression in native launches.
//
// Same inner problem and product as bhg_logreg.hip:  H p = X^T( s .* (X p) ) + lam .* p,  s_i = sigma_i (1 - sigma_i) / n, sigma_i
// from x_i . w.  What changes is who runs the K loop (cg.py:38-56, neumann.py:59-66 of the reference): not the host with K x
// (three product launches + a recurrence kernel sized for 10 M-element vectors), but
//   single : ONE launch of ONE workgroup — w, lam and the state (x, r, p | v, p) in LDS, X re-read from cache per iteration;
//   strips : G workgroups own contiguous row strips and write a [G][d] partial; small follow-up launches sum the partials in strip
//            order, add lam .* p and apply the recurrences (3 launches per CG iteration, 2 per Neumann iteration, none around them).
// Both forms use ONE device body for the pass over X (pass_rows): a wave takes a row into registers, forms z_p = x_i . p and
// z_w = x_i . w against the LDS copies of the direction and the weights, scales u_i = s_i(z_w) z_p and adds u_i x_i into per-lane
// column accumulators while the row is still in registers — X is read once per product and s is never stored.  The waves' accumulators
// meet in LDS in wave order, the strips' partials in strip order, the dots in fp64 in a fixed order: results are bitwise run-to-run
// deterministic; no float atomics, no workgroup waits on another inside a launch, every loop is bounded by its arguments, and
// nothing is read from the workspace that the same solve has not written.
//
// Arithmetic of the recurrences: oracle/recurrence.c / tests/recurrence_ref.py (products rounded to fp32 before add / sub, fp64 dots,
// fp32 quotients, den = dot(fl(cg_alpha Hp), p) but r -= alpha Hp with the un-scaled Hp, no breakdown guard, out_scale folded
// into the last iteration).
#include "bhg_linear_solve.hpp"

namespace bhg {
namespace {

constexpr int kSingleMaxD = 1024;
constexpr int64_t kSingleMaxElems = (int64_t)1 << 18;
constexpr int kStripsMaxD = 4096;
constexpr int kRowsPerStrip = 16;     // auto: G = ceil(n / 16), capped at kMaxStrips
constexpr int kMaxColBlocks = kStripsMaxD / kColBlock;
constexpr size_t kWsVec = 1024;       // byte offset of the vectors of the workspace (strips_ws), past the den partials
static_assert(kWsDen + 8 * kMaxColBlocks <= kWsVec, "the den partials end before the vectors of the workspace");

// ---- the pass over X -------------------------------------------------------------------------------------------------
// A lane holds NR elements of a row: 16-byte path, element e = float (e & 3) of the float4 at column (e / 4) * 256 + lane * 4;
// scalar path (d % 4 != 0: row starts are unaligned), column e * 64 + lane.  Either way NR registers cover 64 * NR columns.
template <int NR, bool VEC>
__device__ __forceinline__ void load_row(const float* __restrict__ row, const int d, const int lane, float (&x)[NR]) {
  if constexpr (VEC) {
#pragma unroll
    for (int g = 0; g < NR / 4; ++g) {
      const int c = g * 256 + lane * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < d) v = *reinterpret_cast<const float4*>(row + c);   // d % 4 == 0: c + 3 < d
      x[4 * g] = v.x; x[4 * g + 1] = v.y; x[4 * g + 2] = v.z; x[4 * g + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int e = 0; e < NR; ++e) {
      const int c = e * 64 + lane;
      x[e] = c < d ? row[c] : 0.f;
    }
  }
}

// acc[e] = sum over the rows {row0 + wave, row0 + wave + nwaves, ...} < row1 of s_i (x_i . p) x_i[column of e], R rows in flight.
// sp / sw: direction and weights in LDS, ZERO from d up to 64 * NR.  nf = (float)n of the WHOLE problem.
template <int NR, bool VEC, int R>
__device__ __forceinline__ void pass_rows(const float* __restrict__ X, const int d, const int row0, const int row1, const int wave,
                                          const int nwaves, const int lane, const float nf, const float* sp, const float* sw,
                                          float (&acc)[NR]) {
#pragma unroll
  for (int e = 0; e < NR; ++e) acc[e] = 0.f;
  for (int base = row0 + wave; base < row1; base += R * nwaves) {
    // (the direction and the weights are re-read from LDS per batch: hoisted out of this loop they would double the registers)
    asm volatile("" ::: "memory");
    float x[R][NR];
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int i = base + q * nwaves;
      if (i < row1) {
        load_row<NR, VEC>(X + (int64_t)i * d, d, lane, x[q]);
      } else {
#pragma unroll
        for (int e = 0; e < NR; ++e) x[q][e] = 0.f;
      }
    }
    float zp[R], zw[R];
#pragma unroll
    for (int q = 0; q < R; ++q) zp[q] = zw[q] = 0.f;
    if constexpr (VEC) {
#pragma unroll
      for (int g = 0; g < NR / 4; ++g) {
        const int c = g * 256 + lane * 4;
        const float4 pv = *reinterpret_cast<const float4*>(sp + c), wv = *reinterpret_cast<const float4*>(sw + c);
#pragma unroll
        for (int q = 0; q < R; ++q) {
          zp[q] = fmaf(x[q][4 * g + 3], pv.w, fmaf(x[q][4 * g + 2], pv.z, fmaf(x[q][4 * g + 1], pv.y, fmaf(x[q][4 * g], pv.x, zp[q]))));
          zw[q] = fmaf(x[q][4 * g + 3], wv.w, fmaf(x[q][4 * g + 2], wv.z, fmaf(x[q][4 * g + 1], wv.y, fmaf(x[q][4 * g], wv.x, zw[q]))));
        }
      }
    } else {
#pragma unroll
      for (int e = 0; e < NR; ++e) {
        const float pv = sp[e * 64 + lane], wv = sw[e * 64 + lane];
#pragma unroll
        for (int q = 0; q < R; ++q) {
          zp[q] = fmaf(x[q][e], pv, zp[q]);
          zw[q] = fmaf(x[q][e], wv, zw[q]);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const float sg = 1.f / (1.f + __expf(-wave_sum_f32(zw[q])));
      const float u = (sg * (1.f - sg) / nf) * wave_sum_f32(zp[q]);   // (a row past row1 is all zeros: it adds 0 * u)
#pragma unroll
      for (int e = 0; e < NR; ++e) acc[e] = fmaf(x[q][e], u, acc[e]);
    }
  }
}

// red[c] = ((acc_wave0 + acc_wave1) + acc_wave2) + ...  for the 64 * NR columns; red is valid for every thread on return.
template <int NR, bool VEC, int W>
__device__ __forceinline__ void combine_waves(float* red, const float (&acc)[NR], const int wave, const int lane) {
#pragma unroll 1
  for (int wv = 0; wv < W; ++wv) {
    if (wave == wv) {
      if constexpr (VEC) {
#pragma unroll
        for (int g = 0; g < NR / 4; ++g) {
          float4* q = reinterpret_cast<float4*>(red + g * 256 + lane * 4);
          float4 v = make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
          if (wv > 0) {
            const float4 o = *q;
            v.x = o.x + v.x; v.y = o.y + v.y; v.z = o.z + v.z; v.w = o.w + v.w;
          }
          *q = v;
        }
      } else {
#pragma unroll
        for (int e = 0; e < NR; ++e) {
          const int c = e * 64 + lane;
          red[c] = wv > 0 ? red[c] + acc[e] : acc[e];
        }
      }
    }
    __syncthreads();
  }
}

constexpr int rows_in_flight(int NR) { return NR <= 4 ? 8 : NR <= 16 ? 4 : 1; }   // (a row of the widest instance is 64 registers)

// ---- single: the whole solve in one workgroup ---------------------------------------------------------------------------------
// CG: sx = x, sr = r, sp = p.  Neumann: sp = v (the direction), sx = the accumulator p.  `a`: cg_alpha | alpha.
template <int NR, bool VEC, int T, bool CG>
__global__ __launch_bounds__(T) void k_logreg_single(const float* __restrict__ X, const float* __restrict__ w,
                                                     const float* __restrict__ lam, const float* __restrict__ rhs,
                                                     float* __restrict__ out, float* __restrict__ coeff, const int n, const int d,
                                                     const int K, const float a, const float out_scale) {
  constexpr int DMAX = 64 * NR, W = T / 64;
  __shared__ __align__(16) float sw[DMAX], sp[DMAX], sh[DMAX];
  __shared__ float slam[DMAX], sx[DMAX], sr[DMAX];
  __shared__ double sred[W];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int j = tid; j < DMAX; j += T) {
    const bool in = j < d;
    const float rv = in ? rhs[j] : 0.f;
    sw[j] = in ? w[j] : 0.f;
    slam[j] = in ? lam[j] : 0.f;
    sp[j] = rv;
    sr[j] = rv;
    sx[j] = CG ? 0.f : rv;
  }
  __syncthreads();
  double rr = 0.0;
  if constexpr (CG) {
    for (int j = tid; j < d; j += T) rr += (double)sr[j] * (double)sr[j];
    rr = block_sum_w<W>(rr, sred);
  }
  const float nf = (float)n;
  for (int k = 0; k < K; ++k) {
    float acc[NR];
    pass_rows<NR, VEC, rows_in_flight(NR)>(X, d, 0, n, wave, W, lane, nf, sp, sw, acc);
    combine_waves<NR, VEC, W>(sh, acc, wave, lane);
    // from here every thread touches its own columns {tid, tid + T, ...} only
    if constexpr (CG) {
      double den = 0.0;
      for (int j = tid; j < d; j += T) {
        const float lp = slam[j] * sp[j];
        const float hp = sh[j] + lp;
        sh[j] = hp;
        const float ahp = a * hp;
        den += (double)ahp * (double)sp[j];
      }
      den = block_sum_w<W>(den, sred);
      const float alpha = (float)rr / (float)den;
      double rn2 = 0.0;
      for (int j = tid; j < d; j += T) {
        const float t = alpha * sh[j];
        const float rn = sr[j] - t;
        sr[j] = rn;
        rn2 += (double)rn * (double)rn;
      }
      rn2 = block_sum_w<W>(rn2, sred);
      const float beta = (float)rn2 / (float)rr;
      for (int j = tid; j < d; j += T) {
        const float ap = alpha * sp[j];
        sx[j] = sx[j] + ap;
        const float bp = beta * sp[j];
        sp[j] = sr[j] + bp;
      }
      rr = rn2;
    } else {
      for (int j = tid; j < d; j += T) {
        const float lp = slam[j] * sp[j];
        const float hv = sh[j] + lp;
        const float t = a * hv;
        const float vn = sp[j] - t;
        sp[j] = vn;
        sx[j] = vn + sx[j];
      }
    }
    __syncthreads();
  }
  for (int j = tid; j < d; j += T) {
    float o = sx[j];
    if (out_scale != 0.f) o = out_scale * o;
    out[j] = o;
    if (coeff) coeff[j] = sw[j] * o;
  }
}

// ---- strips ----------------------------------------------------------------------------------------------------------------------
// Launch 1 of an iteration: workgroup g sums its rows [g rps, (g + 1) rps) into part[g][0..d); an empty strip writes zeros.
template <int NR, bool VEC>
__global__ __launch_bounds__(kThreads) void k_logreg_strip_pass(const float* __restrict__ X, const float* __restrict__ w,
                                                                const float* __restrict__ dir, float* __restrict__ part,
                                                                const int n, const int d, const int rps) {
  constexpr int DMAX = 64 * NR;
  __shared__ __align__(16) float sw[DMAX], sp[DMAX], sh[DMAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int j = tid; j < DMAX; j += kThreads) {
    const bool in = j < d;
    sw[j] = in ? w[j] : 0.f;
    sp[j] = in ? dir[j] : 0.f;
  }
  __syncthreads();
  const int64_t lo = (int64_t)blockIdx.x * rps, hi = lo + rps;
  const int row0 = (int)(lo < n ? lo : n), row1 = (int)(hi < n ? hi : n);
  float acc[NR];
  pass_rows<NR, VEC, rows_in_flight(NR)>(X, d, row0, row1, wave, kWaves, lane, (float)n, sp, sw, acc);
  combine_waves<NR, VEC, kWaves>(sh, acc, wave, lane);
  float* dst = part + (int64_t)blockIdx.x * d;
  if constexpr (VEC) {
    for (int j = tid * 4; j < d; j += kThreads * 4) *reinterpret_cast<float4*>(dst + j) = *reinterpret_cast<const float4*>(sh + j);
  } else {
    for (int j = tid; j < d; j += kThreads) dst[j] = sh[j];
  }
}

// The launches after the pass: thin wrappers of the shared bodies (bhg_linear_solve.hpp), N = d.  The CG update adds the den partials
// serially in workgroup order in every thread.
__global__ __launch_bounds__(kColBlock) void k_logreg_strip_hp(const float* __restrict__ part, const int G,
                                                               const float* __restrict__ lam, const float* __restrict__ p,
                                                               float* __restrict__ Hp, double* __restrict__ denpart, const int d,
                                                               const float cg_alpha) {
  strip_hp_body(part, G, lam, p, Hp, denpart, d, cg_alpha);
}

__global__ __launch_bounds__(kThreads) void k_logreg_strip_cg_update(const float* __restrict__ rhs, const float* __restrict__ w,
                                                                     const float* __restrict__ Hp, const double* __restrict__ denpart,
                                                                     const int nden, double* __restrict__ rr_slot, float* __restrict__ x,
                                                                     float* __restrict__ r, float* __restrict__ p, float* __restrict__ out,
                                                                     float* __restrict__ coeff, const int d, const int k, const int last,
                                                                     const float out_scale) {
  strip_cg_update_body<kThreads, true>(rhs, w, Hp, denpart, nden, rr_slot, x, r, p, out, coeff, d, k, last, out_scale);
}

__global__ __launch_bounds__(kColBlock) void k_logreg_strip_neumann_update(const float* __restrict__ part, const int G,
                                                                           const float* __restrict__ lam, const float* __restrict__ w,
                                                                           const float* vin, const float* pin, float* v, float* p,
                                                                           float* __restrict__ out, float* __restrict__ coeff, const int d,
                                                                           const float alpha, const int last, const float out_scale) {
  strip_neumann_update_body(part, G, lam, w, vin, pin, v, p, out, coeff, d, alpha, last, out_scale);
}

__global__ __launch_bounds__(kThreads) void k_logreg_solve_k0(const float* __restrict__ rhs, const float* __restrict__ w,
                                                              float* __restrict__ out, float* __restrict__ coeff, const int d,
                                                              const int cg, const float out_scale) {
  solve_k0_body(rhs, w, out, coeff, d, cg, out_scale);
}

const StripKernels kStripKernels = {k_logreg_strip_hp, k_logreg_strip_cg_update, kThreads, k_logreg_strip_neumann_update};

// ---- host ------------------------------------------------------------------------------------------------------------------------
bool single_admits(int n, int d) { return d <= kSingleMaxD && (int64_t)n * d <= kSingleMaxElems; }
bool strips_admits(int /*n*/, int d) { return d <= kStripsMaxD; }

// BHG_OK and the plan, or BHG_ERR_ARG with the error set (a forced form the shape does not admit is an error, not a fallback)
int make_plan(const char* fn, int n, int d, int form, int strips, Plan* out) {
  int f;
  const int rc = plan_form(fn, n <= 0 || d <= 0, n, form, strips, single_admits(n, d), strips_admits(n, d), &f);
  if (rc != BHG_OK) return rc;
  if (f == kFormSingle && !single_admits(n, d)) {
    set_error("%s: the single form takes d <= %d and n * d <= %lld", fn, kSingleMaxD, (long long)kSingleMaxElems);
    return BHG_ERR_ARG;
  }
  if (f == kFormStrips && !strips_admits(n, d)) { set_error("%s: the strips form takes d <= %d", fn, kStripsMaxD); return BHG_ERR_ARG; }
  const int64_t want = ((int64_t)n + kRowsPerStrip - 1) / kRowsPerStrip;   // auto
  *out = plan_of(f, n, strips, (int)(want < kMaxStrips ? want : kMaxStrips));
  return BHG_OK;
}

template <bool CG>
int launch_single(hipStream_t st, const float* X, const float* w, const float* lam, const float* rhs, float* out, float* coeff, int n,
                  int d, int K, float a, float out_scale, bool vec) {
#define BHG_LR_SINGLE(NR, VEC, T)                                                                                             \
  hipLaunchKernelGGL((k_logreg_single<NR, VEC, T, CG>), dim3(1), dim3(T), 0, st, X, w, lam, rhs, out, coeff, n, d, K, a, out_scale)
  if (d <= 256) {
    if (vec) BHG_LR_SINGLE(4, true, 1024); else BHG_LR_SINGLE(4, false, 1024);
  } else {
    if (vec) BHG_LR_SINGLE(16, true, 512); else BHG_LR_SINGLE(16, false, 512);
  }
#undef BHG_LR_SINGLE
  return BHG_OK;
}

void launch_pass(hipStream_t st, const Plan& pl, const float* X, const float* w, const float* dir, float* part, int n, int d, bool vec) {
#define BHG_LR_PASS(NR, VEC) \
  hipLaunchKernelGGL((k_logreg_strip_pass<NR, VEC>), dim3(pl.G), dim3(kThreads), 0, st, X, w, dir, part, n, d, pl.rps)
  if (d <= 256) {
    if (vec) BHG_LR_PASS(4, true); else BHG_LR_PASS(4, false);
  } else if (d <= 1024) {
    if (vec) BHG_LR_PASS(16, true); else BHG_LR_PASS(16, false);
  } else {
    if (vec) BHG_LR_PASS(64, true); else BHG_LR_PASS(64, false);
  }
#undef BHG_LR_PASS
}

template <bool CG>
int solve(const char* fn, const float* X, const float* w, const float* lam, const float* rhs, float* out, float* coeff, void* ws, int n,
          int d, int K, float a, float out_scale, int form, int strips, void* stream) {
  if (!(X && w && lam && rhs && out && ws)) { set_error("%s: NULL pointer", fn); return BHG_ERR_ARG; }
  if (K < 0) { set_error("%s: negative iteration count", fn); return BHG_ERR_ARG; }
  Plan pl;
  const int rc = make_plan(fn, n, d, form, strips, &pl);
  if (rc != BHG_OK) return rc;
  if (pl.form == kFormNone) { set_error("%s: no native form takes d = %d (d <= %d)", fn, d, kStripsMaxD); return BHG_ERR_ARG; }
  if (((uintptr_t)ws & 15) != 0) { set_error("%s: the workspace must be 16-byte aligned", fn); return BHG_ERR_ARG; }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (K == 0) {
    hipLaunchKernelGGL(k_logreg_solve_k0, dim3((d + kThreads - 1) / kThreads), dim3(kThreads), 0, st, rhs, w, out, coeff, d, CG ? 1 : 0,
                       out_scale);
    BHG_HIP_CHECK(hipGetLastError());
    return BHG_OK;
  }
  const bool vec = d % 4 == 0 && ((uintptr_t)X & 15) == 0;   // else row starts are unaligned: the scalar path
  if (pl.form == kFormSingle) {
    launch_single<CG>(st, X, w, lam, rhs, out, coeff, n, d, K, a, out_scale, vec);
    BHG_HIP_CHECK(hipGetLastError());
    return BHG_OK;
  }
  run_strips<CG>(st, kStripKernels, strips_ws(ws, kWsVec, d), pl.G,
                 [&](const float* dir, float* part) { launch_pass(st, pl, X, w, dir, part, n, d, vec); }, lam, w, rhs, out, coeff, d, K, a,
                 out_scale);
  BHG_HIP_CHECK(hipGetLastError());
  return BHG_OK;
}

}  // namespace
}  // namespace bhg

using namespace bhg;

extern "C" {

int bhg_logreg_solve_plan(int n, int d, int form, int strips, char* buf, size_t buf_bytes) {
  BHG_REQUIRE(buf && buf_bytes > 0, "NULL buffer");
  Plan pl;
  const int rc = make_plan(__func__, n, d, form, strips, &pl);
  if (rc != BHG_OK) return rc;
  plan_line(pl, buf, buf_bytes);
  return BHG_OK;
}

size_t bhg_logreg_solve_ws_bytes(int n, int d) {
  if (n <= 0 || d <= 0 || d > kStripsMaxD) return 0;
  return strips_ws(nullptr, kWsVec, d).bytes;
}

int bhg_logreg_cg_solve(const float* X, const float* w, const float* lam, const float* rhs, float* out, float* coeff, void* ws, int n,
                        int d, int K, float cg_alpha, float out_scale, int form, int strips, void* stream) {
  return solve<true>(__func__, X, w, lam, rhs, out, coeff, ws, n, d, K, cg_alpha, out_scale, form, strips, stream);
}

int bhg_logreg_neumann_solve(const float* X, const float* w, const float* lam, const float* rhs, float* out, float* coeff, void* ws, int n,
                             int d, int K, float alpha, float out_scale, int form, int strips, void* stream) {
  return solve<false>(__func__, X, w, lam, rhs, out, coeff, ws, n, d, K, alpha, out_scale, form, strips, stream);
}

}  // extern "C"
