// bhg_linear_solve.hpp — what the whole-solve files of the linear inner problems (bhg_logreg_solve.hip, bhg_softreg_solve.hip) share:
// everything of the strips form after "the pass over X", over a flat vector of N elements (N = d | C d).
//
//   device : the fixed-order sums (block_sum_w, strip_sum) and the BODIES of the four post-pass kernels.  The __global__ symbols stay
//            in each file, a few lines around these bodies (and it is their parameters that carry the __restrict__), so that profiles
//            keep the two problems' kernels apart;
//   host   : the plan (form, G, rows per strip) up to each file's admits predicates, auto strip count and error texts, the plan line,
//            the workspace layout  [0] rr (fp64) | [64] den partials (fp64) | [vec_off] Hp, x, r, p (CG) or -, -, v, p (Neumann):
//            4 x pad4(N) floats | partials [G][N],  and the K loop of the strips form (run_strips).
//
// The one fork of the device code: the order in which the CG update adds the den partials (DEN_SERIAL).  Either order is part of
// the result bits of the solver that uses it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "bhg_common.hpp"

namespace bhg {

constexpr int kMaxStrips = 512;               // 2 workgroups of the widest pass per CU x 256 CUs
constexpr int kColBlock = 64;                 // elements per workgroup (one wave) of the partial-summing launches
constexpr size_t kWsRr = 0, kWsDen = 64;

// ---- device ----------------------------------------------------------------------------------------------------------------------
template <int W>
__device__ __forceinline__ double block_sum_w(double v, double* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();  // protect `red` against the previous use
  if (lane == 0) red[w] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < W; ++i) s += red[i];
  return s;
}

// sum over the strips, in strip order, of flat element j (eight loads in flight)
__device__ __forceinline__ double strip_sum(const float* __restrict__ part, const int G, const int N, const int j) {
  double acc = 0.0;
  int g = 0;
  for (; g + 8 <= G; g += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part[(int64_t)(g + u) * N + j];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += (double)v[u];
  }
  for (; g < G; ++g) acc += (double)part[(int64_t)g * N + j];
  return acc;
}

// CG launch 2 (one wave per 64 elements): Hp = sum_g part[g] + fl(lam p), den partial of dot(fl(cg_alpha Hp), p) per workgroup.
__device__ __forceinline__ void strip_hp_body(const float* part, const int G, const float* lam, const float* p, float* Hp,
                                              double* denpart, const int N, const float cg_alpha) {
  const int j = blockIdx.x * kColBlock + threadIdx.x;
  double t = 0.0;
  if (j < N) {
    const float pj = p[j];
    const float lp = lam[j] * pj;
    const float hp = (float)strip_sum(part, G, N, j) + lp;
    Hp[j] = hp;
    const float ahp = cg_alpha * hp;
    t = (double)ahp * (double)pj;
  }
  t = wave_sum(t);
  if (threadIdx.x == 0) denpart[blockIdx.x] = t;
}

// CG launch 3 (ONE workgroup of T threads): both step lengths from fp64 sums in a fixed order, then x, r, p.  Iteration 0 takes x = 0,
// r = p = rhs and r.r from rhs itself; rr travels to the next iteration in the workspace.  The last iteration writes out / coeff.
// DEN_SERIAL: every thread adds the den partials in workgroup order; else thread t takes partial t (nden <= T) and block_sum_w
// adds them.
template <int T, bool DEN_SERIAL>
__device__ __forceinline__ void strip_cg_update_body(const float* rhs, const float* w, const float* Hp, const double* denpart,
                                                     const int nden, double* rr_slot, float* x, float* r, float* p, float* out,
                                                     float* coeff, const int N, const int k, const int last, const float out_scale) {
  constexpr int W = T / 64;
  __shared__ double sred[W];
  const int tid = threadIdx.x;
  const float* rin = k == 0 ? rhs : r;
  const float* pin = k == 0 ? rhs : p;
  double rr;
  if (k == 0) {
    double s = 0.0;
    for (int j = tid; j < N; j += T) s += (double)rhs[j] * (double)rhs[j];
    rr = block_sum_w<W>(s, sred);
  } else {
    rr = *rr_slot;
  }
  double den = 0.0;
  if constexpr (DEN_SERIAL) {
    for (int b = 0; b < nden; ++b) den += denpart[b];
  } else {
    den = block_sum_w<W>(tid < nden ? denpart[tid] : 0.0, sred);
  }
  const float alpha = (float)rr / (float)den;
  double rn2 = 0.0;
  for (int j = tid; j < N; j += T) {
    const float t = alpha * Hp[j];
    const float rn = rin[j] - t;
    rn2 += (double)rn * (double)rn;
  }
  rn2 = block_sum_w<W>(rn2, sred);
  const float beta = (float)rn2 / (float)rr;
  for (int j = tid; j < N; j += T) {
    const float pj = pin[j];
    const float t = alpha * Hp[j];
    const float rn = rin[j] - t;
    const float ap = alpha * pj;
    float xn = (k == 0 ? 0.f : x[j]) + ap;
    const float bp = beta * pj;
    if (last) {
      if (out_scale != 0.f) xn = out_scale * xn;
      out[j] = xn;
      if (coeff) coeff[j] = w[j] * xn;
    } else {
      x[j] = xn;
      r[j] = rn;
      p[j] = rn + bp;
    }
  }
  if (tid == 0) *rr_slot = rn2;
}

// Neumann launch 2 (one wave per 64 elements): Hv = sum_g part[g] + fl(lam v); v' = v - fl(alpha Hv); p' = v' + p.  Iteration 0
// reads v = p = rhs.  The last iteration writes out / coeff.
__device__ __forceinline__ void strip_neumann_update_body(const float* part, const int G, const float* lam, const float* w,
                                                          const float* vin, const float* pin, float* v, float* p, float* out,
                                                          float* coeff, const int N, const float alpha, const int last,
                                                          const float out_scale) {
  const int j = blockIdx.x * kColBlock + threadIdx.x;
  if (j >= N) return;
  const float vj = vin[j];
  const float lv = lam[j] * vj;
  const float hv = (float)strip_sum(part, G, N, j) + lv;
  const float t = alpha * hv;
  const float vn = vj - t;
  float pn = vn + pin[j];
  if (last) {
    if (out_scale != 0.f) pn = out_scale * pn;
    out[j] = pn;
    if (coeff) coeff[j] = w[j] * pn;
  } else {
    v[j] = vn;
    p[j] = pn;
  }
}

// K == 0 (kThreads per workgroup): x = 0 (CG) | p = rhs (Neumann), scaled.
__device__ __forceinline__ void solve_k0_body(const float* rhs, const float* w, float* out, float* coeff, const int N, const int cg,
                                              const float out_scale) {
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= N) return;
  float o = cg ? 0.f : rhs[j];
  if (out_scale != 0.f) o = out_scale * o;
  out[j] = o;
  if (coeff) coeff[j] = w[j] * o;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
enum { kFormNone = -1, kFormAuto = 0, kFormSingle = 1, kFormStrips = 2 };
struct Plan {
  int form;   // kFormNone | kFormSingle | kFormStrips
  int G;      // strips
  int rps;    // rows per strip
};

// The checks every plan starts with, then the form: the forced one, or the first of single / strips that admits the shape.
// BHG_OK and *f, or BHG_ERR_ARG with the error set.  (A forced form the shape does not admit is the caller's error to word.)
inline int plan_form(const char* fn, bool empty, int n, int form, int strips, bool single_ok, bool strips_ok, int* f) {
  if (empty) { set_error("%s: empty problem", fn); return BHG_ERR_ARG; }
  if (n > (1 << 30)) { set_error("%s: more than 2^30 rows", fn); return BHG_ERR_ARG; }
  if (form < kFormAuto || form > kFormStrips) { set_error("%s: form must be 0 (auto), 1 (single) or 2 (strips)", fn); return BHG_ERR_ARG; }
  if (strips < 0 || strips > kMaxStrips) { set_error("%s: strips must be 0 (auto) .. %d", fn, kMaxStrips); return BHG_ERR_ARG; }
  *f = form != kFormAuto ? form : single_ok ? kFormSingle : strips_ok ? kFormStrips : kFormNone;
  return BHG_OK;
}

// the plan of form f; strips: G = `strips`, or `auto_G` when that is 0 (auto)
inline Plan plan_of(int f, int n, int strips, int auto_G) {
  Plan pl{f, 0, 0};
  if (f == kFormStrips) {
    pl.G = strips != 0 ? strips : auto_G;
    pl.rps = (int)(((int64_t)n + pl.G - 1) / pl.G);
  }
  return pl;
}

inline void plan_line(const Plan& pl, char* buf, size_t buf_bytes) {
  if (pl.form == kFormSingle)
    snprintf(buf, buf_bytes, "single: 1 launch per solve");
  else if (pl.form == kFormStrips)
    snprintf(buf, buf_bytes, "strips G=%d: %d rows per strip, 3 launches per cg iteration, 2 per neumann iteration", pl.G, pl.rps);
  else
    snprintf(buf, buf_bytes, "none");
}

// The workspace of the strips form for N elements, its vectors at byte `vec_off` (past the den partials): the pointers into `ws`
// (NULL: only `bytes` means anything) and the size the *_solve_ws_bytes functions report.
struct StripsWs {
  double *rr, *den;
  float *Hp, *x, *r, *p, *part;
  size_t bytes;
};
inline StripsWs strips_ws(void* ws, size_t vec_off, size_t N) {
  const size_t np = (N + 3) & ~(size_t)3, part_off = vec_off + 4 * sizeof(float) * np;
  const uintptr_t base = reinterpret_cast<uintptr_t>(ws);
  float* vecs = reinterpret_cast<float*>(base + vec_off);
  return StripsWs{reinterpret_cast<double*>(base + kWsRr), reinterpret_cast<double*>(base + kWsDen), vecs, vecs + np, vecs + 2 * np,
                  vecs + 3 * np, reinterpret_cast<float*>(base + part_off), part_off + sizeof(float) * (size_t)kMaxStrips * N};
}

// the post-pass kernels of a problem (their bodies are the ones above) and the thread count of its CG update
struct StripKernels {
  void (*hp)(const float*, int, const float*, const float*, float*, double*, int, float);
  void (*cg_update)(const float*, const float*, const float*, const double*, int, double*, float*, float*, float*, float*, float*, int,
                    int, int, float);
  int cg_threads;
  void (*neumann_update)(const float*, int, const float*, const float*, const float*, const float*, float*, float*, float*, float*, int,
                         float, int, float);
};

// The K loop (K > 0) of the strips form: 3 launches per CG iteration, 2 per Neumann iteration, none around them.  pass(dir, part)
// launches the problem's pass over X along `dir` into the [G][N] partials.  `a`: cg_alpha | alpha.
template <bool CG, typename Pass>
void run_strips(hipStream_t st, const StripKernels& kn, const StripsWs& s, int G, Pass pass, const float* lam, const float* w,
                const float* rhs, float* out, float* coeff, int N, int K, float a, float out_scale) {
  const int cb = (N + kColBlock - 1) / kColBlock;
  for (int k = 0; k < K; ++k) {
    const int last = k == K - 1;
    if (CG) {
      pass(k == 0 ? rhs : (const float*)s.p, s.part);
      hipLaunchKernelGGL(kn.hp, dim3(cb), dim3(kColBlock), 0, st, (const float*)s.part, G, lam, k == 0 ? rhs : (const float*)s.p, s.Hp,
                         s.den, N, a);
      hipLaunchKernelGGL(kn.cg_update, dim3(1), dim3(kn.cg_threads), 0, st, rhs, w, (const float*)s.Hp, (const double*)s.den, cb, s.rr,
                         s.x, s.r, s.p, out, coeff, N, k, last, out_scale);
    } else {
      pass(k == 0 ? rhs : (const float*)s.r, s.part);
      hipLaunchKernelGGL(kn.neumann_update, dim3(cb), dim3(kColBlock), 0, st, (const float*)s.part, G, lam, w,
                         k == 0 ? rhs : (const float*)s.r, k == 0 ? rhs : (const float*)s.p, s.r, s.p, out, coeff, N, a, last, out_scale);
    }
  }
}

}  // namespace bhg
