// bhg_layernorm.hip — the Hessian-vector product's share of a layer-normalisation layer, fused.
//
// Where it sits on the path: betty/hypergradient/cg.py:39-41 / neumann.py:62 take H p as the DOUBLE BACKWARD
// `torch.autograd.grad(in_grad, params, grad_outputs=p)`.  For a transformer inner problem (BASELINE cfg 4: RoBERTa-base, 25 nn.LayerNorm
// layers) ATen differentiates native_layer_norm_backward by DECOMPOSING it, as it does for batch norm: 216 ATen operator calls per layer
// and product on a 64 x 768 input, most of them activation-sized streaming passes.
//
// The backward of a layer norm over the last D elements of M rows (xh = (x - mean) * rstd, y = gamma * xh + beta) is the map
//     F : (x, gy, gamma) -> (gx, ggamma, gbeta)
//         g = gamma * gy        m1 = mean_j g        m2 = mean_j (g * xh)
//         gx = rstd * (g - m1 - xh * m2)        ggamma_j = sum_i gy_ij * xh_ij        gbeta_j = sum_i gy_ij
// and one Hessian-vector product needs its VECTOR-JACOBIAN product: given cotangents (a, b, c) of (gx, ggamma, gbeta), the gradients of
//     Phi = <a, gx> + <b, ggamma> + <c, gbeta>
// with respect to x, gy and gamma — mean and rstd being functions of x.  With the per-row means
//     A0 = mean a     A1 = mean (a * xh)     Sag = mean (a * g)     B0 = mean (b * gy)     B1 = mean (b * gy * xh)
// and at = a - A0 - xh * A1 they are (float64 restatement and its check against autograd: tests/layernorm_ref.py)
//     dgy      = gamma * rstd * at + b * xh + c
//     dgamma_j = sum_i gy_ij * rstd_i * at_ij
//     q        = -rstd * (g * A1 + m2 * a) + b * gy            t = rstd * (Sag - m1 * A0 - m2 * A1)
//     dx       = rstd * (q - mean q - xh * mean (q * xh)) - rstd * xh * t
// q depends on row means, but its own two row means do not need a second round over the row: mean xh = 0 and mean xh^2 = 1 are NOT
// used (they hold only to rounding for the fp32 statistics the forward saved) — the means of q are linear in sums of the first round:
//     mean q = -rstd * (m1 * A1 + m2 * A0) + B0        mean (q * xh) = -2 * rstd * m2 * A1 + B1
// so ONE round of seven row sums serves the whole row.
//
// TWO launches: k_ln_vjp_rows (a row lives in registers between its sums and its outputs: x, gy, a read once, dx, dgy written once; the
// thread <-> column mapping is fixed over the rows a workgroup walks, so each thread adds its columns' dgamma terms in fp64 registers;
// per-slice partials part[slice][D]) and k_ln_vjp_combine (one thread per column adds the slices in slice order; skipped when dgamma is
// not wanted).  No atomics: bitwise run-to-run deterministic, like the rest of the library.  20 algorithmic bytes per element.
//
// Layout: fp32, M contiguous rows of D.  D % 4 == 0: every access of the row tensors is a 16-byte vector; otherwise scalar accesses.
#include "bhg_common.hpp"

namespace bhg {
namespace {

constexpr int kLnMaxSlices = 64;   // slices of the M rows (workgroups of the row pass): what bhg_layernorm_ws_bytes reserves
constexpr int kLnMaxD = 8192;      // 32 elements per thread and array at 256 threads per row
constexpr int kLnSums = 7;

struct LnArgs {
  const float* x; const float* gy; const float* a;      // a may be NULL (cotangent of gx not defined: treated as zero)
  const float* gamma;                                   // may be NULL (elementwise_affine = False: gamma = 1)
  const float* mean; const float* rstd;                 // [M]
  const float* b; const float* c;                       // [D], may be NULL (zero)
  float* dx; float* dgy; float* dgamma;                 // dgamma may be NULL (no partials, no combine pass)
  double* part;                                         // [slices][D]
  long long M;
  int D;
  int vec;                                              // 4: 16-byte accesses (D % 4 == 0); 1: scalar
  int tpr, ltpr;                                        // threads per row (a power of two <= 256) and its log2
  int rows;                                             // 256 / tpr rows side by side: one row group
  int nv;                                               // vectors per thread: ceil((D / vec) / tpr)
  int inst;                                             // the kernel instance's vectors per thread: nv rounded up to a supported count
  long long groups, gps;                                // row groups, and row groups per slice
  int slices;                                           // workgroups of the row pass: ceil(groups / gps) <= kLnMaxSlices, none empty
};

template <int VEC>
__device__ __forceinline__ void ln_load(const float* __restrict__ p, float* v) {
  if (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = p[0];
  }
}
template <int VEC>
__device__ __forceinline__ void ln_store(float* __restrict__ p, const float* v) {
  if (VEC == 4)
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else
    p[0] = v[0];
}

// Keeps the compiler from gathering the gamma / b / c fetches of a whole 32-element row in front of the arithmetic (three more arrays'
// worth of live registers: the kernel then needs a private segment).  No instruction: memory accesses do not move across it.
__device__ __forceinline__ void ln_fence() { asm volatile("" ::: "memory"); }

// The same value, but one the compiler cannot trace: what is computed from it is computed where it is used.  No instruction.
__device__ __forceinline__ int ln_opaque(int v) { asm volatile("" : "+v"(v)); return v; }

// Column of element e (vector e / VEC, lane e % VEC) of thread tv of a row: may lie past the row's end (the caller masks).
template <int VEC>
__device__ __forceinline__ int ln_col(const int e, const int tv, const int tpr) { return (tv + (e / VEC) * tpr) * VEC + e % VEC; }

// The kLnSums sums over the tpr threads of a row, valid in every thread of the row.  tpr < 64: a butterfly inside the wave (both partners
// add the same two numbers, so the row's threads hold the same bits); tpr >= 64: the wave sum, then the row's waves in wave order.
// Contains barriers when tpr > 64: every thread of the workgroup calls it the same number of times.
__device__ __forceinline__ void ln_row_sums(double (&s)[kLnSums], const int tpr, double* red) {
  if (tpr >= 64) {
#pragma unroll
    for (int i = 0; i < kLnSums; ++i) s[i] = wave_sum(s[i]);
  } else {
    for (int m = tpr >> 1; m > 0; m >>= 1) {
#pragma unroll
      for (int i = 0; i < kLnSums; ++i) s[i] += __shfl_xor(s[i], m);
    }
  }
  if (tpr > 64) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();  // protect `red` against the previous row group
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < kLnSums; ++i) red[i * kWaves + wave] = s[i];
    }
    __syncthreads();
    const int nw = tpr >> 6, w0 = (wave / nw) * nw;
#pragma unroll
    for (int i = 0; i < kLnSums; ++i) {
      double t = 0.0;
      for (int j = 0; j < nw; ++j) t += red[i * kWaves + w0 + j];
      s[i] = t;
    }
  }
}

// grid = slices.  Workgroup s walks the row groups [s * gps, min((s + 1) * gps, groups)); row group g is the rows g * rows + tr,
// tr = thread / tpr; thread tv = thread % tpr of a row owns the vectors tv, tv + tpr, ... (< NV of them) of every row it meets.
template <int VEC, int NV>
__global__ __launch_bounds__(kThreads) void k_ln_vjp_rows(LnArgs q) {
  constexpr int E = VEC * NV;
  __shared__ double red[kLnSums * kWaves];
  __shared__ double cols[NV == 2 ? kThreads * E : 1];   // rows side by side (tpr < 256) only occur with two vectors per thread
  const int tid = threadIdx.x, tpr = q.tpr, tv = tid & (tpr - 1), tr = tid >> q.ltpr;
  const int nvec = q.D / VEC;
  const double inv_d = 1.0 / (double)q.D;
  const bool has_a = q.a != nullptr, want_dgamma = q.dgamma != nullptr;
  // An absent gamma / b / c is read as element 0 of `mean` (M >= 1) and the value discarded: a select per element, where a test of
  // the pointer is a branch around every fetch.
  const bool hg = q.gamma != nullptr, hb = q.b != nullptr, hc = q.c != nullptr;
  const float* __restrict__ gp = hg ? q.gamma : q.mean;
  const float* __restrict__ bp = hb ? q.b : q.mean;
  const float* __restrict__ cp = hc ? q.c : q.mean;
  const int mg = hg ? -1 : 0, mb = hb ? -1 : 0, mc = hc ? -1 : 0;
  double acc[E];
#pragma unroll
  for (int e = 0; e < E; ++e) acc[e] = 0.0;

  const long long g0 = (long long)blockIdx.x * q.gps;
  const long long g1 = g0 + q.gps < q.groups ? g0 + q.gps : q.groups;
  for (long long g = g0; g < g1; ++g) {
    const long long row = g * q.rows + tr;
    const bool live = row < q.M;
    // addresses: a workgroup-uniform 64-bit base (the row group) plus a 32-bit offset (< 256 * 32 elements) per thread and vector
    const long long gbase = g * q.rows * q.D;
    const float* __restrict__ xg = q.x + gbase;
    const float* __restrict__ gyg = q.gy + gbase;
    const float* __restrict__ ag = has_a ? q.a + gbase : nullptr;
    const unsigned rbase = (unsigned)(tr * q.D);
    float xv[E], gv[E], av[E];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int v = tv + k * tpr;
      const bool in = v < nvec;
#pragma unroll
      for (int u = 0; u < VEC; ++u) {
        xv[k * VEC + u] = 0.f; gv[k * VEC + u] = 0.f; av[k * VEC + u] = 0.f;
      }
      if (in && live) {
        const unsigned off = rbase + (unsigned)(v * VEC);
        ln_load<VEC>(xg + off, xv + k * VEC);
        ln_load<VEC>(gyg + off, gv + k * VEC);
        if (has_a) ln_load<VEC>(ag + off, av + k * VEC);
      }
    }
    const double mu = live ? (double)q.mean[row] : 0.0, r = live ? (double)q.rstd[row] : 0.0;
    // elements outside the row (or rows outside the tensor) were loaded as zeros of gy and a: every term below carries one of the two
    double s[kLnSums];
#pragma unroll
    for (int i = 0; i < kLnSums; ++i) s[i] = 0.0;
    // gamma, b, c ([D]) are fetched where they are used, in both passes over the row, not held: they stay in the cache, and 32 elements
    // per thread of three more arrays would not fit the register file.  Scalar loads: only the row tensors need 16-byte alignment.
    // (the column index goes through ln_opaque in each pass: hoisted out of the row loop, the addresses of three vectors at every element
    // cost six registers per element)
    const int tv1 = ln_opaque(tv);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int col = ln_col<VEC>(e, tv1, tpr), cc = col < q.D ? col : 0;
      const double xh = ((double)xv[e] - mu) * r;
      const float lg = gp[cc & mg], lb = bp[cc & mb];   // fetched whether present or not
      const double gm = hg ? (double)lg : 1.0, bb = hb ? (double)lb : 0.0;
      const double gg = gm * (double)gv[e], aa = (double)av[e], bg = bb * (double)gv[e];
      s[0] += gg;
      s[1] += gg * xh;
      s[2] += aa;
      s[3] += aa * xh;
      s[4] += aa * gg;
      s[5] += bg;
      s[6] += bg * xh;
      if (E > 8 && (e & 1) == 1) ln_fence();
    }
    ln_row_sums(s, tpr, red);
    // The row is held as the fp32 values that were loaded, nothing else: without this the compiler keeps the first pass's fp64
    // intermediates (xh, gamma * gy, ... : ~20 registers per element instead of 5) alive for the second pass.  No instruction.
#pragma unroll
    for (int e = 0; e < E; ++e) asm volatile("" : "+v"(xv[e]), "+v"(gv[e]), "+v"(av[e]));
    const double m1 = s[0] * inv_d, m2 = s[1] * inv_d, A0 = s[2] * inv_d, A1 = s[3] * inv_d, Sag = s[4] * inv_d;
    const double B0 = s[5] * inv_d, B1 = s[6] * inv_d;
    const double Q0 = -r * (m1 * A1 + m2 * A0) + B0;    // mean q
    const double Q1 = -2.0 * r * m2 * A1 + B1;          // mean (q * xh)
    const double t = r * (Sag - m1 * A0 - m2 * A1);
    const int tv2 = ln_opaque(tv);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      float ox[VEC], og[VEC];
#pragma unroll
      for (int u = 0; u < VEC; ++u) {
        const int e = k * VEC + u;
        const int col = ln_col<VEC>(e, tv2, tpr), cc = col < q.D ? col : 0;
        const double xh = ((double)xv[e] - mu) * r;
        const float lg = gp[cc & mg], lb = bp[cc & mb], lc = cp[cc & mc];
        const double gm = hg ? (double)lg : 1.0, bb = hb ? (double)lb : 0.0, cv = hc ? (double)lc : 0.0;
        const double gy = (double)gv[e], aa = (double)av[e];
        const double at = aa - A0 - xh * A1;
        og[u] = (float)(gm * r * at + bb * xh + cv);
        acc[e] += gy * r * at;
        const double qv = -r * (gm * gy * A1 + m2 * aa) + bb * gy;
        ox[u] = (float)(r * (qv - Q0 - xh * Q1) - r * xh * t);
      }
      const int v = tv2 + k * tpr;
      if (v < nvec && live) {
        const unsigned off = rbase + (unsigned)(v * VEC);
        ln_store<VEC>(q.dx + gbase + off, ox);
        ln_store<VEC>(q.dgy + gbase + off, og);
      }
      if (E > 8 && ((k * VEC + VEC - 1) & 3) == 3) ln_fence();
    }
  }

  if (!want_dgamma) return;   // uniform over the workgroup
  double* out = q.part + (long long)blockIdx.x * q.D;
  if (NV == 2 && q.rows > 1) {
    // rows side by side: the threads tr = 0 .. rows - 1 of one column are added in tr order
    const int width = tpr * E;   // >= D; rows * width = kThreads * E
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
      for (int u = 0; u < VEC; ++u) cols[tr * width + (tv + k * tpr) * VEC + u] = acc[k * VEC + u];
    __syncthreads();
    for (int col = tid; col < q.D; col += kThreads) {
      double v = 0.0;
      for (int j = 0; j < q.rows; ++j) v += cols[j * width + col];
      out[col] = v;
    }
  } else {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int v = tv + k * tpr;
      if (v < nvec) {
#pragma unroll
        for (int u = 0; u < VEC; ++u) out[v * VEC + u] = acc[k * VEC + u];
      }
    }
  }
}

// grid = ceil(D / 256): one thread per column adds the slices in slice order.
__global__ __launch_bounds__(kThreads) void k_ln_vjp_combine(const double* __restrict__ part, float* __restrict__ dgamma, const int D,
                                                             const int slices) {
  const int col = blockIdx.x * kThreads + threadIdx.x;
  if (col >= D) return;
  double v = 0.0;
  for (int s = 0; s < slices; ++s) v += part[(long long)s * D + col];
  dgamma[col] = (float)v;
}

// Why the launch does not take a shape, or NULL where it does: bhg_layernorm_backward_vjp and bhg_layernorm_plan refuse the same shapes.
inline const char* ln_shape_error(long long M, int D) {
  if (!(M > 0 && D > 0)) return "empty tensor";
  if (D > kLnMaxD) return "more than 8192 elements per row";
  if (M > (1LL << 40)) return "more than 2^40 rows";   // keeps every 64-bit product below far from overflow
  return nullptr;
}

// The slicing of the M rows, in closed form (nothing is searched: tpr comes from a shift loop of at most 8 steps, `gps` from the bounded
// slice count and the count again from gps, so it cannot exceed the bound and no slice is empty).
inline const char* ln_plan(LnArgs* q, long long M, int D) {
  const char* bad = ln_shape_error(M, D);
  if (bad) return bad;
  q->M = M; q->D = D;
  q->vec = D % 4 == 0 ? 4 : 1;
  const int nvec = D / q->vec;
  // two vectors per thread until a row takes the whole workgroup: a narrow row leaves no thread idle (256 / tpr rows side by side)
  int tpr = 1, ltpr = 0;
  while (tpr < kThreads && 2 * tpr < nvec) { tpr <<= 1; ++ltpr; }
  q->tpr = tpr; q->ltpr = ltpr;
  q->rows = kThreads / tpr;
  q->nv = (nvec + tpr - 1) / tpr;
  // supported instance counts: 16-byte path 2, 4, 8; scalar path 2, 8, 32 (D <= 8192: nv <= 8 resp. 32)
  if (q->vec == 4) q->inst = q->nv <= 2 ? 2 : q->nv <= 4 ? 4 : 8;
  else q->inst = q->nv <= 2 ? 2 : q->nv <= 8 ? 8 : 32;
  q->groups = (M + q->rows - 1) / q->rows;
  long long slices = q->groups < kLnMaxSlices ? q->groups : kLnMaxSlices;
  q->gps = (q->groups + slices - 1) / slices;
  q->slices = (int)((q->groups + q->gps - 1) / q->gps);
  return nullptr;
}

template <int VEC, int NV>
inline void ln_launch_rows(const LnArgs& q, hipStream_t st) {
  hipLaunchKernelGGL((k_ln_vjp_rows<VEC, NV>), dim3(q.slices), dim3(kThreads), 0, st, q);
}

}  // namespace
}  // namespace bhg

using namespace bhg;

extern "C" {

size_t bhg_layernorm_ws_bytes(int D) { return D > 0 && D <= kLnMaxD ? sizeof(double) * kLnMaxSlices * (size_t)D : 0; }

int bhg_layernorm_plan(long long M, int D, char* buf, size_t buf_bytes) {
  BHG_REQUIRE(buf && buf_bytes > 0, "NULL buffer");
  LnArgs q{};
  const char* bad = ln_plan(&q, M, D);
  BHG_REQUIRE(!bad, bad);
  const int len = snprintf(buf, buf_bytes, "vec=%d tpr=%d rows=%d nv=%d inst=%d groups=%lld gps=%lld slices=%d max_slices=%d ws=%lld",
                           q.vec, q.tpr, q.rows, q.nv, q.inst, q.groups, q.gps, q.slices, kLnMaxSlices,
                           (long long)(sizeof(double) * (size_t)q.slices * (size_t)D));
  BHG_REQUIRE(len > 0 && (size_t)len < buf_bytes, "buffer too small for the plan line");
  return BHG_OK;
}

int bhg_layernorm_backward_vjp(const float* x, const float* gy, const float* a, const float* gamma, const float* mean, const float* rstd,
                               const float* b, const float* c, long long M, int D, float* dx, float* dgy, float* dgamma, void* ws,
                               size_t ws_bytes, void* stream) {
  BHG_REQUIRE(x && gy && mean && rstd && dx && dgy && ws, "null pointer");
  LnArgs q{};
  const char* bad = ln_plan(&q, M, D);
  BHG_REQUIRE(!bad, bad);
  BHG_REQUIRE(ws_bytes >= bhg_layernorm_ws_bytes(D), "workspace smaller than bhg_layernorm_ws_bytes(D)");
  BHG_REQUIRE(((uintptr_t)ws & 7) == 0, "the workspace must be 8-byte aligned");
  if (q.vec == 4)
    for (const void* p : {(const void*)x, (const void*)gy, (const void*)a, (const void*)dx, (const void*)dgy})
      BHG_REQUIRE(((uintptr_t)p & 15) == 0, "x, gy, a, dx and dgy must be 16-byte aligned when D is a multiple of 4");
  q.x = x; q.gy = gy; q.a = a; q.gamma = gamma; q.mean = mean; q.rstd = rstd; q.b = b; q.c = c;
  q.dx = dx; q.dgy = dgy; q.dgamma = dgamma; q.part = static_cast<double*>(ws);
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (q.vec * 100 + q.inst) {
    case 402: ln_launch_rows<4, 2>(q, st); break;
    case 404: ln_launch_rows<4, 4>(q, st); break;
    case 408: ln_launch_rows<4, 8>(q, st); break;
    case 102: ln_launch_rows<1, 2>(q, st); break;
    case 108: ln_launch_rows<1, 8>(q, st); break;
    default: ln_launch_rows<1, 32>(q, st); break;
  }
  if (dgamma) hipLaunchKernelGGL(k_ln_vjp_combine, dim3((D + kThreads - 1) / kThreads), dim3(kThreads), 0, st, q.part, dgamma, D, q.slices);
  BHG_HIP_CHECK(hipGetLastError());
  return BHG_OK;
}

}  // extern "C"
