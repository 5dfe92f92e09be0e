// bhg_rmsnorm.hip — the Hessian-vector product's share of an RMS-normalisation layer, fused.
//
// Where it sits on the path: betty/hypergradient/cg.py:39-41 / neumann.py:62 take H p as the DOUBLE BACKWARD
// `torch.autograd.grad(in_grad, params, grad_outputs=p)`.  nn.RMSNorm is the normalisation of a LLaMA-style pre-norm decoder block (twice
// per block, once more before the head); on the GPU it runs aten::_fused_rms_norm, whose derivative formula becomes a chain of
// element-wise operators as soon as grad mode is on.
//
// The backward of an RMS norm over the last D elements of M rows (r = rstd = rsqrt(mean_j x^2 + eps), xh = x * r, y = gamma * xh) is
//     F : (x, gy, gamma) -> (gx, ggamma)
//         g = gamma * gy        m2 = mean_j (g * xh)
//         gx = r * (g - xh * m2)        ggamma_j = sum_i gy_ij * xh_ij
// and one Hessian-vector product needs its VECTOR-JACOBIAN product: given cotangents (a, b) of (gx, ggamma), the gradients of
//     Phi = <a, gx> + <b, ggamma>
// with respect to x, gy and gamma — r being a function of x.  With the per-row means
//     A1 = mean (a * xh)     Sag = mean (a * g)     B1 = mean (b * gy * xh)
// and at = a - xh * A1 they are (float64 restatement and its check against autograd: tests/rmsnorm_ref.py)
//     dgy      = gamma * r * at + b * xh
//     dgamma_j = sum_i gy_ij * r_i * at_ij
//     q        = -r * (g * A1 + m2 * a) + b * gy            t = r * (Sag - m2 * A1)
//     dx       = r * (q - xh * mean (q * xh)) - r * xh * t
// mean xh^2 = 1 is NOT used (it is 1 - eps * r^2: far from 1 for a row whose mean square is of the order of eps) — the mean of q * xh is
// linear in sums of the first round:
//     mean (q * xh) = -2 * r * m2 * A1 + B1
// so ONE round of four row sums (m2, A1, Sag, B1), in fp64, serves the whole row.
//
// TWO launches: k_rms_vjp_rows (a row lives in registers between its sums and its outputs: x, gy, a read once, dx, dgy written once; the
// thread <-> column mapping is fixed over the rows a workgroup walks, so each thread adds its columns' dgamma terms in fp64 registers;
// per-slice partials part[slice][D]) and k_rms_vjp_combine (the slices of a column are added in slice order; skipped when dgamma is not
// wanted).  No atomics: bitwise run-to-run deterministic, like the rest of the library.  20 algorithmic bytes per element.
//
// The row pass is bhg_layernorm.hip's with four sums instead of seven, no mean and no beta — and WITHOUT its bound of 64 workgroups: the
// slices fill the chip (rms_plan below).
//
// Registers of k_rms_vjp_rows<VEC, NV> on gfx950 (-Rpass-analysis=kernel-resource-usage; no instance has a private segment), and the
// waves per SIMD at that count — one wave of a workgroup per SIMD, so also the workgroups of 256 threads a CU holds:
//     <4, 2>  126 VGPRs            4          <1, 2>    64 VGPRs            8
//     <4, 4>  166 VGPRs            3          <1, 8>   114 VGPRs            4
//     <4, 8>  256 VGPRs + 4 AGPRs  1          <1, 32>  256 VGPRs + 42 AGPRs 1
// (x, gy, a) of 32 elements per thread are 96 registers and their 32 fp64 accumulators 64 more: the two 32-element instances come out
// four resp. 42 registers above the 256 that two waves per SIMD allow, and asking the compiler for two waves (amdgpu_waves_per_eu)
// makes it spill 3 resp. 44 registers to a private segment.  They stay at one wave per SIMD: 256 workgroups of the row pass.
//
// Layout: fp32, M contiguous rows of D.  D % 4 == 0: every access of the row tensors is a 16-byte vector; otherwise scalar accesses.
#include "bhg_common.hpp"

namespace bhg {
namespace {

constexpr int kRmsCUs = 256;        // MI355X
constexpr int kRmsMaxD = 8192;      // 32 elements per thread and array at 256 threads per row
constexpr int kRmsSums = 4;
constexpr int kRmsMinRows = 8;      // rows per slice, M allowing: a slice costs 16 D bytes of partials (8 D written, 8 D read back), a
                                    // row 20 D bytes, so 8 rows per slice keep the partials to 10 % of the traffic
constexpr int kRmsCombCols = 64;    // k_rms_vjp_combine: columns per workgroup, and 256 / 64 = 4 runs of slices per column

struct RmsArgs {
  const float* x; const float* gy; const float* a;      // a may be NULL (cotangent of gx not defined: treated as zero)
  const float* gamma;                                   // may be NULL (elementwise_affine = False: gamma = 1)
  const float* rstd;                                    // [M]
  const float* b;                                       // [D], may be NULL (zero)
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
  int slices, max_slices;                               // workgroups of the row pass: ceil(groups / gps) <= max_slices, none empty
};

template <int VEC>
__device__ __forceinline__ void rms_load(const float* __restrict__ p, float* v) {
  if (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = p[0];
  }
}
template <int VEC>
__device__ __forceinline__ void rms_store(float* __restrict__ p, const float* v) {
  if (VEC == 4)
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else
    p[0] = v[0];
}

// Keeps the compiler from gathering the gamma / b fetches of a whole 32-element row in front of the arithmetic (two more arrays' worth
// of live registers).  No instruction: memory accesses do not move across it.
__device__ __forceinline__ void rms_fence() { asm volatile("" ::: "memory"); }

// The same value, but one the compiler cannot trace: what is computed from it is computed where it is used.  No instruction.
__device__ __forceinline__ int rms_opaque(int v) { asm volatile("" : "+v"(v)); return v; }

// Column of element e (vector e / VEC, lane e % VEC) of thread tv of a row: may lie past the row's end (the caller masks).
template <int VEC>
__device__ __forceinline__ int rms_col(const int e, const int tv, const int tpr) { return (tv + (e / VEC) * tpr) * VEC + e % VEC; }

// The kRmsSums sums over the tpr threads of a row, valid in every thread of the row.  tpr < 64: a butterfly inside the wave (both
// partners add the same two numbers, so the row's threads hold the same bits); tpr >= 64: the wave sum, then the row's waves in wave
// order.  Contains barriers when tpr > 64: every thread of the workgroup calls it the same number of times.
__device__ __forceinline__ void rms_row_sums(double (&s)[kRmsSums], const int tpr, double* red) {
  if (tpr >= 64) {
#pragma unroll
    for (int i = 0; i < kRmsSums; ++i) s[i] = wave_sum(s[i]);
  } else {
    for (int m = tpr >> 1; m > 0; m >>= 1) {
#pragma unroll
      for (int i = 0; i < kRmsSums; ++i) s[i] += __shfl_xor(s[i], m);
    }
  }
  if (tpr > 64) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();  // protect `red` against the previous row group
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < kRmsSums; ++i) red[i * kWaves + wave] = s[i];
    }
    __syncthreads();
    const int nw = tpr >> 6, w0 = (wave / nw) * nw;
#pragma unroll
    for (int i = 0; i < kRmsSums; ++i) {
      double t = 0.0;
      for (int j = 0; j < nw; ++j) t += red[i * kWaves + w0 + j];
      s[i] = t;
    }
  }
}

// grid = slices.  Workgroup s walks the row groups [s * gps, min((s + 1) * gps, groups)); row group g is the rows g * rows + tr,
// tr = thread / tpr; thread tv = thread % tpr of a row owns the vectors tv, tv + tpr, ... (< NV of them) of every row it meets.
template <int VEC, int NV>
__global__ __launch_bounds__(kThreads) void k_rms_vjp_rows(RmsArgs q) {
  constexpr int E = VEC * NV;
  __shared__ double red[kRmsSums * kWaves];
  __shared__ double cols[NV == 2 ? kThreads * E : 1];   // rows side by side (tpr < 256) only occur with two vectors per thread
  const int tid = threadIdx.x, tpr = q.tpr, tv = tid & (tpr - 1), tr = tid >> q.ltpr;
  const int nvec = q.D / VEC;
  const double inv_d = 1.0 / (double)q.D;
  const bool has_a = q.a != nullptr, want_dgamma = q.dgamma != nullptr;
  // An absent gamma / b is read as element 0 of `rstd` (M >= 1) and the value discarded: a select per element, where a test of the
  // pointer is a branch around every fetch.
  const bool hg = q.gamma != nullptr, hb = q.b != nullptr;
  const float* __restrict__ gp = hg ? q.gamma : q.rstd;
  const float* __restrict__ bp = hb ? q.b : q.rstd;
  const int mg = hg ? -1 : 0, mb = hb ? -1 : 0;
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
        rms_load<VEC>(xg + off, xv + k * VEC);
        rms_load<VEC>(gyg + off, gv + k * VEC);
        if (has_a) rms_load<VEC>(ag + off, av + k * VEC);
      }
    }
    const double r = live ? (double)q.rstd[row] : 0.0;
    // elements outside the row (or rows outside the tensor) were loaded as zeros of gy and a: every term below carries one of the two
    double s[kRmsSums];
#pragma unroll
    for (int i = 0; i < kRmsSums; ++i) s[i] = 0.0;
    // gamma and b ([D]) are fetched where they are used, in both passes over the row, not held: they stay in the cache, and 32 elements
    // per thread of two more arrays would not fit the register file.  Scalar loads: only the row tensors need 16-byte alignment.
    // (the column index goes through rms_opaque in each pass: hoisted out of the row loop, the addresses of two vectors at every element
    // cost four registers per element)
    const int tv1 = rms_opaque(tv);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int col = rms_col<VEC>(e, tv1, tpr), cc = col < q.D ? col : 0;
      const double xh = (double)xv[e] * r;
      const float lg = gp[cc & mg], lb = bp[cc & mb];   // fetched whether present or not
      const double gm = hg ? (double)lg : 1.0, bb = hb ? (double)lb : 0.0;
      const double gg = gm * (double)gv[e], aa = (double)av[e], bg = bb * (double)gv[e];
      s[0] += gg * xh;
      s[1] += aa * xh;
      s[2] += aa * gg;
      s[3] += bg * xh;
      if (E > 8 && (e & 1) == 1) rms_fence();
    }
    rms_row_sums(s, tpr, red);
    // The row is held as the fp32 values that were loaded, nothing else: without this the compiler keeps the first pass's fp64
    // intermediates alive for the second pass.  No instruction.
#pragma unroll
    for (int e = 0; e < E; ++e) asm volatile("" : "+v"(xv[e]), "+v"(gv[e]), "+v"(av[e]));
    const double m2 = s[0] * inv_d, A1 = s[1] * inv_d, Sag = s[2] * inv_d, B1 = s[3] * inv_d;
    const double Q1 = -2.0 * r * m2 * A1 + B1;          // mean (q * xh)
    const double t = r * (Sag - m2 * A1);
    const int tv2 = rms_opaque(tv);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      float ox[VEC], og[VEC];
#pragma unroll
      for (int u = 0; u < VEC; ++u) {
        const int e = k * VEC + u;
        const int col = rms_col<VEC>(e, tv2, tpr), cc = col < q.D ? col : 0;
        const double xh = (double)xv[e] * r;
        const float lg = gp[cc & mg], lb = bp[cc & mb];
        const double gm = hg ? (double)lg : 1.0, bb = hb ? (double)lb : 0.0;
        const double gy = (double)gv[e], aa = (double)av[e];
        const double at = aa - xh * A1;
        og[u] = (float)(gm * r * at + bb * xh);
        acc[e] += gy * r * at;
        const double qv = -r * (gm * gy * A1 + m2 * aa) + bb * gy;
        ox[u] = (float)(r * (qv - xh * Q1) - r * xh * t);
      }
      const int v = tv2 + k * tpr;
      if (v < nvec && live) {
        const unsigned off = rbase + (unsigned)(v * VEC);
        rms_store<VEC>(q.dx + gbase + off, ox);
        rms_store<VEC>(q.dgy + gbase + off, og);
      }
      if (E > 8 && ((k * VEC + VEC - 1) & 3) == 3) rms_fence();
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

// grid = ceil(D / 64).  A workgroup owns 64 columns; thread (run, c) = (thread / 64, thread % 64) adds run `run` of the slices of its
// column — the slices [run * per, (run + 1) * per), per = ceil(slices / 4) — in slice order, and the four runs are added in run order:
// a fixed order whatever the slice count, with four times the loads in flight of one thread per column.
__global__ __launch_bounds__(kThreads) void k_rms_vjp_combine(const double* __restrict__ part, float* __restrict__ dgamma, const int D,
                                                              const int slices) {
  constexpr int kRuns = kThreads / kRmsCombCols;
  __shared__ double runs[kRuns][kRmsCombCols];
  const int c = threadIdx.x & (kRmsCombCols - 1), run = threadIdx.x / kRmsCombCols;
  const int col = blockIdx.x * kRmsCombCols + c;
  const int per = (slices + kRuns - 1) / kRuns;
  const int s0 = run * per, s1 = s0 + per < slices ? s0 + per : slices;
  double v = 0.0;
  if (col < D) {
#pragma unroll 4
    for (int s = s0; s < s1; ++s) v += part[(long long)s * D + col];
  }
  runs[run][c] = v;
  __syncthreads();
  if (run == 0 && col < D) {
    double t = runs[0][c];
#pragma unroll
    for (int j = 1; j < kRuns; ++j) t += runs[j][c];
    dgamma[col] = (float)t;
  }
}

// Why the launch does not take a shape, or NULL where it does: bhg_rmsnorm_backward_vjp and bhg_rmsnorm_plan refuse the same shapes.
inline const char* rms_shape_error(long long M, int D) {
  if (!(M > 0 && D > 0)) return "empty tensor";
  if (D > kRmsMaxD) return "more than 8192 elements per row";
  if (M > (1LL << 40)) return "more than 2^40 rows";   // keeps every 64-bit product below far from overflow
  return nullptr;
}

// Workgroups of the row pass that are resident at once: the CUs times the workgroups a CU holds at the instance's register count (the
// table in the header of this file).
inline int rms_max_slices(int vec, int inst) {
  const int per_cu = vec == 4 ? (inst == 2 ? 4 : inst == 4 ? 3 : 1) : (inst == 2 ? 8 : inst == 8 ? 4 : 1);
  return kRmsCUs * per_cu;
}

// The slicing of the M rows, in closed form (nothing is searched: tpr comes from a shift loop of at most 8 steps, `gps` from the bounded
// slice count and the count again from gps, so it cannot exceed the bound and no slice is empty).  The slice count is what fills the
// chip once (rms_max_slices), but no more than leaves every slice kRmsMinRows rows: gps * rows >= kRmsMinRows whenever there is more
// than one slice, so slices <= ceil(M / kRmsMinRows).
inline const char* rms_plan(RmsArgs* q, long long M, int D) {
  const char* bad = rms_shape_error(M, D);
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
  q->max_slices = rms_max_slices(q->vec, q->inst);
  q->groups = (M + q->rows - 1) / q->rows;
  const long long min_gps = (kRmsMinRows + q->rows - 1) / q->rows;
  long long slices = q->groups / min_gps;
  if (slices < 1) slices = 1;
  if (slices > q->max_slices) slices = q->max_slices;
  q->gps = (q->groups + slices - 1) / slices;
  q->slices = (int)((q->groups + q->gps - 1) / q->gps);
  return nullptr;
}

template <int VEC, int NV>
inline void rms_launch_rows(const RmsArgs& q, hipStream_t st) {
  hipLaunchKernelGGL((k_rms_vjp_rows<VEC, NV>), dim3(q.slices), dim3(kThreads), 0, st, q);
}

}  // namespace
}  // namespace bhg

using namespace bhg;

extern "C" {

size_t bhg_rmsnorm_ws_bytes(long long M, int D) {
  RmsArgs q{};
  return rms_plan(&q, M, D) ? 0 : sizeof(double) * (size_t)q.slices * (size_t)D;
}

int bhg_rmsnorm_plan(long long M, int D, char* buf, size_t buf_bytes) {
  BHG_REQUIRE(buf && buf_bytes > 0, "NULL buffer");
  RmsArgs q{};
  const char* bad = rms_plan(&q, M, D);
  BHG_REQUIRE(!bad, bad);
  const int len = snprintf(buf, buf_bytes, "vec=%d tpr=%d rows=%d nv=%d inst=%d groups=%lld gps=%lld slices=%d max_slices=%d ws=%lld",
                           q.vec, q.tpr, q.rows, q.nv, q.inst, q.groups, q.gps, q.slices, q.max_slices,
                           (long long)(sizeof(double) * (size_t)q.slices * (size_t)D));
  BHG_REQUIRE(len > 0 && (size_t)len < buf_bytes, "buffer too small for the plan line");
  return BHG_OK;
}

int bhg_rmsnorm_backward_vjp(const float* x, const float* gy, const float* a, const float* gamma, const float* rstd, const float* b,
                             long long M, int D, float* dx, float* dgy, float* dgamma, void* ws, size_t ws_bytes, void* stream) {
  RmsArgs q{};
  const char* bad = rms_plan(&q, M, D);
  BHG_REQUIRE(!bad, bad);
  BHG_REQUIRE(x && gy && rstd && dx && dgy, "null pointer");
  BHG_REQUIRE(gamma || !(b || dgamma), "b and dgamma need gamma");
  if (dgamma) {
    BHG_REQUIRE(ws, "dgamma needs a workspace");
    BHG_REQUIRE(ws_bytes >= sizeof(double) * (size_t)q.slices * (size_t)D, "workspace smaller than bhg_rmsnorm_ws_bytes(M, D)");
    BHG_REQUIRE(((uintptr_t)ws & 7) == 0, "the workspace must be 8-byte aligned");
  }
  if (q.vec == 4)
    for (const void* p : {(const void*)x, (const void*)gy, (const void*)a, (const void*)dx, (const void*)dgy})
      BHG_REQUIRE(((uintptr_t)p & 15) == 0, "x, gy, a, dx and dgy must be 16-byte aligned when D is a multiple of 4");
  q.x = x; q.gy = gy; q.a = a; q.gamma = gamma; q.rstd = rstd; q.b = b;
  q.dx = dx; q.dgy = dgy; q.dgamma = dgamma; q.part = static_cast<double*>(ws);
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (q.vec * 100 + q.inst) {
    case 402: rms_launch_rows<4, 2>(q, st); break;
    case 404: rms_launch_rows<4, 4>(q, st); break;
    case 408: rms_launch_rows<4, 8>(q, st); break;
    case 102: rms_launch_rows<1, 2>(q, st); break;
    case 108: rms_launch_rows<1, 8>(q, st); break;
    default: rms_launch_rows<1, 32>(q, st); break;
  }
  if (dgamma)
    hipLaunchKernelGGL(k_rms_vjp_combine, dim3((D + kRmsCombCols - 1) / kRmsCombCols), dim3(kThreads), 0, st, q.part, dgamma, D, q.slices);
  BHG_HIP_CHECK(hipGetLastError());
  return BHG_OK;
}

}  // extern "C"
