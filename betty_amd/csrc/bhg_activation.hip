// bhg_activation.hip — the Hessian-vector product's share of a smooth activation, plain or gated, fused into ONE launch.
//
// Where it sits on the path: betty/hypergradient/cg.py:39-41 / neumann.py:62 take H p as the DOUBLE BACKWARD
// `torch.autograd.grad(in_grad, params, grad_outputs=p)`.  ATen differentiates an activation's backward by decomposition: 5 (tanh) to 37
// (tanh-approximated GELU) element-wise launches per activation and product, each rereading and rewriting activation-sized tensors.
//
// Plain activation y = f(x).  The first backward is the map F : (x, gy) -> gx = gy * f'(x); for a cotangent a of gx
//     dgy = a * f'(x)            dx = a * gy * f''(x)
// Gated activation y = f(u) * v (SwiGLU, GeGLU; F.glu with f = sigmoid, v the FIRST half of the input and u the second).  The first
// backward is F : (u, v, gy) -> (gu, gv) = (gy f'(u) v, gy f(u)); for cotangents au of gu and av of gv (either may be absent)
//     dgy = au f'(u) v + av f(u)        du = au gy f''(u) v + av gy f'(u)        dv = au gy f'(u)
// (float64 restatement and its check against autograd: tests/activation_ref.py.)
//
// Kinds, with phi / Phi the standard normal density / distribution and sg the logistic function:
//   gelu       f' = Phi + x phi                 f'' = phi (2 - x^2)
//   gelu_tanh  w = k (x + c x^3), t = tanh w, s = sech^2 w:  f = x (1 + t) / 2,  f' = (1 + t) / 2 + x s w' / 2,
//              f'' = s w' + x (s w'' - 2 t s w'^2) / 2
//   silu       p = sg(x), m = sg(-x):  f = x p,  f' = p (1 + x m),  f'' = p m (2 + x (m - p))
//   tanh       f' = sech^2 x,  f'' = -2 tanh x sech^2 x
//   sigmoid    f' = p m,  f'' = p m (m - p)
//   softplus   z = beta x:  z > threshold (ATen's linear branch): f' = 1, f'' = 0;  else f' = sg(z), f'' = beta sg(z) sg(-z)
// Nothing is formed by subtraction from one: with e = exp(-|z|) and r = 1 / (1 + e), sg(|z|) = r and sg(-|z|) = e r; with e = exp(-2 |w|),
// tanh |w| = (1 - e) r, sech^2 w = 4 e r r and (1 + tanh w) / 2 = sg(2 w).  Every exp argument is <= 0: nothing overflows.
//
// ONE launch each, 256 threads per workgroup, grid = min(work / 256, 2048 = 256 CUs x 8) and a grid-stride loop whose trip count is a
// function of the arguments alone.  Plain: n contiguous elements in units of one 16-byte vector (the n % 4 tail is the last unit, taken
// element by element by the thread it falls to) or, when a pointer is not 16-byte aligned, of one element.  Gated: element (r, j) of every
// array is ptr + r * ld + j; a row gets tpr threads (a power of two <= 256), 256 / tpr rows sit side by side in a workgroup, a row longer
// than 256 units takes cb = ceil(units / 256) workgroups; a workgroup's (row group, column block) advances by a fixed step per trip, so
// that there is one integer division per thread and launch, none per element.  The kernels are templated on the kind: no instance carries
// another kind's transcendentals.  fp32 arithmetic (-ffp-contract=off), 64-bit indexing, no atomics, no LDS, no workspace: bitwise
// run-to-run deterministic.  x, gy, a read once, dx, dgy written once: 20 bytes per element (gated: 32).
#include "bhg_common.hpp"

#include <initializer_list>

namespace bhg {
namespace {

constexpr long long kActMaxGrid = 2048;          // 256 CUs x 8 workgroups: beyond it the grid-stride loop takes the rest
constexpr long long kActMaxIndex = 1LL << 62;    // element offsets and 4 * offset stay inside 64 bits

struct ActPlan {
  int vec;            // 4: 16-byte accesses; 1: scalar
  long long units;    // ceil(n / vec)
  long long grid;     // workgroups, none empty
  long long iters;    // trips of the grid-stride loop: ceil(units / (grid * 256))
};

struct ActArgs {
  const float* x; const float* gy; const float* a;
  float* dx; float* dgy;          // either may be NULL: not stored
  long long n, units, iters;
  float beta, threshold;          // softplus only
};

struct GatedPlan {
  int vec;              // 4 or 1
  int tpr, ltpr;        // threads per row (a power of two <= 256) and its log2
  int rpb;              // rows side by side in a workgroup: 256 / tpr
  long long hu;         // units per row: H / vec
  long long cb;         // column blocks per row: ceil(hu / tpr) (1 unless tpr == 256)
  long long rgroups;    // ceil(rows / rpb)
  long long work;       // rgroups * cb workgroup-sized pieces
  long long grid, iters;
  long long step_r, step_c;   // grid / cb, grid % cb: how (row group, column block) advance per trip
};

struct GatedArgs {
  const float* u; const float* v; const float* gy; const float* au; const float* av;   // au or av may be NULL (absent), not both
  float* du; float* dv; float* dgy;                                                     // any may be NULL: not stored
  long long ld_u, ld_v, ld_gy, ld_au, ld_av, ld_du, ld_dv, ld_dgy;
  long long rows, H;
  GatedPlan p;
};

__device__ __forceinline__ float act_rcp(const float v) { return __builtin_amdgcn_rcpf(v); }

// sg(z) and sg(-z) without a subtraction from one
__device__ __forceinline__ void act_logistic(const float z, float& p, float& m) {
  const float e = expf(-fabsf(z));
  const float r = act_rcp(1.0f + e);
  const float small = e * r;
  p = z >= 0.0f ? r : small;
  m = z >= 0.0f ? small : r;
}

// f(x), f'(x), f''(x) of kind KIND; what a caller does not use is not computed (everything is inlined).
template <int KIND>
__device__ __forceinline__ void act_derivs(const float x, const float beta, const float threshold, float& f, float& f1, float& f2) {
  if (KIND == BHG_ACT_GELU) {
    const float x2 = fminf(x * x, 3.0e38f);                       // 0 * inf would be NaN in f''
    const float phi = 0.3989422804014327f * expf(-0.5f * x2);
    const float Phi = 0.5f * (1.0f + erff(x * 0.7071067811865476f));
    f = x * Phi;
    f1 = Phi + x * phi;
    f2 = phi * (2.0f - x2);
  } else if (KIND == BHG_ACT_GELU_TANH) {
    constexpr float k = 0.7978845608028654f, c = 0.044715f;
    const float xc = fminf(fmaxf(x, -1.0e4f), 1.0e4f);            // beyond it sech^2 w is 0 in fp32: the same values, and x^3 stays finite
    const float x2 = xc * xc;
    const float w = k * (xc + c * x2 * xc);
    const float wp = k * (1.0f + (3.0f * c) * x2);
    const float wpp = (6.0f * k * c) * xc;
    const float e = expf(-2.0f * fabsf(w));
    const float r = act_rcp(1.0f + e);
    const float ta = (1.0f - e) * r;
    const float t = w >= 0.0f ? ta : -ta;
    const float s = 4.0f * e * r * r;
    const float half1pt = w >= 0.0f ? r : e * r;                  // (1 + tanh w) / 2 = sg(2 w)
    f = x * half1pt;
    f1 = half1pt + 0.5f * xc * s * wp;
    f2 = s * wp + 0.5f * xc * (s * wpp - 2.0f * t * s * wp * wp);
  } else if (KIND == BHG_ACT_SILU) {
    float p, m;
    act_logistic(x, p, m);
    f = x * p;
    f1 = p * (1.0f + x * m);
    f2 = p * m * (2.0f + x * (m - p));
  } else if (KIND == BHG_ACT_TANH) {
    const float e = expf(-2.0f * fabsf(x));
    const float r = act_rcp(1.0f + e);
    const float ta = (1.0f - e) * r;
    const float t = x >= 0.0f ? ta : -ta;
    const float s = 4.0f * e * r * r;
    f = t;
    f1 = s;
    f2 = -2.0f * t * s;
  } else if (KIND == BHG_ACT_SIGMOID) {
    float p, m;
    act_logistic(x, p, m);
    f = p;
    f1 = p * m;
    f2 = p * m * (m - p);
  } else {   // BHG_ACT_SOFTPLUS: only the plain kernel, which does not read f
    const float z = beta * x;
    float p, m;
    act_logistic(z, p, m);
    const bool lin = z > threshold;
    f = x;
    f1 = lin ? 1.0f : p;
    f2 = lin ? 0.0f : beta * p * m;
  }
}

template <int KIND>
__device__ __forceinline__ void act_plain_one(const float x, const float gy, const float a, const float beta, const float threshold,
                                              float& dx, float& dgy) {
  float f, f1, f2;
  act_derivs<KIND>(x, beta, threshold, f, f1, f2);
  dgy = a * f1;
  dx = a * gy * f2;
}

// grid = min(ceil(units / 256), 2048); unit i of trip t: (t * gridDim.x + blockIdx.x) * 256 + threadIdx.x.
template <int KIND, int VEC>
__global__ __launch_bounds__(kThreads) void k_act_vjp(const ActArgs q) {
  const long long stride = (long long)gridDim.x * kThreads;
  long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  for (long long t = 0; t < q.iters; ++t, i += stride) {
    if (i >= q.units) continue;
    const long long e0 = i * VEC;
    if (VEC == 4 && e0 + 4 <= q.n) {
      const float4 x = *reinterpret_cast<const float4*>(q.x + e0);
      const float4 gy = *reinterpret_cast<const float4*>(q.gy + e0);
      const float4 a = *reinterpret_cast<const float4*>(q.a + e0);
      float4 dx, dgy;
      act_plain_one<KIND>(x.x, gy.x, a.x, q.beta, q.threshold, dx.x, dgy.x);
      act_plain_one<KIND>(x.y, gy.y, a.y, q.beta, q.threshold, dx.y, dgy.y);
      act_plain_one<KIND>(x.z, gy.z, a.z, q.beta, q.threshold, dx.z, dgy.z);
      act_plain_one<KIND>(x.w, gy.w, a.w, q.beta, q.threshold, dx.w, dgy.w);
      if (q.dx) *reinterpret_cast<float4*>(q.dx + e0) = dx;
      if (q.dgy) *reinterpret_cast<float4*>(q.dgy + e0) = dgy;
    } else {
      // the scalar instance's element, or the n % 4 tail of the vector instance: at most 3 elements, one thread of the launch
      const long long e1 = e0 + VEC < q.n ? e0 + VEC : q.n;
      for (long long e = e0; e < e1; ++e) {
        float dx, dgy;
        act_plain_one<KIND>(q.x[e], q.gy[e], q.a[e], q.beta, q.threshold, dx, dgy);
        if (q.dx) q.dx[e] = dx;
        if (q.dgy) q.dgy[e] = dgy;
      }
    }
  }
}

template <int KIND>
__device__ __forceinline__ void act_gated_one(const float u, const float v, const float gy, const float au, const float av, float& du,
                                              float& dv, float& dgy) {
  float f, f1, f2;
  act_derivs<KIND>(u, 0.0f, 0.0f, f, f1, f2);
  const float g1 = gy * f1;
  dgy = au * f1 * v + av * f;
  du = au * gy * f2 * v + av * g1;
  dv = au * g1;
}

template <int VEC>
__device__ __forceinline__ void act_load(const float* __restrict__ p, float* v) {
  if (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = p[0];
  }
}
template <int VEC>
__device__ __forceinline__ void act_store(float* __restrict__ p, const float* v) {
  if (VEC == 4)
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else
    p[0] = v[0];
}

// Workgroup piece w = (row group rg, column block c), w = rg * cb + c; trip t takes piece t * gridDim.x + blockIdx.x: (rg, c) advance by
// (step_r, step_c) with one carry.  Thread tid: row rg * rpb + (tid >> ltpr), unit c * tpr + (tid & (tpr - 1)) of the row.
template <int KIND, int VEC>
__global__ __launch_bounds__(kThreads) void k_gated_act_vjp(const GatedArgs q) {
  const GatedPlan& p = q.p;
  long long rg = (long long)blockIdx.x / p.cb;
  long long c = (long long)blockIdx.x - rg * p.cb;
  const int lr = (int)threadIdx.x >> p.ltpr, lt = (int)threadIdx.x & (p.tpr - 1);
  const bool has_au = q.au != nullptr, has_av = q.av != nullptr;
  for (long long t = 0; t < p.iters; ++t) {
    const long long r = rg * p.rpb + lr;
    const long long j = (c * p.tpr + lt) * VEC;
    if (rg < p.rgroups && r < q.rows && j < q.H) {   // j + VEC <= H: the vector instance runs only when H % 4 == 0
      float u[VEC], v[VEC], gy[VEC], au[VEC], av[VEC], du[VEC], dv[VEC], dgy[VEC];
      act_load<VEC>(q.u + r * q.ld_u + j, u);
      act_load<VEC>(q.v + r * q.ld_v + j, v);
      act_load<VEC>(q.gy + r * q.ld_gy + j, gy);
      if (has_au) {
        act_load<VEC>(q.au + r * q.ld_au + j, au);
      } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) au[e] = 0.0f;
      }
      if (has_av) {
        act_load<VEC>(q.av + r * q.ld_av + j, av);
      } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) av[e] = 0.0f;
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) act_gated_one<KIND>(u[e], v[e], gy[e], au[e], av[e], du[e], dv[e], dgy[e]);
      if (q.du) act_store<VEC>(q.du + r * q.ld_du + j, du);
      if (q.dv) act_store<VEC>(q.dv + r * q.ld_dv + j, dv);
      if (q.dgy) act_store<VEC>(q.dgy + r * q.ld_dgy + j, dgy);
    }
    rg += p.step_r;
    c += p.step_c;
    if (c >= p.cb) { c -= p.cb; ++rg; }
  }
}

inline const char* act_plan(ActPlan* p, long long n, int aligned16) {
  if (!(n > 0)) return "empty tensor (n must be positive)";
  if (n > kActMaxIndex) return "more than 2^62 elements: beyond what a 64-bit byte offset holds";
  p->vec = aligned16 ? 4 : 1;
  p->units = (n + p->vec - 1) / p->vec;
  const long long groups = (p->units + kThreads - 1) / kThreads;
  p->grid = groups < kActMaxGrid ? groups : kActMaxGrid;
  p->iters = (groups + p->grid - 1) / p->grid;
  return nullptr;
}

inline const char* gated_plan(GatedPlan* p, long long rows, long long H, int vec_ok) {
  if (!(rows > 0 && H > 0)) return "empty tensor (rows and H must be positive)";
  if (rows > kActMaxIndex / H) return "rows * ld beyond 2^62: beyond what a 64-bit byte offset holds";
  p->vec = (vec_ok && H % 4 == 0) ? 4 : 1;
  p->hu = H / p->vec;
  int tpr = 1, ltpr = 0;
  while (tpr < kThreads && tpr < p->hu) { tpr <<= 1; ++ltpr; }
  p->tpr = tpr; p->ltpr = ltpr;
  p->rpb = kThreads / tpr;
  p->cb = (p->hu + tpr - 1) / tpr;
  p->rgroups = (rows + p->rpb - 1) / p->rpb;
  p->work = p->rgroups * p->cb;   // <= rows * H
  p->grid = p->work < kActMaxGrid ? p->work : kActMaxGrid;
  p->iters = (p->work + p->grid - 1) / p->grid;
  p->step_r = p->grid / p->cb;
  p->step_c = p->grid % p->cb;
  return nullptr;
}

inline bool act_aligned16(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (((uintptr_t)p & 15) != 0) return false;   // NULL counts as aligned
  return true;
}

inline const char* act_kind_name(int kind) {
  switch (kind) {
    case BHG_ACT_GELU: return "gelu";
    case BHG_ACT_GELU_TANH: return "gelu_tanh";
    case BHG_ACT_SILU: return "silu";
    case BHG_ACT_TANH: return "tanh";
    case BHG_ACT_SIGMOID: return "sigmoid";
    case BHG_ACT_SOFTPLUS: return "softplus";
    default: return nullptr;
  }
}

template <int KIND>
inline void act_launch(const ActArgs& q, const ActPlan& p, hipStream_t st) {
  if (p.vec == 4) hipLaunchKernelGGL((k_act_vjp<KIND, 4>), dim3((unsigned)p.grid), dim3(kThreads), 0, st, q);
  else hipLaunchKernelGGL((k_act_vjp<KIND, 1>), dim3((unsigned)p.grid), dim3(kThreads), 0, st, q);
}

template <int KIND>
inline void gated_launch(const GatedArgs& q, hipStream_t st) {
  if (q.p.vec == 4) hipLaunchKernelGGL((k_gated_act_vjp<KIND, 4>), dim3((unsigned)q.p.grid), dim3(kThreads), 0, st, q);
  else hipLaunchKernelGGL((k_gated_act_vjp<KIND, 1>), dim3((unsigned)q.p.grid), dim3(kThreads), 0, st, q);
}

}  // namespace
}  // namespace bhg

using namespace bhg;

extern "C" {

int bhg_act_plan(long long n, int aligned16, char* buf, size_t buf_bytes) {
  BHG_REQUIRE(buf && buf_bytes > 0, "NULL buffer");
  ActPlan p{};
  const char* bad = act_plan(&p, n, aligned16);
  BHG_REQUIRE(!bad, bad);
  const int len = snprintf(buf, buf_bytes, "vec=%d block=%d grid=%lld iters=%lld units=%lld inst=%s", p.vec, kThreads, p.grid, p.iters, p.units,
                           p.vec == 4 ? "k_act_vjp<kind,4>" : "k_act_vjp<kind,1>");
  BHG_REQUIRE(len > 0 && (size_t)len < buf_bytes, "buffer too small for the plan line");
  return BHG_OK;
}

int bhg_act_backward_vjp(int kind, float beta, float threshold, const float* x, const float* gy, const float* a, float* dx, float* dgy,
                         long long n, void* stream) {
  BHG_REQUIRE(act_kind_name(kind), "unknown kind");
  BHG_REQUIRE(x && gy && a, "null pointer (x, gy and a are required)");
  BHG_REQUIRE(dx || dgy, "no output wanted (dx and dgy are both NULL)");
  ActPlan p{};
  const char* bad = act_plan(&p, n, act_aligned16({x, gy, a, dx, dgy}) ? 1 : 0);
  BHG_REQUIRE(!bad, bad);
  ActArgs q{};
  q.x = x; q.gy = gy; q.a = a; q.dx = dx; q.dgy = dgy;
  q.n = n; q.units = p.units; q.iters = p.iters; q.beta = beta; q.threshold = threshold;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (kind) {
    case BHG_ACT_GELU: act_launch<BHG_ACT_GELU>(q, p, st); break;
    case BHG_ACT_GELU_TANH: act_launch<BHG_ACT_GELU_TANH>(q, p, st); break;
    case BHG_ACT_SILU: act_launch<BHG_ACT_SILU>(q, p, st); break;
    case BHG_ACT_TANH: act_launch<BHG_ACT_TANH>(q, p, st); break;
    case BHG_ACT_SIGMOID: act_launch<BHG_ACT_SIGMOID>(q, p, st); break;
    default: act_launch<BHG_ACT_SOFTPLUS>(q, p, st); break;
  }
  BHG_HIP_CHECK(hipGetLastError());
  return BHG_OK;
}

int bhg_gated_act_plan(long long rows, long long H, int vec_ok, char* buf, size_t buf_bytes) {
  BHG_REQUIRE(buf && buf_bytes > 0, "NULL buffer");
  GatedPlan p{};
  const char* bad = gated_plan(&p, rows, H, vec_ok);
  BHG_REQUIRE(!bad, bad);
  const int len = snprintf(buf, buf_bytes, "vec=%d block=%d grid=%lld iters=%lld tpr=%d rows=%d cb=%lld rgroups=%lld work=%lld inst=%s", p.vec,
                           kThreads, p.grid, p.iters, p.tpr, p.rpb, p.cb, p.rgroups, p.work,
                           p.vec == 4 ? "k_gated_act_vjp<kind,4>" : "k_gated_act_vjp<kind,1>");
  BHG_REQUIRE(len > 0 && (size_t)len < buf_bytes, "buffer too small for the plan line");
  return BHG_OK;
}

int bhg_gated_act_backward_vjp(int kind, long long rows, long long H, const float* u, long long ld_u, const float* v, long long ld_v,
                               const float* gy, long long ld_gy, const float* au, long long ld_au, const float* av, long long ld_av, float* du,
                               long long ld_du, float* dv, long long ld_dv, float* dgy, long long ld_dgy, void* stream) {
  BHG_REQUIRE(act_kind_name(kind), "unknown kind");
  BHG_REQUIRE(kind != BHG_ACT_SOFTPLUS, "softplus has no gated form");
  BHG_REQUIRE(rows > 0 && H > 0, "empty tensor (rows and H must be positive)");
  BHG_REQUIRE(u && v && gy, "null pointer (u, v and gy are required)");
  BHG_REQUIRE(au || av, "no cotangent (au and av are both NULL)");
  BHG_REQUIRE(du || dv || dgy, "no output wanted (du, dv and dgy are all NULL)");
  long long max_ld = H;
  bool ld4 = true;
  const struct { const void* p; long long ld; } arrays[] = {{u, ld_u}, {v, ld_v}, {gy, ld_gy}, {au, ld_au}, {av, ld_av},
                                                           {du, ld_du}, {dv, ld_dv}, {dgy, ld_dgy}};
  for (const auto& t : arrays) {
    if (!t.p) continue;
    BHG_REQUIRE(t.ld >= H, "a leading dimension is smaller than H");
    if (t.ld > max_ld) max_ld = t.ld;
    if (t.ld % 4 != 0) ld4 = false;
  }
  BHG_REQUIRE(rows <= kActMaxIndex / max_ld, "rows * ld beyond 2^62: beyond what a 64-bit byte offset holds");
  GatedArgs q{};
  const char* bad = gated_plan(&q.p, rows, H, (ld4 && act_aligned16({u, v, gy, au, av, du, dv, dgy})) ? 1 : 0);
  BHG_REQUIRE(!bad, bad);
  q.u = u; q.v = v; q.gy = gy; q.au = au; q.av = av; q.du = du; q.dv = dv; q.dgy = dgy;
  q.ld_u = ld_u; q.ld_v = ld_v; q.ld_gy = ld_gy; q.ld_au = ld_au; q.ld_av = ld_av; q.ld_du = ld_du; q.ld_dv = ld_dv; q.ld_dgy = ld_dgy;
  q.rows = rows; q.H = H;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (kind) {
    case BHG_ACT_GELU: gated_launch<BHG_ACT_GELU>(q, st); break;
    case BHG_ACT_GELU_TANH: gated_launch<BHG_ACT_GELU_TANH>(q, st); break;
    case BHG_ACT_SILU: gated_launch<BHG_ACT_SILU>(q, st); break;
    case BHG_ACT_TANH: gated_launch<BHG_ACT_TANH>(q, st); break;
    default: gated_launch<BHG_ACT_SIGMOID>(q, st); break;
  }
  BHG_HIP_CHECK(hipGetLastError());
  return BHG_OK;
}

}  // extern "C"
