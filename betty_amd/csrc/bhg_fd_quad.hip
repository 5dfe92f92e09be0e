// bhg_fd_quad.hip — the central finite difference (darts, SAMA) of an inner loss whose upper parameters enter only through a
// term QUADRATIC in the inner weights, in closed form: one streaming pass, no forward pass of the network.
//
// betty/hypergradient/darts.py:37-67 (sama.py:25-59 alike) perturbs the live inner weights with three in-place axpys,
// w+ = w + eps v, w- = w+ - 2 eps v, w = w- + eps v (skipped under *_multitask), differentiates the user's training_step at w+ and
// w- to the upper parameters and returns (g- - g+) / (2 eps).  For two declared structures g depends on w affinely or
// quadratically and the difference has no truncation error:
//   mode 0, proximal (implicit MAML):  L = data(w) + reg ||w - theta||^2,  g(w) = dL/dtheta = -2 reg (w - theta),
//           (g- - g+) / (2 eps) = 2 reg (w+ - w-) / (2 eps) = 2 reg v                  -> out = scale * v, scale = 2 reg;
//   mode 1, logistic + L2:  L = mean BCE + 1/2 sum_j lam_j w_j^2,  g(w) = dL/dlam = w^2 / 2,
//           (g- - g+) / (2 eps) = (w- - w+)(w- + w+) / (4 eps) = -w v  (w+ + w- = 2 w) -> out = -(w * v), w the UNPERTURBED weight.
// What the hop still owes the caller is the weights the three axpys leave behind, rounding for rounding: per element
// w1 = fl(w + fl(a1 v)), w2 = fl(w1 + fl(a2 v)), w3 = fl(w2 + fl(a1 v)) with a1 = fl(1 * eps), a2 = fl(-2 * eps) as k_axpy_multi
// (bhg_vector.hip) forms them; w <- w3, or w2 when restore == 0.
//
// Traffic: read w and v, write w and out = 16 N bytes (20 N when accumulating into out), against the opaque hop's three axpys
// (36 N) plus the norm's pass over v (4 N) — the 40 N of darts.py's vector work — plus two forward and two backward passes of the
// network.  No atomics, no LDS, no reduction: every element is owned by one thread, so the result is deterministic.
// A translation unit of its own, linked after bhg_fd.o: the K-loop kernels of bhg_mlp.hip keep their anchored code placement.
#include <math.h>

#include "bhg_common.hpp"

namespace bhg {
namespace {

constexpr int kQuadT = 128;   // tensors per launch: three inline tables of 128 pointers = 3 KiB of kernel arguments, no table writes

struct QuadTab {
  float* w[kQuadT];         // live inner weights (read, overwritten)
  const float* v[kQuadT];   // direction
  float* o[kQuadT];         // result
};

// One element: the weight the three axpys of darts.py:37-63 leave behind (k_axpy_multi's roundings), and the closed-form result.
template <int MODE, bool ACC>
__device__ __forceinline__ void quad_elem(float w, float v, float o_old, float a1, float a2, float scale, int restore, float& w_new,
                                          float& o_new) {
  const float w1 = add_rn(w, mul_rn(a1, v));
  const float w2 = add_rn(w1, mul_rn(a2, v));
  w_new = restore ? add_rn(w2, mul_rn(a1, v)) : w2;
  const float r = MODE == 0 ? mul_rn(scale, v) : -mul_rn(w, v);
  o_new = ACC ? add_rn(o_old, r) : r;
}

// grid = grid_for(n_chunks) workgroups striding over the chunk table; block = 256.  Tensors [t0, t0 + kQuadT) of the layout are this
// launch's; chunks of other tensors are skipped (T > kQuadT takes several launches).
template <int MODE, bool ACC>
__global__ __launch_bounds__(kThreads) void k_quad_fd(QuadTab tab, int t0, const bhg_chunk* __restrict__ chunks, int n_chunks,
                                                      const float* __restrict__ eps_dev, float scale, int restore) {
  const float eps = *eps_dev;
  const float a1 = mul_rn(1.f, eps), a2 = mul_rn(-2.f, eps);
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const bhg_chunk ck = chunks[c];
    const int t = ck.tensor - t0;
    if (t < 0 || t >= kQuadT) continue;
    float* w = tab.w[t] + ck.src_off;
    const float* v = tab.v[t] + ck.src_off;
    float* o = tab.o[t] + ck.src_off;
    int len = ck.len;
    // Chunks start a multiple of 4096 elements into their tensor, so a chunk is 16-byte aligned exactly when the tensor is.  The
    // three tensors of a chunk that share one misalignment get a scalar head up to the next 16-byte boundary and the vector body
    // from there; three different misalignments (no common boundary) take the scalar loop for the whole chunk.
    const unsigned mw = (unsigned)((uintptr_t)w & 15u), mv = (unsigned)((uintptr_t)v & 15u), mo = (unsigned)((uintptr_t)o & 15u);
    if ((mw | mv | mo) != 0u) {
      int head = len;
      if (mw == mv && mw == mo) head = min(len, (int)((16u - mw) >> 2));
      for (int e = threadIdx.x; e < head; e += kThreads) {
        float wn, on;
        quad_elem<MODE, ACC>(w[e], v[e], ACC ? o[e] : 0.f, a1, a2, scale, restore, wn, on);
        w[e] = wn;
        o[e] = on;
      }
      w += head; v += head; o += head; len -= head;
      if (len <= 0) continue;
    }
    float4 wv[kVecPerThread], vv[kVecPerThread], ov[kVecPerThread];
#pragma unroll
    for (int i = 0; i < kVecPerThread; ++i) {
      const int e = 4 * (threadIdx.x + kThreads * i);
      wv[i] = ld4(w, e, len);
      vv[i] = ld4(v, e, len);
      ov[i] = ACC ? ld4(o, e, len) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < kVecPerThread; ++i) {
      const int e = 4 * (threadIdx.x + kThreads * i);
      float4 wn, on;
      quad_elem<MODE, ACC>(wv[i].x, vv[i].x, ov[i].x, a1, a2, scale, restore, wn.x, on.x);
      quad_elem<MODE, ACC>(wv[i].y, vv[i].y, ov[i].y, a1, a2, scale, restore, wn.y, on.y);
      quad_elem<MODE, ACC>(wv[i].z, vv[i].z, ov[i].z, a1, a2, scale, restore, wn.z, on.z);
      quad_elem<MODE, ACC>(wv[i].w, vv[i].w, ov[i].w, a1, a2, scale, restore, wn.w, on.w);
      st4(w, e, len, wn);
      st4(o, e, len, on);
    }
  }
}

inline int quad_grid(int n_chunks) { return n_chunks < kMaxBlocks ? (n_chunks > 0 ? n_chunks : 1) : kMaxBlocks; }   // grid_for of bhg_vector.hip

}  // namespace
}  // namespace bhg

using namespace bhg;

extern "C" {

int bhg_quad_fd(void* const* w, const void* const* dir, void* const* out, int T, const bhg_chunk* chunks_dev, int n_chunks,
                const float* eps_dev, float scale, int mode, int restore, int accumulate, void* stream) {
  BHG_REQUIRE(w && dir && out, "tensor table is NULL");
  BHG_REQUIRE(T >= 1, "T must be >= 1");
  BHG_REQUIRE(n_chunks >= 0, "negative chunk count");
  BHG_REQUIRE(chunks_dev != nullptr || n_chunks == 0, "chunk table is NULL");
  BHG_REQUIRE(eps_dev, "eps is NULL");
  BHG_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (proximal) or 1 (logistic)");
  BHG_REQUIRE(isfinite(scale), "scale is not finite");
  for (int i = 0; i < T; ++i) {
    BHG_REQUIRE(w[i] && dir[i] && out[i], "NULL weight, direction or output tensor");
    BHG_REQUIRE((((uintptr_t)w[i] | (uintptr_t)dir[i] | (uintptr_t)out[i]) & 3u) == 0, "tensors must be 4-byte aligned");
  }
  if (n_chunks == 0) return BHG_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(quad_grid(n_chunks)), block(kThreads);
  for (int t0 = 0; t0 < T; t0 += kQuadT) {
    QuadTab tab;
    memset(&tab, 0, sizeof(tab));
    const int cnt = T - t0 < kQuadT ? T - t0 : kQuadT;
    for (int i = 0; i < cnt; ++i) {
      tab.w[i] = static_cast<float*>(w[t0 + i]);
      tab.v[i] = static_cast<const float*>(dir[t0 + i]);
      tab.o[i] = static_cast<float*>(out[t0 + i]);
    }
    if (mode == 0 && !accumulate) hipLaunchKernelGGL((k_quad_fd<0, false>), grid, block, 0, st, tab, t0, chunks_dev, n_chunks, eps_dev, scale, restore);
    else if (mode == 0) hipLaunchKernelGGL((k_quad_fd<0, true>), grid, block, 0, st, tab, t0, chunks_dev, n_chunks, eps_dev, scale, restore);
    else if (!accumulate) hipLaunchKernelGGL((k_quad_fd<1, false>), grid, block, 0, st, tab, t0, chunks_dev, n_chunks, eps_dev, scale, restore);
    else hipLaunchKernelGGL((k_quad_fd<1, true>), grid, block, 0, st, tab, t0, chunks_dev, n_chunks, eps_dev, scale, restore);
  }
  BHG_HIP_CHECK(hipGetLastError());
  return BHG_OK;
}

}  // extern "C"
