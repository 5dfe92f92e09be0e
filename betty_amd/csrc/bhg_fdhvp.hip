// bhg_fdhvp.hip — the weight side of the finite-difference Hessian-vector product (gfx950 only).
//
// hypergradient/_common.py: FiniteDifferenceHVP takes H p from two first-order gradients,
//     H p ~= ( grad L(w + eps p) - grad L(w - eps p) ) / (2 eps),
// K times per solve.  The live inner weights are perturbed FROM A FLAT SNAPSHOT w0 taken once per solve (bhg_flatten),
//     w_t <- w0_t + (sign * eps) * p_t,
// not by in-place +eps, -2 eps, +eps steps: K iterations of in-place axpys would let the weights drift by K roundings, here every
// perturbed point is one rounding away from its exact value and the solve ends with bhg_scatter(w0) — the weights come back bit
// for bit.  The product's consumers (bhg_cg_step_fd / bhg_neumann_step_fd) live with the recurrences in bhg_vector.hip.
//
// One streaming pass, 12*N bytes (read w0, p; write w), 16-byte accesses, chunked like k_axpy_multi; eps is read from device
// memory (bhg_darts_eps writes it: no host synchronisation); the product is rounded before the add, like ATen's separate ops.
#include "bhg_common.hpp"

namespace bhg {
namespace {

__global__ __launch_bounds__(kThreads) void k_fd_perturb(PtrTab w, const float* __restrict__ w0, PtrTab dir,
                                                         const bhg_chunk* __restrict__ chunks, int n_chunks,
                                                         const float* __restrict__ eps_dev, float sign) {
  const float a = mul_rn(sign, *eps_dev);
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const bhg_chunk ck = chunks[c];
    float* d = tab_ptr(w, ck.tensor) + ck.src_off;
    const float* s = tab_ptr(dir, ck.tensor) + ck.src_off;
    const float* b = w0 + ck.flat_off;
    float4 bv[kVecPerThread], sv[kVecPerThread];
#pragma unroll
    for (int i = 0; i < kVecPerThread; ++i) {
      const int e = 4 * (threadIdx.x + kThreads * i);
      bv[i] = ld4(b, e, ck.len);
      sv[i] = ld4(s, e, ck.len);
    }
#pragma unroll
    for (int i = 0; i < kVecPerThread; ++i) {
      const int e = 4 * (threadIdx.x + kThreads * i);
      st4(d, e, ck.len, add_scaled4(bv[i], a, sv[i]));
    }
  }
}

}  // namespace
}  // namespace bhg

using namespace bhg;

extern "C" int bhg_fd_perturb(void* const* w, const float* w0_flat, const void* const* dir, int T, const bhg_chunk* chunks_dev,
                              int n_chunks, const float* eps_dev, float sign, void* ws, void* stream) {
  BHG_REQUIRE((w != nullptr && dir != nullptr) || T == 0, "tensor table is NULL");
  BHG_REQUIRE(T >= 0 && n_chunks >= 0, "negative size");
  BHG_REQUIRE(chunks_dev != nullptr || n_chunks == 0, "chunk table is NULL");
  if (n_chunks == 0) return BHG_OK;
  BHG_REQUIRE(w0_flat, "snapshot is NULL");
  BHG_REQUIRE(eps_dev, "eps is NULL");
  hipStream_t st = static_cast<hipStream_t>(stream);
  PtrTab tw, td;
  if (int rc = make_table(&tw, const_cast<const void* const*>(w), T, ws, 0, st)) return rc;
  if (int rc = make_table(&td, dir, T, ws, 1, st)) return rc;
  const int grid = n_chunks < kMaxBlocks ? n_chunks : kMaxBlocks;
  hipLaunchKernelGGL(k_fd_perturb, dim3(grid), dim3(kThreads), 0, st, tw, w0_flat, td, chunks_dev, n_chunks, eps_dev, sign);
  BHG_HIP_CHECK(hipGetLastError());
  return BHG_OK;
}
