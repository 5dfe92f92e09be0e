// bhg_mlp_tail.hip — the closing launch of the LAST iteration of a fused CG solve without a solution vector (k_t2_dots).  See
// bhg_mlp_tail.hpp for the identity.  A translation unit of its own: the code object of bhg_mlp.o stays as the placement sweep
// measured it (tests/test_code_placement.py).
//
// k_t2_dots: per layer, T2_l = 2 sum_{m < B, n} Gb_l[m][n] Rh_{l-1}[m][n] in fp64.  Both arrays are row-major [RA][RB], so the rows
// < B are ONE contiguous run of B RB floats: a layer is a flat dot product over B RB / 4 float4 — rows >= B are never addressed.
//   partition   layer i owns the workgroups [wg0_i, wg0_i + nwg_i) (the host's table; proportional to the layers' sizes, at most
//               kT2DotsMaxWgs in all); workgroup j of a layer takes the float4 [j per, (j + 1) per), per = ceil(n4 / nwg)
//   order       a thread adds its float4 in index order (dot4: ((x + y) + z) + w), then lanes (wave_sum), then waves 0 .. 3: fixed,
//               so two runs give the same bits.  Every product of two floats is exact in fp64; only the sums round.
//   loads       kT2U = 2 float4 of either array per thread and round (clamped to the workgroup's last float4, added only where live):
//               four 16-byte loads back to back, and only then the first wait — the loaded registers pass through an empty asm statement, so no
//               use of a value can be scheduled ahead of the last load.  One round covers 512 float4 per workgroup: at 256
//               workgroups every shape up to 131072 float4 (the benchmark's: 89600, ~350 per workgroup) is one round trip to memory
//   slots       workgroup j writes slot j of its layer; the slots no workgroup owns (j + nwg, j + 2 nwg, ... < slots) are cleared
//               by the same workgroups — the step length sums every slot of every layer
// No atomics, no polling, 32 bytes of LDS (the reduction).
#include "bhg_mlp_tail.hpp"

namespace bhg {
namespace {

constexpr int kT2U = 2;
struct T2Prob {
  const float* gb; const float* rh; double* part;
  int n4, slots, wg0, nwg;
};
struct T2Args {
  T2Prob p[BHG_MLP_MAX_LAYERS];
  int n;
};

__global__ __launch_bounds__(kThreads) void k_t2_dots(const T2Args g) {
  int i = 0;
  while (i + 1 < g.n && (int)blockIdx.x >= g.p[i + 1].wg0) ++i;
  const T2Prob q = g.p[i];
  const int j = (int)blockIdx.x - q.wg0;
  const int per = (q.n4 + q.nwg - 1) / q.nwg;
  const int c0 = j * per;
  const int c1 = c0 + per < q.n4 ? c0 + per : q.n4;   // (c1 <= c0: a workgroup without a share stores its zero)
  const float4* __restrict__ ga = reinterpret_cast<const float4*>(q.gb);
  const float4* __restrict__ gr = reinterpret_cast<const float4*>(q.rh);
  double acc = 0.0;
  for (int b = c0 + (int)threadIdx.x; b < c1; b += kThreads * kT2U) {
    float4 va[kT2U], vr[kT2U];
#pragma unroll
    for (int u = 0; u < kT2U; ++u) {
      const int idx = b + kThreads * u;
      int at = idx < c1 ? idx : c1 - 1;
      // (the index is opaque to the compiler: knowing where it came from, hipcc puts each load behind the branch of its add below —
      //  a round trip per load instead of one for all of them)
      asm volatile("" : "+v"(at));
      va[u] = ga[at];
      vr[u] = gr[at];
    }
    // every loaded register is an operand here: all four loads are issued above it, the waits and the arithmetic below
    static_assert(kT2U == 2, "the operand list below names two float4 of either array");
    asm volatile("" : "+v"(va[0].x), "+v"(va[0].y), "+v"(va[0].z), "+v"(va[0].w), "+v"(vr[0].x), "+v"(vr[0].y), "+v"(vr[0].z), "+v"(vr[0].w),
                      "+v"(va[1].x), "+v"(va[1].y), "+v"(va[1].z), "+v"(va[1].w), "+v"(vr[1].x), "+v"(vr[1].y), "+v"(vr[1].z), "+v"(vr[1].w));
#pragma unroll
    for (int u = 0; u < kT2U; ++u)
      if (b + kThreads * u < c1) acc += dot4(va[u], vr[u]);
  }
  __shared__ double red[kWaves];
  const double s = block_sum(acc, red);
  if (threadIdx.x == 0) q.part[j] = 2.0 * s;
  for (int z = j + q.nwg * (1 + (int)threadIdx.x); z < q.slots; z += q.nwg * kThreads) q.part[z] = 0.0;
}

}  // namespace

int launch_t2_dots(const T2DotsLaunch& a, hipStream_t st) {
  BHG_REQUIRE(a.n >= 1 && a.n <= BHG_MLP_MAX_LAYERS && a.partT2 && a.B >= 1, "bad arguments");
  T2Args g{};
  int64_t total = 0;
  for (int i = 0; i < a.n; ++i) {
    BHG_REQUIRE(a.gb[i] && a.rh[i] && (((uintptr_t)a.gb[i] | (uintptr_t)a.rh[i]) & 15) == 0, "operands must be 16-byte aligned device pointers");
    BHG_REQUIRE(a.RA[i] >= 32 && a.RA[i] % 32 == 0 && a.RB[i] >= 32 && a.RB[i] % 32 == 0 && a.B <= a.RA[i] && a.t2_off[i] >= 0,
                "rows and widths are multiples of 32, B <= RA");
    const int64_t n4 = (int64_t)a.B * (a.RB[i] / 4);
    BHG_REQUIRE(n4 < ((int64_t)1 << 30), "a layer of the dot products is too large for 32-bit float4 indices");
    total += n4;
  }
  // one workgroup per layer, the rest in proportion to the layers' sizes; none beyond a layer's slots or without 256 float4 of its own
  const int spare = kT2DotsMaxWgs - a.n;
  int wgs = 0;
  for (int i = 0; i < a.n; ++i) {
    T2Prob& q = g.p[i];
    q.gb = a.gb[i]; q.rh = a.rh[i]; q.part = a.partT2 + a.t2_off[i];
    q.n4 = (int)((int64_t)a.B * (a.RB[i] / 4));
    q.slots = (a.RA[i] / 32) * (a.RB[i] / 32);
    int nwg = 1 + (int)((int64_t)spare * q.n4 / total);
    const int useful = (q.n4 + kThreads - 1) / kThreads;
    if (nwg > useful) nwg = useful;
    if (nwg > q.slots) nwg = q.slots;
    q.nwg = nwg; q.wg0 = wgs;
    wgs += nwg;
  }
  g.n = a.n;
  BHG_REQUIRE(wgs >= 1 && wgs <= kT2DotsMaxWgs, "internal: workgroup table");
  hipLaunchKernelGGL(k_t2_dots, dim3(wgs), dim3(kThreads), 0, st, g);
  BHG_HIP_CHECK(hipGetLastError());
  return BHG_OK;
}

}  // namespace bhg

using namespace bhg;

extern "C" int bhg_mlp_t2_dots(int n, const float* const* gb, const float* const* rh, const int* RA, const int* RB, int B,
                               double* partT2, const int* t2_off, void* stream) {
  BHG_REQUIRE(n >= 1 && n <= BHG_MLP_MAX_LAYERS && gb && rh && RA && RB && t2_off, "bad arguments");
  T2DotsLaunch a{};
  a.n = n; a.B = B; a.partT2 = partT2;
  for (int i = 0; i < n; ++i) { a.gb[i] = gb[i]; a.rh[i] = rh[i]; a.RA[i] = RA[i]; a.RB[i] = RB[i]; a.t2_off[i] = t2_off[i]; }
  return launch_t2_dots(a, static_cast<hipStream_t>(stream));
}
