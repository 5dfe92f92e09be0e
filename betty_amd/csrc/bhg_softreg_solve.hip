// bhg_softreg_solve.hip — the whole CG / Neumann solve of softmax regression with a per-weight L2 penalty in native launches: the
// multi-class sibling of bhg_logreg_solve.hip.
//
//   W, lam, V : [C, d] row-major (the flat vector is W row-major, N = C d),  X : [n, d],  P = softmax(X W^T) (row maximum subtracted)
//   H V = U^T X + lam .* V,   Z = X V^T,   U = (P .* Z - P .* rowsum(P .* Z)) / n         (the labels drop out of the Hessian)
//
// Who runs the K loop (cg.py:38-56, neumann.py:59-66 of the reference):
//   single : ONE launch of ONE workgroup — the direction and the product in LDS, x / r / lam / W in registers, X re-read from cache
//            per iteration, the final scaling and coeff inside the launch (C d <= 4096 and n d <= 2^18);
//   strips : G workgroups own contiguous row strips and write a [G][C d] partial; small follow-up launches sum the partials in strip
//            order in fp64, add lam .* V and apply the recurrences (3 launches per CG iteration, 2 per Neumann iteration).
// Both forms use ONE device body for the pass over X (pass_rows), on the fp32 matrix cores (v_mfma_f32_16x16x4_f32, exact fp32):
//   phase 1  a wave owns a 16-row tile, classes padded to 16: Z and the logits X W^T accumulate over k = d (two MFMAs per k-step of 4);
//   phase 2  the tile's P and U in registers — a softmax row lives in one 16-lane row of the wave, padded classes are masked out of
//            the maximum, the sum and U; the U of rows past the strip is written as zero;  U -> LDS;
//   phase 3  U^T X: the waves split the COLUMNS (64 per wave and slot), k = the 256 rows of the workgroup's super-tile; this second
//            read of the X tile hits cache — HBM sees X once per product — as long as the live super-tiles of all workgroups
//            (256 rows x d each) fit the Infinity Cache (they do not at 65536 x 3072).  The accumulators stay in
//            registers across super-tiles and each wave stores its own columns: no combine step.
// P is recomputed by every product (not stored per solve): the logits ride on the X operand phase 1 loads anyway, at the price of
// four more MFMAs per 16 x 16 block of X (12 instead of 8: DESIGN.md has the measured consequence).
//
// Sums meet in a fixed order everywhere (MFMA k order, strips in strip order in fp64, dots in fp64 in a fixed tree): results are
// bitwise run-to-run deterministic; no float atomics, no workgroup waits on another inside a launch, every loop is bounded by its
// arguments, and nothing is read from the workspace that the same solve has not written.
//
// The sample-weighted sibling (bhg_wsoftreg_*: one weight a_i per row of X, a constant penalty `reg` in lam's place) runs the same
// solver: its pass scales a row of U by a_i before the division by n (pass_rows<.., kPassWeighted>, kernels of their own: the
// unweighted kernels' device code does not know about the weight), everything after the pass is shared.  k_wsoftreg_mixed is the
// one pass over X of its mixed second derivative: phase 1 and the softmax of phase 2, a per-row epilogue, no phase 3.
//
// Arithmetic of the recurrences: oracle/recurrence.c / tests/recurrence_ref.py (products rounded to fp32 before add / sub, fp64 dots,
// fp32 quotients, den = dot(fl(cg_alpha Hp), p) but r -= alpha Hp with the un-scaled Hp, no breakdown guard, out_scale folded
// into the last iteration).
#include <float.h>

#include "bhg_linear_solve.hpp"

namespace bhg {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kT = 1024;                      // threads of the pass, the single form and the CG update
constexpr int kW = kT / 64;                   // 16 waves
constexpr int kTile = 16;                     // rows of a wave's tile = padded classes
constexpr int kSuper = kW * kTile;            // rows of a workgroup's super-tile
constexpr int kMaxC = 16;
constexpr int kMaxD = 4096;
constexpr int kMaxN = 32768;                  // C d
constexpr int kSlots = kMaxD / (64 * kW);     // 64-column chunks a wave owns in phase 3 ...
constexpr int kSingleMaxN = 4096;
constexpr int64_t kSingleMaxElems = (int64_t)1 << 18;
constexpr int kSinglePer = kSingleMaxN / kT;  // state elements per thread of the single form
constexpr int kSingleSlots = kSingleMaxN / 2 / (64 * kW);   // ... and in the single form: C >= 2, so d <= kSingleMaxN / 2
constexpr int kAutoRowsPerStrip = 64;
constexpr size_t kAutoPartBytes = (size_t)16 << 20;   // auto: G N floats stay under this
constexpr int kMaxColBlocks = kMaxN / kColBlock;
constexpr size_t kWsVec = 8192;               // byte offset of the vectors of the workspace (strips_ws), past the den partials
static_assert(kSlots * 64 * kW == kMaxD && kSingleSlots * 64 * kW * 2 == kSingleMaxN, "the waves' column chunks cover the widest row");
static_assert(kMaxColBlocks <= kT, "the CG update sums the den partials one per thread");
static_assert(kWsDen + 8 * kMaxColBlocks <= kWsVec, "the den partials end before the vectors of the workspace");

// ---- the pass over X -------------------------------------------------------------------------------------------------
// Four consecutive floats of a row from column c, zero from column `d` on.  VEC: one 16-byte load (d % 4 == 0 and 16-byte aligned
// rows: c < d implies c + 3 < d); else scalar loads (row starts are unaligned).  d = 0 reads nothing.
template <bool VEC>
__device__ __forceinline__ float4 ld4g(const float* p, const int c, const int d) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if constexpr (VEC) {
    if (c < d) v = *reinterpret_cast<const float4*>(p + c);
  } else {
    if (c < d) v.x = p[c];
    if (c + 1 < d) v.y = p[c + 1];
    if (c + 2 < d) v.z = p[c + 2];
    if (c + 3 < d) v.w = p[c + 3];
  }
  return v;
}

__device__ __forceinline__ f32x4 mfma4(const float a, const float b, const f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// over the 16 lanes of a row of the wave; the result is in every lane of the row, the same bits
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_mov_f32<0xB1>(v);
  v += dpp_mov_f32<0x4E>(v);
  v += dpp_mov_f32<0x141>(v);
  v += dpp_mov_f32<0x140>(v);
  return v;
}
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, dpp_mov_f32<0xB1>(v));
  v = fmaxf(v, dpp_mov_f32<0x4E>(v));
  v = fmaxf(v, dpp_mov_f32<0x141>(v));
  v = fmaxf(v, dpp_mov_f32<0x140>(v));
  return v;
}

// acc += U^T X over the rows [row0, row1) for the columns this wave owns.  Every thread of the kT-thread workgroup calls it with the
// same arguments.  W, dir: [C, d] (global or LDS).  sU: kSuper * 16 floats of LDS.  nf = (float)n of the WHOLE problem.
// MODE (rw is read in the modes that name it only):
//   kPassPlain     the product above;
//   kPassWeighted  row i of U is scaled by rw.a[i] (the weight of the sample, indexed like the rows of X) before the division by n;
//                  loaded in phase 2, once per row;
//   kPassMixed     phases 1 and 2 only, for ONE super-tile [row0, row1): instead of U, lane q = 0 of row i stores
//                  rw.c[i] = sum_c (P_ic - [c == rw.y[i]]) Z_ic / n; sU and acc are not touched.
// Operand maps of the 16x16x4 MFMA: lane l gives A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15], and holds
// D[i = 4 (l >> 4) + reg][j = l & 15].  A k-step may take its four k's in any order as long as A and B agree, so a lane feeds the
// four components of ONE 16-byte load to four consecutive MFMAs.
//   phase 1: A = X[row q][k], B = V[class q][k] | W[class q][k]  -> lane holds Z | logits [row 4 g + reg][class q]
//   phase 3: A = U[row 4 t + g][class q] (LDS), B = X[row 4 t + g][col 4 q + e] into accumulator e
//            -> acc[slot][e][reg] = (U^T X)[class 4 g + reg][col 64 chunk + 4 q + e]
enum { kPassPlain = 0, kPassWeighted = 1, kPassMixed = 2 };
struct RowArgs {
  const float* a;        // kPassWeighted: n sample weights
  const long long* y;    // kPassMixed: n labels
  float* c;              // kPassMixed: n cotangents
};
template <bool VEC, int SLOTS, int MODE>
__device__ __forceinline__ void pass_rows(const float* __restrict__ X, const float* W, const float* dir, const RowArgs rw, float* sU,
                                          const int d, const int C, const int row0, const int row1, const float nf,
                                          f32x4 (&acc)[SLOTS][4]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, q = lane & 15;
#pragma unroll
  for (int s = 0; s < SLOTS; ++s)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[s][e] = f32x4{0.f, 0.f, 0.f, 0.f};
  // Lanes without an operand of their own read a neighbour's, so that the loads of the main loops are unconditional (several in
  // flight): a padded class reads class 0 and is masked out of the softmax (its P and U are zero whatever Z it got), a row past the
  // strip reads the strip's last row and its U is written as zero, a column past d (phase 3, VEC) reads the row's last four and lands
  // in accumulator columns store_acc drops.
  const bool cls = q < C;
  const float* wq = W + (cls ? q * d : 0);
  const float* vq = dir + (cls ? q * d : 0);
  const int dmain = VEC ? d & ~15 : 0;          // phase 1: columns whose 16-byte k-steps load unconditionally
  for (int st = row0; st < row1; st += kSuper) {
    const int live = row1 - st < kSuper ? row1 - st : kSuper;
    const int t0 = wave * kTile;
    const float* xs = X + (int64_t)st * d;       // the super-tile's first row: one 64-bit base for the whole workgroup
    if (t0 < live) {
      const int i = t0 + q;                       // (row offsets inside a super-tile fit 32 bits: kSuper * kMaxD floats)
      const float* xr = xs + (i < live ? i : live - 1) * d;
      f32x4 az = {0.f, 0.f, 0.f, 0.f}, al = {0.f, 0.f, 0.f, 0.f};
      int k0 = 0;
      if (dmain > 0) {                            // X two k-steps ahead of its MFMAs (V and W come from cache, X from HBM)
        float4 a = *reinterpret_cast<const float4*>(xr + 4 * g);
        float4 a1 = *reinterpret_cast<const float4*>(xr + (16 < dmain ? 16 : 0) + 4 * g);
        for (; k0 < dmain; k0 += 16) {
          const int c = k0 + 4 * g;
          const int kn = k0 + 32 < dmain ? k0 + 32 : dmain - 16;   // (the last steps re-read the last block: unused)
          const float4 a2 = *reinterpret_cast<const float4*>(xr + kn + 4 * g);
          const float4 v = *reinterpret_cast<const float4*>(vq + c), w = *reinterpret_cast<const float4*>(wq + c);
          az = mfma4(a.x, v.x, az); al = mfma4(a.x, w.x, al);
          az = mfma4(a.y, v.y, az); al = mfma4(a.y, w.y, al);
          az = mfma4(a.z, v.z, az); al = mfma4(a.z, w.z, al);
          az = mfma4(a.w, v.w, az); al = mfma4(a.w, w.w, al);
          a = a1;
          a1 = a2;
        }
      }
      for (; k0 < d; k0 += 16) {
        const int c = k0 + 4 * g;
        const float4 a = ld4g<VEC>(xr, c, d), v = ld4g<VEC>(vq, c, d), w = ld4g<VEC>(wq, c, d);
        az = mfma4(a.x, v.x, az); al = mfma4(a.x, w.x, al);
        az = mfma4(a.y, v.y, az); al = mfma4(a.y, w.y, al);
        az = mfma4(a.z, v.z, az); al = mfma4(a.z, w.z, al);
        az = mfma4(a.w, v.w, az); al = mfma4(a.w, w.w, al);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float lg = cls ? al[r] : -FLT_MAX;
        const float m = row16_max(lg);
        const float e = cls ? expf(lg - m) : 0.f;
        const float p = e / row16_sum(e);
        if constexpr (MODE == kPassMixed) {
          // the epilogue of the mixed second derivative: one lane per row stores c; a label outside [0, C) matches no class
          const int row = st + t0 + 4 * g + r;
          const long long yi = row < row1 ? rw.y[row] : -1;
          const float t = row16_sum(cls ? (p - ((long long)q == yi ? 1.f : 0.f)) * az[r] : 0.f);
          if (row < row1 && q == 0) rw.c[row] = t / nf;
        } else {
          const float pz = p * az[r];
          const float t = row16_sum(pz);
          if constexpr (MODE == kPassWeighted) {
            const int row = st + t0 + 4 * g + r;
            const float ai = row < row1 ? rw.a[row] : 0.f;
            sU[(t0 + 4 * g + r) * 16 + q] = row < row1 ? ((pz - p * t) * ai) / nf : 0.f;
          } else {
            sU[(t0 + 4 * g + r) * 16 + q] = st + t0 + 4 * g + r < row1 ? (pz - p * t) / nf : 0.f;
          }
        }
      }
    }
    if constexpr (MODE == kPassMixed) return;     // (one super-tile per workgroup, no phase 3)
    __syncthreads();
    const int rows4 = (live + 3) & ~3;          // (rows past `live` up to here belong to a live tile: their U is zero)
    const int rows8 = VEC ? live & ~7 : 0;      // phase 3: rows taken two unconditional 16-byte k-steps at a time
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int c = (wave + kW * s) * 64 + 4 * q;
      if ((wave + kW * s) * 64 < d) {
        const int cc = !VEC || c + 4 <= d ? c : d - 4;   // (used by VEC only: d % 4 == 0, so d >= 4)
        const float* up = sU + g * 16 + q;
        int R = 0;
        for (; R < rows8; R += 8) {
          const int o = (R + g) * d + cc;
          const float4 b0 = *reinterpret_cast<const float4*>(xs + o), b1 = *reinterpret_cast<const float4*>(xs + o + 4 * d);
          const float a0 = up[R * 16], a1 = up[(R + 4) * 16];
          acc[s][0] = mfma4(a0, b0.x, acc[s][0]); acc[s][1] = mfma4(a0, b0.y, acc[s][1]);
          acc[s][2] = mfma4(a0, b0.z, acc[s][2]); acc[s][3] = mfma4(a0, b0.w, acc[s][3]);
          acc[s][0] = mfma4(a1, b1.x, acc[s][0]); acc[s][1] = mfma4(a1, b1.y, acc[s][1]);
          acc[s][2] = mfma4(a1, b1.z, acc[s][2]); acc[s][3] = mfma4(a1, b1.w, acc[s][3]);
        }
        for (; R < rows4; R += 4) {
          const int i = R + g;
          const float4 b = ld4g<VEC>(xs + (i < live ? i : live - 1) * d, c, d);
          const float a = up[R * 16];
          acc[s][0] = mfma4(a, b.x, acc[s][0]);
          acc[s][1] = mfma4(a, b.y, acc[s][1]);
          acc[s][2] = mfma4(a, b.z, acc[s][2]);
          acc[s][3] = mfma4(a, b.w, acc[s][3]);
        }
      }
    }
    __syncthreads();                            // sU is rewritten by the next super-tile
  }
}

// dst[class][col] = acc for the real classes and columns this wave owns (dst: [C, d], global or LDS)
template <bool VEC, int SLOTS>
__device__ __forceinline__ void store_acc(float* dst, const int d, const int C, const f32x4 (&acc)[SLOTS][4]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, q = lane & 15;
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int c = (wave + kW * s) * 64 + 4 * q;
    if (c >= d) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = 4 * g + r;
      if (k >= C) continue;
      float* o = dst + k * d + c;
      if constexpr (VEC) {
        *reinterpret_cast<float4*>(o) = make_float4(acc[s][0][r], acc[s][1][r], acc[s][2][r], acc[s][3][r]);
      } else {
        o[0] = acc[s][0][r];
        if (c + 1 < d) o[1] = acc[s][1][r];
        if (c + 2 < d) o[2] = acc[s][2][r];
        if (c + 3 < d) o[3] = acc[s][3][r];
      }
    }
  }
}

// ---- single: the whole solve in one workgroup ---------------------------------------------------------------------------------
// CG: x, r in registers, sdir = p.  Neumann: sdir = v (the direction), x = the accumulator p.  `a`: cg_alpha | alpha.  A thread owns
// the flat elements {tid, tid + kT, ...}.
// The body of both single kernels.  sdir, sh: kSingleMaxN floats of LDS each, sU: kSuper * 16, sred: kW doubles.  ROWW: `aw` holds one
// weight per row of X (pass_rows).
template <bool VEC, bool ROWW>
__device__ __forceinline__ void single_body(const float* __restrict__ X, const float* __restrict__ W, const float* __restrict__ lam,
                                            const float* __restrict__ aw, const float* __restrict__ rhs, float* __restrict__ out,
                                            float* __restrict__ coeff, const int n, const int d, const int C, const int K, const int cg,
                                            const float a, const float out_scale, float* sdir, float* sh, float* sU, double* sred) {
  const int tid = threadIdx.x, N = C * d;
  float wv[kSinglePer], lv[kSinglePer], xv[kSinglePer], rv[kSinglePer];
#pragma unroll
  for (int u = 0; u < kSinglePer; ++u) {
    const int j = tid + kT * u;
    const bool in = j < N;
    const float r0 = in ? rhs[j] : 0.f;
    wv[u] = in ? W[j] : 0.f;
    lv[u] = in ? lam[j] : 0.f;
    sdir[j] = r0;
    rv[u] = r0;
    xv[u] = cg ? 0.f : r0;
  }
  __syncthreads();
  double rr = 0.0;
  if (cg) {
#pragma unroll
    for (int u = 0; u < kSinglePer; ++u) rr += (double)rv[u] * (double)rv[u];
    rr = block_sum_w<kW>(rr, sred);
  }
  const float nf = (float)n;
  for (int k = 0; k < K; ++k) {
    f32x4 acc[kSingleSlots][4];
    pass_rows<VEC, kSingleSlots, ROWW ? kPassWeighted : kPassPlain>(X, W, sdir, RowArgs{aw, nullptr, nullptr}, sU, d, C, 0, n, nf, acc);
    store_acc<VEC, kSingleSlots>(sh, d, C, acc);
    __syncthreads();
    // from here every thread touches its own elements only
    if (cg) {
      float hp[kSinglePer];
      double den = 0.0;
#pragma unroll
      for (int u = 0; u < kSinglePer; ++u) {
        const int j = tid + kT * u;
        const float pj = j < N ? sdir[j] : 0.f;
        const float lp = lv[u] * pj;
        hp[u] = (j < N ? sh[j] : 0.f) + lp;
        const float ahp = a * hp[u];
        den += (double)ahp * (double)pj;
      }
      den = block_sum_w<kW>(den, sred);
      const float alpha = (float)rr / (float)den;
      double rn2 = 0.0;
#pragma unroll
      for (int u = 0; u < kSinglePer; ++u) {
        const float t = alpha * hp[u];
        rv[u] = rv[u] - t;
        rn2 += (double)rv[u] * (double)rv[u];
      }
      rn2 = block_sum_w<kW>(rn2, sred);
      const float beta = (float)rn2 / (float)rr;
#pragma unroll
      for (int u = 0; u < kSinglePer; ++u) {
        const int j = tid + kT * u;
        if (j < N) {
          const float pj = sdir[j];
          const float ap = alpha * pj;
          xv[u] = xv[u] + ap;
          const float bp = beta * pj;
          sdir[j] = rv[u] + bp;
        }
      }
      rr = rn2;
    } else {
#pragma unroll
      for (int u = 0; u < kSinglePer; ++u) {
        const int j = tid + kT * u;
        if (j < N) {
          const float vj = sdir[j];
          const float lp = lv[u] * vj;
          const float hv = sh[j] + lp;
          const float t = a * hv;
          const float vn = vj - t;
          sdir[j] = vn;
          xv[u] = vn + xv[u];
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < kSinglePer; ++u) {
    const int j = tid + kT * u;
    if (j < N) {
      float o = xv[u];
      if (out_scale != 0.f) o = out_scale * o;
      out[j] = o;
      if (coeff) coeff[j] = wv[u] * o;
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(kT) void k_softreg_single(const float* __restrict__ X, const float* __restrict__ W,
                                                       const float* __restrict__ lam, const float* __restrict__ rhs,
                                                       float* __restrict__ out, float* __restrict__ coeff, const int n, const int d,
                                                       const int C, const int K, const int cg, const float a, const float out_scale) {
  __shared__ __align__(16) float sdir[kSingleMaxN], sh[kSingleMaxN], sU[kSuper * 16];
  __shared__ double sred[kW];
  single_body<VEC, false>(X, W, lam, nullptr, rhs, out, coeff, n, d, C, K, cg, a, out_scale, sdir, sh, sU, sred);
}

// the sample-weighted problem: aw[n], `reg` in lam's place, no coeff (its cotangent is k_wsoftreg_mixed's)
template <bool VEC>
__global__ __launch_bounds__(kT) void k_wsoftreg_single(const float* __restrict__ X, const float* __restrict__ W,
                                                        const float* __restrict__ reg, const float* __restrict__ aw,
                                                        const float* __restrict__ rhs, float* __restrict__ out, const int n, const int d,
                                                        const int C, const int K, const int cg, const float a, const float out_scale) {
  __shared__ __align__(16) float sdir[kSingleMaxN], sh[kSingleMaxN], sU[kSuper * 16];
  __shared__ double sred[kW];
  single_body<VEC, true>(X, W, reg, aw, rhs, out, nullptr, n, d, C, K, cg, a, out_scale, sdir, sh, sU, sred);
}

// ---- strips ----------------------------------------------------------------------------------------------------------------------
// Launch 1 of an iteration: workgroup b sums its rows [b rps, (b + 1) rps) into part[b][0..N); an empty strip writes zeros.
template <bool VEC>
__global__ __launch_bounds__(kT) void k_softreg_strip_pass(const float* __restrict__ X, const float* __restrict__ W,
                                                           const float* __restrict__ dir, float* __restrict__ part, const int n,
                                                           const int d, const int C, const int rps) {
  __shared__ float sU[kSuper * 16];
  const int64_t lo = (int64_t)blockIdx.x * rps, hi = lo + rps;
  const int row0 = (int)(lo < n ? lo : n), row1 = (int)(hi < n ? hi : n);
  f32x4 acc[kSlots][4];
  pass_rows<VEC, kSlots, kPassPlain>(X, W, dir, RowArgs{nullptr, nullptr, nullptr}, sU, d, C, row0, row1, (float)n, acc);
  store_acc<VEC, kSlots>(part + (int64_t)blockIdx.x * C * d, d, C, acc);
}

// ... of the sample-weighted problem: aw[n], indexed like the rows of X
template <bool VEC>
__global__ __launch_bounds__(kT) void k_wsoftreg_strip_pass(const float* __restrict__ X, const float* __restrict__ W,
                                                            const float* __restrict__ dir, const float* __restrict__ aw,
                                                            float* __restrict__ part, const int n, const int d, const int C,
                                                            const int rps) {
  __shared__ float sU[kSuper * 16];
  const int64_t lo = (int64_t)blockIdx.x * rps, hi = lo + rps;
  const int row0 = (int)(lo < n ? lo : n), row1 = (int)(hi < n ? hi : n);
  f32x4 acc[kSlots][4];
  pass_rows<VEC, kSlots, kPassWeighted>(X, W, dir, RowArgs{aw, nullptr, nullptr}, sU, d, C, row0, row1, (float)n, acc);
  store_acc<VEC, kSlots>(part + (int64_t)blockIdx.x * C * d, d, C, acc);
}

// ---- the mixed second derivative of the sample-weighted problem -------------------------------------------------------------------
// c_i = sum_c (P_ic - [c == y_i]) Z_ic / n with Z = X dir^T: the cotangent of the weight a_i along `dir`.  Workgroup b owns the 256 rows
// of super-tile b, a wave a 16-row tile: phase 1 and the softmax of pass_rows (kPassMixed), then lane q = 0 of each row stores its c.
// Nothing is combined across waves or workgroups; rows past n store nothing; a label outside [0, C) matches no class.
template <bool VEC>
__global__ __launch_bounds__(kT) void k_wsoftreg_mixed(const float* __restrict__ X, const float* __restrict__ W,
                                                       const float* __restrict__ dir, const long long* __restrict__ y,
                                                       float* __restrict__ c, const int n, const int d, const int C) {
  const int st = blockIdx.x * kSuper;           // (the grid is ceil(n / kSuper) workgroups: st < n <= 2^30)
  f32x4 acc[1][4];
  pass_rows<VEC, 1, kPassMixed>(X, W, dir, RowArgs{nullptr, y, c}, nullptr, d, C, st, n - st < kSuper ? n : st + kSuper, (float)n, acc);
}

// The launches after the pass: thin wrappers of the shared bodies (bhg_linear_solve.hpp), N = C d; the sample-weighted problem runs
// them too.  The CG update takes the den partials one per thread through block_sum_w.
__global__ __launch_bounds__(kColBlock) void k_softreg_strip_hp(const float* __restrict__ part, const int G,
                                                                const float* __restrict__ lam, const float* __restrict__ p,
                                                                float* __restrict__ Hp, double* __restrict__ denpart, const int N,
                                                                const float cg_alpha) {
  strip_hp_body(part, G, lam, p, Hp, denpart, N, cg_alpha);
}

__global__ __launch_bounds__(kT) void k_softreg_strip_cg_update(const float* __restrict__ rhs, const float* __restrict__ W,
                                                                const float* __restrict__ Hp, const double* __restrict__ denpart,
                                                                const int nden, double* __restrict__ rr_slot, float* __restrict__ x,
                                                                float* __restrict__ r, float* __restrict__ p, float* __restrict__ out,
                                                                float* __restrict__ coeff, const int N, const int k, const int last,
                                                                const float out_scale) {
  strip_cg_update_body<kT, false>(rhs, W, Hp, denpart, nden, rr_slot, x, r, p, out, coeff, N, k, last, out_scale);
}

__global__ __launch_bounds__(kColBlock) void k_softreg_strip_neumann_update(const float* __restrict__ part, const int G,
                                                                            const float* __restrict__ lam, const float* __restrict__ W,
                                                                            const float* vin, const float* pin, float* v, float* p,
                                                                            float* __restrict__ out, float* __restrict__ coeff, const int N,
                                                                            const float alpha, const int last, const float out_scale) {
  strip_neumann_update_body(part, G, lam, W, vin, pin, v, p, out, coeff, N, alpha, last, out_scale);
}

__global__ __launch_bounds__(kThreads) void k_softreg_solve_k0(const float* __restrict__ rhs, const float* __restrict__ W,
                                                               float* __restrict__ out, float* __restrict__ coeff, const int N,
                                                               const int cg, const float out_scale) {
  solve_k0_body(rhs, W, out, coeff, N, cg, out_scale);
}

const StripKernels kStripKernels = {k_softreg_strip_hp, k_softreg_strip_cg_update, kT, k_softreg_strip_neumann_update};

// ---- host ------------------------------------------------------------------------------------------------------------------------
bool family_admits(int d, int C) { return C >= 2 && C <= kMaxC && d >= 1 && d <= kMaxD && (int64_t)C * d <= kMaxN; }
bool single_admits(int n, int d, int C) {
  return family_admits(d, C) && C * d <= kSingleMaxN && (int64_t)n * d <= kSingleMaxElems;
}

// auto: kAutoRowsPerStrip rows per strip, as many strips as the partial buffer's cap and kMaxStrips allow
int auto_strips(int n, int d, int C) {
  int64_t want = ((int64_t)n + kAutoRowsPerStrip - 1) / kAutoRowsPerStrip;
  const int64_t cap = (int64_t)(kAutoPartBytes / (sizeof(float) * (size_t)C * (size_t)d));
  if (want > cap) want = cap;
  if (want > kMaxStrips) want = kMaxStrips;
  return (int)(want < 1 ? 1 : want);
}

// BHG_OK and the plan, or BHG_ERR_ARG with the error set (a forced form the shape does not admit is an error, not a fallback)
int make_plan(const char* fn, int n, int d, int C, int form, int strips, Plan* out) {
  int f;
  const int rc = plan_form(fn, n <= 0 || d <= 0 || C <= 0, n, form, strips, single_admits(n, d, C), family_admits(d, C), &f);
  if (rc != BHG_OK) return rc;
  if (f == kFormSingle && !single_admits(n, d, C)) {
    set_error("%s: the single form takes 2 <= C <= %d, C * d <= %d and n * d <= %lld", fn, kMaxC, kSingleMaxN, (long long)kSingleMaxElems);
    return BHG_ERR_ARG;
  }
  if (f == kFormStrips && !family_admits(d, C)) {
    set_error("%s: the strips form takes 2 <= C <= %d, d <= %d and C * d <= %d", fn, kMaxC, kMaxD, kMaxN);
    return BHG_ERR_ARG;
  }
  *out = plan_of(f, n, strips, f == kFormStrips ? auto_strips(n, d, C) : 0);
  return BHG_OK;
}

// aw: the row weights of the sample-weighted problem (then lam is its `reg` and coeff is not written), or NULL
void launch_single(hipStream_t st, const float* X, const float* W, const float* lam, const float* aw, const float* rhs, float* out,
                   float* coeff, int n, int d, int C, int K, int cg, float a, float out_scale, bool vec) {
  if (aw && vec)
    hipLaunchKernelGGL((k_wsoftreg_single<true>), dim3(1), dim3(kT), 0, st, X, W, lam, aw, rhs, out, n, d, C, K, cg, a, out_scale);
  else if (aw)
    hipLaunchKernelGGL((k_wsoftreg_single<false>), dim3(1), dim3(kT), 0, st, X, W, lam, aw, rhs, out, n, d, C, K, cg, a, out_scale);
  else if (vec)
    hipLaunchKernelGGL((k_softreg_single<true>), dim3(1), dim3(kT), 0, st, X, W, lam, rhs, out, coeff, n, d, C, K, cg, a, out_scale);
  else
    hipLaunchKernelGGL((k_softreg_single<false>), dim3(1), dim3(kT), 0, st, X, W, lam, rhs, out, coeff, n, d, C, K, cg, a, out_scale);
}

void launch_pass(hipStream_t st, const Plan& pl, const float* X, const float* W, const float* dir, const float* aw, float* part, int n,
                 int d, int C, bool vec) {
  if (aw && vec)
    hipLaunchKernelGGL((k_wsoftreg_strip_pass<true>), dim3(pl.G), dim3(kT), 0, st, X, W, dir, aw, part, n, d, C, pl.rps);
  else if (aw)
    hipLaunchKernelGGL((k_wsoftreg_strip_pass<false>), dim3(pl.G), dim3(kT), 0, st, X, W, dir, aw, part, n, d, C, pl.rps);
  else if (vec)
    hipLaunchKernelGGL((k_softreg_strip_pass<true>), dim3(pl.G), dim3(kT), 0, st, X, W, dir, part, n, d, C, pl.rps);
  else
    hipLaunchKernelGGL((k_softreg_strip_pass<false>), dim3(pl.G), dim3(kT), 0, st, X, W, dir, part, n, d, C, pl.rps);
}

template <bool CG>
int solve(const char* fn, const float* X, const float* W, const float* lam, const float* aw, const float* rhs, float* out, float* coeff,
          void* ws, int n, int d, int C, int K, float a, float out_scale, int form, int strips, void* stream) {
  if (!(X && W && lam && rhs && out && ws)) { set_error("%s: NULL pointer", fn); return BHG_ERR_ARG; }
  if (K < 0) { set_error("%s: negative iteration count", fn); return BHG_ERR_ARG; }
  Plan pl;
  const int rc = make_plan(fn, n, d, C, form, strips, &pl);
  if (rc != BHG_OK) return rc;
  if (pl.form == kFormNone) {
    set_error("%s: no native form takes C = %d, d = %d (2 <= C <= %d, d <= %d, C * d <= %d)", fn, C, d, kMaxC, kMaxD, kMaxN);
    return BHG_ERR_ARG;
  }
  if (((uintptr_t)ws & 15) != 0) { set_error("%s: the workspace must be 16-byte aligned", fn); return BHG_ERR_ARG; }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int N = C * d;
  if (K == 0) {
    hipLaunchKernelGGL(k_softreg_solve_k0, dim3((N + kThreads - 1) / kThreads), dim3(kThreads), 0, st, rhs, W, out, coeff, N, CG ? 1 : 0,
                       out_scale);
    BHG_HIP_CHECK(hipGetLastError());
    return BHG_OK;
  }
  // else row starts (of X, W or the direction) are unaligned: the scalar path
  const bool vec = d % 4 == 0 && (((uintptr_t)X | (uintptr_t)W | (uintptr_t)rhs) & 15) == 0;
  if (pl.form == kFormSingle) {
    launch_single(st, X, W, lam, aw, rhs, out, coeff, n, d, C, K, CG ? 1 : 0, a, out_scale, vec);
    BHG_HIP_CHECK(hipGetLastError());
    return BHG_OK;
  }
  run_strips<CG>(st, kStripKernels, strips_ws(ws, kWsVec, N), pl.G,
                 [&](const float* dir, float* part) { launch_pass(st, pl, X, W, dir, aw, part, n, d, C, vec); }, lam, W, rhs, out, coeff, N,
                 K, a, out_scale);
  BHG_HIP_CHECK(hipGetLastError());
  return BHG_OK;
}

}  // namespace
}  // namespace bhg

using namespace bhg;

extern "C" {

int bhg_softreg_solve_plan(int n, int d, int C, int form, int strips, char* buf, size_t buf_bytes) {
  BHG_REQUIRE(buf && buf_bytes > 0, "NULL buffer");
  Plan pl;
  const int rc = make_plan(__func__, n, d, C, form, strips, &pl);
  if (rc != BHG_OK) return rc;
  plan_line(pl, buf, buf_bytes);
  return BHG_OK;
}

size_t bhg_softreg_solve_ws_bytes(int n, int d, int C) {
  if (n <= 0 || !family_admits(d, C)) return 0;
  return strips_ws(nullptr, kWsVec, (size_t)C * d).bytes;
}

int bhg_softreg_cg_solve(const float* X, const float* W, const float* lam, const float* rhs, float* out, float* coeff, void* ws, int n,
                         int d, int C, int K, float cg_alpha, float out_scale, int form, int strips, void* stream) {
  return solve<true>(__func__, X, W, lam, nullptr, rhs, out, coeff, ws, n, d, C, K, cg_alpha, out_scale, form, strips, stream);
}

int bhg_softreg_neumann_solve(const float* X, const float* W, const float* lam, const float* rhs, float* out, float* coeff, void* ws, int n,
                              int d, int C, int K, float alpha, float out_scale, int form, int strips, void* stream) {
  return solve<false>(__func__, X, W, lam, nullptr, rhs, out, coeff, ws, n, d, C, K, alpha, out_scale, form, strips, stream);
}

// The sample-weighted problem: plan, family and workspace are bhg_softreg_solve_plan's / bhg_softreg_solve_ws_bytes'.
int bhg_wsoftreg_cg_solve(const float* X, const float* W, const float* reg, const float* a, const float* rhs, float* out, void* ws, int n,
                          int d, int C, int K, float cg_alpha, float out_scale, int form, int strips, void* stream) {
  BHG_REQUIRE(a, "NULL pointer");
  return solve<true>(__func__, X, W, reg, a, rhs, out, nullptr, ws, n, d, C, K, cg_alpha, out_scale, form, strips, stream);
}

int bhg_wsoftreg_neumann_solve(const float* X, const float* W, const float* reg, const float* a, const float* rhs, float* out, void* ws,
                               int n, int d, int C, int K, float alpha, float out_scale, int form, int strips, void* stream) {
  BHG_REQUIRE(a, "NULL pointer");
  return solve<false>(__func__, X, W, reg, a, rhs, out, nullptr, ws, n, d, C, K, alpha, out_scale, form, strips, stream);
}

int bhg_wsoftreg_mixed(const float* X, const float* W, const float* dir, const int64_t* y, float* c, int n, int d, int C, void* stream) {
  BHG_REQUIRE(X && W && dir && y && c, "NULL pointer");
  BHG_REQUIRE(n > 0 && d > 0 && C > 0, "empty problem");
  BHG_REQUIRE(n <= (1 << 30), "more than 2^30 rows");
  if (!family_admits(d, C)) {
    set_error("%s: no native form takes C = %d, d = %d (2 <= C <= %d, d <= %d, C * d <= %d)", __func__, C, d, kMaxC, kMaxD, kMaxN);
    return BHG_ERR_ARG;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool vec = d % 4 == 0 && (((uintptr_t)X | (uintptr_t)W | (uintptr_t)dir) & 15) == 0;
  const dim3 grid((n + kSuper - 1) / kSuper);
  const long long* yy = reinterpret_cast<const long long*>(y);
  if (vec)
    hipLaunchKernelGGL((k_wsoftreg_mixed<true>), grid, dim3(kT), 0, st, X, W, dir, yy, c, n, d, C);
  else
    hipLaunchKernelGGL((k_wsoftreg_mixed<false>), grid, dim3(kT), 0, st, X, W, dir, yy, c, n, d, C);
  BHG_HIP_CHECK(hipGetLastError());
  return BHG_OK;
}

}  // extern "C"
