// bhg_attention.hip — the Hessian-vector product's share of an attention core, fused, for short sequences.
//
// Where it sits on the path: betty/hypergradient/cg.py:39-41 / neumann.py:62 take H p as the DOUBLE BACKWARD
// `torch.autograd.grad(in_grad, params, grad_outputs=p)`.  The fused SDPA kernels have no double backward, so a transformer inner
// problem runs its attention on the math path and ATen differentiates bmm -> softmax -> bmm by decomposition, per product.
//
// Per (batch, head): Q, gO, aQ are L x d, K, V, aK, aV are S x d, m is an additive L x S mask (not differentiated), s the scale.
//     forward         P = softmax_rows(s Q K^T + m)        O = P V
//     first backward  F : (Q, K, V, gO) -> (gQ, gK, gV)
//         gP = gO V^T      D = rowsum(P * gP)      gS = P * (gP - D)
//         gQ = s gS K      gK = s gS^T Q           gV = P^T gO
// and one Hessian-vector product needs the VECTOR-JACOBIAN product of F: given cotangents aQ, aK, aV of gQ, gK, gV (any may be absent =
// zero), the gradients of <aQ, gQ> + <aK, gK> + <aV, gV> with respect to Q, K, V, gO (float64 restatement and its check against
// autograd: tests/attention_ref.py)
//     T   = s (aQ K^T + Q aK^T)            E = rowsum(P * T)
//     bgP = P * (T - E)
//     bP  = T * (gP - D) - gP * E + gO aV^T
//     bS  = P * (bP - rowsum(P * bP))
//     dgO = bgP V + P aV                   dV = bgP^T gO
//     dQ  = s (bS K + gS aK)               dK = s (bS^T Q + gS^T aQ)
// Twelve small products and four row reductions (five with the softmax denominator).
//
// ONE launch, no workspace: one workgroup of 256 threads per (b, h), everything in the LDS of its CU.  The LDS holds four L x S score
// matrices X0 .. X3 and FOUR operand slots of max(L, S) x d; the seven operand matrices are staged through the slots in five phases:
//     1  Q K gO V   -> slots 0 1 2 3     X0 = Q K^T, X1 = gO V^T
//     2  aQ aK      -> slots 2 3         X2 = aQ K^T + Q aK^T                              (skipped when both are absent)
//     3  gO aV      -> slots 0 1         X3 = gO aV^T                                      (the product skipped when aV is absent)
//        rows       one wave per row, one lane per column: X0 = P, X1 = gS, X2 = bgP, X3 = bS; the five row sums in fp64
//     4  V          -> slot 2            dV = X2^T gO, dgO = X2 V + X0 aV
//     5  K Q aQ     -> slots 0 1 2       dQ = s (X3 K + X1 aK), dK = s (X3^T Q + X1^T aQ)   (aK is still in slot 3)
// The products are a register-tiled fp32 FMA loop (4 x 4 outputs per thread, explicit fmaf: the compiler contracts nothing,
// -ffp-contract=off); the fp32-input MFMA runs at the packed vector rate on gfx950 and was not built.  No atomics, no grid
// barrier: bitwise run-to-run deterministic.  Every loop is bounded by L, S, d <= 64.
//
// Layout: fp32.  Inputs with four element strides each (batch, head, row, and a last stride that must be 1); outputs contiguous (B, H, L | S, d).
// vec = 4 (16-byte global and LDS accesses) when d % 4 == 0 and every stride of a present input is a multiple of 4; otherwise scalar.
#include "bhg_common.hpp"

#include <math.h>

namespace bhg {
namespace {

constexpr int kAtMax = 64;                 // L, S, d <= 64
constexpr int kAtSlots = 4, kAtPhases = 5;
constexpr int kAtMaxLds = 160 * 1024;      // what one workgroup may take on gfx950
enum { AT_Q = 0, AT_K, AT_V, AT_GO, AT_AQ, AT_AK, AT_AV, AT_IN };
enum { AT_DQ = 0, AT_DK, AT_DV, AT_DGO, AT_OUT };

struct AtArgs {
  const float* in[AT_IN];      // q k v go aq ak av; the last three may be NULL
  long long st[AT_IN][3];      // element strides: batch, head, row
  const float* mask;           // may be NULL
  long long mst[4];            // element strides of the mask: batch, head, row, column (0 = broadcast)
  float* out[AT_OUT];          // dq dk dv dgo, contiguous; each may be NULL
  int B, H, L, S, d;
  int causal;
  float scale;
  int vec;                     // 4: 16-byte accesses; 1: scalar
  int ps, pd;                  // row pitches (floats) of a score matrix and of an operand slot
  int rows;                    // rows of an operand slot: max(L, S)
  int lds;                     // bytes of dynamic LDS
};

// Global -> LDS: `rows` rows of d floats, row stride rs in global memory and `pitch` in the LDS.
template <int VEC>
__device__ __forceinline__ void at_stage(float* __restrict__ dst, const int pitch, const float* __restrict__ src, const long long rs,
                                         const int rows, const int d) {
  const int nv = d / VEC, n = rows * nv;
  for (int idx = threadIdx.x; idx < n; idx += kThreads) {
    const int r = idx / nv, c = (idx - r * nv) * VEC;
    if (VEC == 4)
      *reinterpret_cast<float4*>(dst + r * pitch + c) = *reinterpret_cast<const float4*>(src + r * rs + c);
    else
      dst[r * pitch + c] = src[r * rs + c];
  }
}

// The thread's 4 x 4 outputs.  Rows ty + 16 r everywhere except the transposed product on the vector path (4 ty + r: its four
// rows are ONE 16-byte read of a score row); columns 4 tx + u on the vector path of the output products (one 16-byte access), tx + 16 u
// otherwise.  An index past the matrix is clamped for the reads (a duplicate, computed and dropped) and masked at the store.
__device__ __forceinline__ int at_clamp(const int i, const int n) { return i < n ? i : n - 1; }

// acc[r][c] += sum_k A[ty + 16 r][k] * Bm[tx + 16 c][k]      (L x S outputs, contraction over d; both operands in slots of pitch pd)
template <int VEC>
__device__ __forceinline__ void at_nt(float (&acc)[4][4], const float* __restrict__ A, const float* __restrict__ Bm, const int pd, const int L,
                                      const int S, const int d, const int ty, const int tx) {
  const float* ar[4];
  const float* br[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    ar[r] = A + at_clamp(ty + 16 * r, L) * pd;
    br[r] = Bm + at_clamp(tx + 16 * r, S) * pd;
  }
  if (VEC == 4) {
    for (int k = 0; k < d; k += 4) {
      float4 a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        a[r] = *reinterpret_cast<const float4*>(ar[r] + k);
        b[r] = *reinterpret_cast<const float4*>(br[r] + k);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c)
          acc[r][c] = fmaf(a[r].w, b[c].w, fmaf(a[r].z, b[c].z, fmaf(a[r].y, b[c].y, fmaf(a[r].x, b[c].x, acc[r][c]))));
    }
  } else {
    for (int k = 0; k < d; ++k) {
      float a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        a[r] = ar[r][k];
        b[r] = br[r][k];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = fmaf(a[r], b[c], acc[r][c]);
    }
  }
}

__device__ __forceinline__ void at_store_scores(float* __restrict__ X, const int ps, const float (&acc)[4][4], const int L, const int S,
                                                const int ty, const int tx) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (ty + 16 * r < L && tx + 16 * c < S) X[(ty + 16 * r) * ps + tx + 16 * c] = acc[r][c];
}

// The four columns of row `row` (pitch pd) of an operand slot that this thread's outputs take.
template <int VEC>
__device__ __forceinline__ void at_cols(float (&m)[4], const float* __restrict__ row, const int d, const int tx) {
  if (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(row + (4 * tx < d ? 4 * tx : 0));
    m[0] = t.x; m[1] = t.y; m[2] = t.z; m[3] = t.w;
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) m[u] = row[at_clamp(tx + 16 * u, d)];
  }
}

// acc[r][u] += sum_j X[ty + 16 r][j] * M[j][col u]           (L x d outputs, contraction over the n = S columns of X)
template <int VEC>
__device__ __forceinline__ void at_nn(float (&acc)[4][4], const float* __restrict__ X, const int ps, const float* __restrict__ M, const int pd,
                                      const int L, const int n, const int d, const int ty, const int tx) {
  const float* xr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) xr[r] = X + at_clamp(ty + 16 * r, L) * ps;
  for (int j = 0; j < n; ++j) {
    float m[4], x[4];
    at_cols<VEC>(m, M + j * pd, d, tx);
#pragma unroll
    for (int r = 0; r < 4; ++r) x[r] = xr[r][j];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[r][u] = fmaf(x[r], m[u], acc[r][u]);
  }
}

// Row of the transposed product's output r of this thread.
template <int VEC>
__device__ __forceinline__ int at_tn_row(const int ty, const int r) { return VEC == 4 ? 4 * ty + r : ty + 16 * r; }

// acc[r][u] += sum_i X[i][row r] * M[i][col u]               (S x d outputs, contraction over the n = L rows of X)
// Vector path: ps >= S rounded up to 4, so the 16-byte read of a score row stays inside the row; what it reads past column S only
// reaches outputs that the store masks.
template <int VEC>
__device__ __forceinline__ void at_tn(float (&acc)[4][4], const float* __restrict__ X, const int ps, const float* __restrict__ M, const int pd,
                                      const int S, const int n, const int d, const int ty, const int tx) {
  int xc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) xc[r] = VEC == 4 ? (4 * ty < S ? 4 * ty : 0) + r : at_clamp(ty + 16 * r, S);
  for (int i = 0; i < n; ++i) {
    float m[4], x[4];
    at_cols<VEC>(m, M + i * pd, d, tx);
    if (VEC == 4) {
      const float4 t = *reinterpret_cast<const float4*>(X + i * ps + xc[0]);
      x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) x[r] = X[i * ps + xc[r]];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[r][u] = fmaf(x[r], m[u], acc[r][u]);
  }
}

// out[row][col] = f * acc, rows x d, contiguous.  TN: the rows of the transposed product.
template <int VEC, bool TN>
__device__ __forceinline__ void at_store_out(float* __restrict__ out, const float (&acc)[4][4], const float f, const int rows, const int d,
                                             const int ty, const int tx) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = TN ? at_tn_row<VEC>(ty, r) : ty + 16 * r;
    if (row >= rows) continue;
    if (VEC == 4) {
      if (4 * tx < d)
        *reinterpret_cast<float4*>(out + row * d + 4 * tx) = make_float4(f * acc[r][0], f * acc[r][1], f * acc[r][2], f * acc[r][3]);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (tx + 16 * u < d) out[row * d + tx + 16 * u] = f * acc[r][u];
    }
  }
}

__device__ __forceinline__ void at_zero(float (&acc)[4][4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
}

__device__ __forceinline__ float at_wave_max(float v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
  return v;
}

// grid = B * H, one workgroup per (b, h).
template <int VEC>
__global__ __launch_bounds__(kThreads) void k_attn_vjp(const AtArgs q) {
  extern __shared__ __attribute__((aligned(16))) float at_lds[];
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int L = q.L, S = q.S, d = q.d, ps = q.ps, pd = q.pd;
  const int b = blockIdx.x / q.H, h = blockIdx.x - b * q.H;
  float* const X0 = at_lds;
  float* const X1 = X0 + L * ps;
  float* const X2 = X1 + L * ps;
  float* const X3 = X2 + L * ps;
  float* const slot0 = X3 + L * ps;
  float* const slot1 = slot0 + q.rows * pd;
  float* const slot2 = slot1 + q.rows * pd;
  float* const slot3 = slot2 + q.rows * pd;
  const float* src[AT_IN];
#pragma unroll
  for (int i = 0; i < AT_IN; ++i) src[i] = q.in[i] ? q.in[i] + (b * q.st[i][0] + h * q.st[i][1]) : nullptr;
  const bool has_aq = src[AT_AQ] != nullptr, has_ak = src[AT_AK] != nullptr, has_av = src[AT_AV] != nullptr;
  const bool has_t = has_aq || has_ak;
  float* const dq = q.out[AT_DQ] ? q.out[AT_DQ] + (long long)blockIdx.x * L * d : nullptr;
  float* const dk = q.out[AT_DK] ? q.out[AT_DK] + (long long)blockIdx.x * S * d : nullptr;
  float* const dv = q.out[AT_DV] ? q.out[AT_DV] + (long long)blockIdx.x * S * d : nullptr;
  float* const dgo = q.out[AT_DGO] ? q.out[AT_DGO] + (long long)blockIdx.x * L * d : nullptr;
  float acc[4][4];

  // phase 1: X0 = Q K^T (unscaled), X1 = gP = gO V^T
  at_stage<VEC>(slot0, pd, src[AT_Q], q.st[AT_Q][2], L, d);
  at_stage<VEC>(slot1, pd, src[AT_K], q.st[AT_K][2], S, d);
  at_stage<VEC>(slot2, pd, src[AT_GO], q.st[AT_GO][2], L, d);
  at_stage<VEC>(slot3, pd, src[AT_V], q.st[AT_V][2], S, d);
  __syncthreads();
  at_zero(acc);
  at_nt<VEC>(acc, slot0, slot1, pd, L, S, d, ty, tx);
  at_store_scores(X0, ps, acc, L, S, ty, tx);
  at_zero(acc);
  at_nt<VEC>(acc, slot2, slot3, pd, L, S, d, ty, tx);
  at_store_scores(X1, ps, acc, L, S, ty, tx);
  __syncthreads();

  // phase 2: X2 = aQ K^T + Q aK^T (unscaled)
  if (has_t) {
    if (has_aq) at_stage<VEC>(slot2, pd, src[AT_AQ], q.st[AT_AQ][2], L, d);
    if (has_ak) at_stage<VEC>(slot3, pd, src[AT_AK], q.st[AT_AK][2], S, d);
    __syncthreads();
    at_zero(acc);
    if (has_aq) at_nt<VEC>(acc, slot2, slot1, pd, L, S, d, ty, tx);
    if (has_ak) at_nt<VEC>(acc, slot0, slot3, pd, L, S, d, ty, tx);
    at_store_scores(X2, ps, acc, L, S, ty, tx);
    __syncthreads();
  }

  // phase 3: X3 = gO aV^T
  at_stage<VEC>(slot0, pd, src[AT_GO], q.st[AT_GO][2], L, d);
  if (has_av) at_stage<VEC>(slot1, pd, src[AT_AV], q.st[AT_AV][2], S, d);
  __syncthreads();
  if (has_av) {
    at_zero(acc);
    at_nt<VEC>(acc, slot0, slot1, pd, L, S, d, ty, tx);
    at_store_scores(X3, ps, acc, L, S, ty, tx);
  }
  __syncthreads();

  // rows: one wave per row, lane j = column j (S <= 64).  The softmax denominator and the three row sums in fp64.
  {
    const int lane = tid & 63, wave = tid >> 6;
    const bool in = lane < S;
    const int j = in ? lane : 0;
    const float* mrow = q.mask ? q.mask + (b * q.mst[0] + h * q.mst[1] + j * q.mst[3]) : nullptr;
    for (int i = wave; i < L; i += kWaves) {
      const int at = i * ps + j;
      float sc = q.scale * X0[at];
      if (mrow) sc += mrow[i * q.mst[2]];
      if (!in || (q.causal && j > i)) sc = -INFINITY;
      const float mx = at_wave_max(sc);
      const double e = in ? (double)expf(sc - mx) : 0.0;   // a fully masked row: -inf - -inf, NaN as on the math path
      const double sum = wave_sum(e);
      const float pf = (float)(e / sum);
      const double p = (double)pf;
      const double gp = (double)X1[at];
      const double t = has_t ? (double)(q.scale * X2[at]) : 0.0;
      const double w = has_av ? (double)X3[at] : 0.0;
      const double D = wave_sum(in ? p * gp : 0.0);
      const double E = wave_sum(in ? p * t : 0.0);
      const double bp = t * (gp - D) - gp * E + w;
      const double R = wave_sum(in ? p * bp : 0.0);
      if (in) {
        X0[at] = pf;
        X1[at] = (float)(p * (gp - D));   // gS
        X2[at] = (float)(p * (t - E));    // bgP
        X3[at] = (float)(p * (bp - R));   // bS
      }
    }
  }
  __syncthreads();

  // phase 4: dV = bgP^T gO, dgO = bgP V + P aV     (gO in slot 0, aV in slot 1)
  if (dgo) at_stage<VEC>(slot2, pd, src[AT_V], q.st[AT_V][2], S, d);
  __syncthreads();
  if (dv) {
    at_zero(acc);
    at_tn<VEC>(acc, X2, ps, slot0, pd, S, L, d, ty, tx);
    at_store_out<VEC, true>(dv, acc, 1.f, S, d, ty, tx);
  }
  if (dgo) {
    at_zero(acc);
    at_nn<VEC>(acc, X2, ps, slot2, pd, L, S, d, ty, tx);
    if (has_av) at_nn<VEC>(acc, X0, ps, slot1, pd, L, S, d, ty, tx);
    at_store_out<VEC, false>(dgo, acc, 1.f, L, d, ty, tx);
  }
  if (!dq && !dk) return;   // uniform over the workgroup
  __syncthreads();

  // phase 5: dQ = s (bS K + gS aK), dK = s (bS^T Q + gS^T aQ)     (aK still in slot 3)
  if (dq) at_stage<VEC>(slot0, pd, src[AT_K], q.st[AT_K][2], S, d);
  if (dk) {
    at_stage<VEC>(slot1, pd, src[AT_Q], q.st[AT_Q][2], L, d);
    if (has_aq) at_stage<VEC>(slot2, pd, src[AT_AQ], q.st[AT_AQ][2], L, d);
  }
  __syncthreads();
  if (dq) {
    at_zero(acc);
    at_nn<VEC>(acc, X3, ps, slot0, pd, L, S, d, ty, tx);
    if (has_ak) at_nn<VEC>(acc, X1, ps, slot3, pd, L, S, d, ty, tx);
    at_store_out<VEC, false>(dq, acc, q.scale, L, d, ty, tx);
  }
  if (dk) {
    at_zero(acc);
    at_tn<VEC>(acc, X3, ps, slot1, pd, S, L, d, ty, tx);
    if (has_aq) at_tn<VEC>(acc, X1, ps, slot2, pd, S, L, d, ty, tx);
    at_store_out<VEC, true>(dk, acc, q.scale, S, d, ty, tx);
  }
}

// Why the launch does not take a shape, or NULL where it does: bhg_attention_backward_vjp and bhg_attention_plan refuse the same shapes.
inline const char* at_shape_error(int B, int H, int L, int S, int d) {
  if (!(B > 0 && H > 0 && L > 0 && S > 0 && d > 0)) return "empty tensor";
  if (L > kAtMax) return "more than 64 queries";
  if (S > kAtMax) return "more than 64 keys";
  if (d > kAtMax) return "more than 64 elements per head";
  if ((long long)B * H > 0x7fffffffLL) return "more than 2^31 - 1 (batch, head) pairs";
  return nullptr;
}

// Shape -> pitches and LDS bytes, in closed form.
//   vector path: the slot pitch is d (d % 8 == 4) or d + 4, an odd number of 16-byte units: the sixteen rows tx + 16 c that one 16-byte
//     read of at_nt touches lie on sixteen different 16-byte bank groups.  The score pitch is S rounded up to 4, plus 4: rows are 16-byte
//     aligned for at_tn, and never a multiple of 32 (the four rows ty .. ty + 3 of one wave's read in at_nn start on different banks).
//   scalar path: both pitches odd.
inline const char* at_plan(AtArgs* q, int B, int H, int L, int S, int d, int vec_ok) {
  const char* bad = at_shape_error(B, H, L, S, d);
  if (bad) return bad;
  q->B = B; q->H = H; q->L = L; q->S = S; q->d = d;
  q->vec = (d % 4 == 0 && vec_ok) ? 4 : 1;
  if (q->vec == 4) {
    q->pd = d % 8 == 4 ? d : d + 4;
    q->ps = (S + 3) / 4 * 4 + 4;
    if (q->ps % 32 == 0) q->ps += 4;   // (S = 25 .. 28, 57 .. 60: the four rows would start on the same bank, or 32 banks apart)
  } else {
    q->pd = d | 1;
    q->ps = S | 1;
  }
  q->rows = L > S ? L : S;
  q->lds = (int)sizeof(float) * (4 * L * q->ps + kAtSlots * q->rows * q->pd);
  if (q->lds > kAtMaxLds) return "the plan needs more than 160 KiB of LDS";   // cannot happen for L, S, d <= 64 (139264 at most)
  return nullptr;
}

// A stride only counts where the index can be non-zero.
inline long long at_stride(const long long* st, int i, int extent) { return extent > 1 ? st[i] : 0; }

}  // namespace
}  // namespace bhg

using namespace bhg;

extern "C" {

int bhg_attention_plan(int B, int H, int L, int S, int d, int vec_ok, char* buf, size_t buf_bytes) {
  BHG_REQUIRE(buf && buf_bytes > 0, "NULL buffer");
  AtArgs q{};
  const char* bad = at_plan(&q, B, H, L, S, d, vec_ok);
  BHG_REQUIRE(!bad, bad);
  const int len = snprintf(buf, buf_bytes, "vec=%d ps=%d pd=%d rows=%d slots=%d phases=%d grid=%lld lds=%d max_lds=%d", q.vec, q.ps, q.pd,
                           q.rows, kAtSlots, kAtPhases, (long long)B * H, q.lds, kAtMaxLds);
  BHG_REQUIRE(len > 0 && (size_t)len < buf_bytes, "buffer too small for the plan line");
  return BHG_OK;
}

int bhg_attention_backward_vjp(const float* q, const float* k, const float* v, const float* go, const float* aq, const float* ak,
                               const float* av, const long long* strides, const float* mask, const long long* mask_strides, int causal,
                               float scale, int B, int H, int L, int S, int d, float* dq, float* dk, float* dv, float* dgo, void* stream) {
  AtArgs a{};
  {
    const char* bad = at_shape_error(B, H, L, S, d);
    BHG_REQUIRE(!bad, bad);
  }
  BHG_REQUIRE(q && k && v && go, "null pointer (q, k, v and go are required)");
  BHG_REQUIRE(aq || ak || av, "all three cotangents are NULL");
  BHG_REQUIRE(dq || dk || dv || dgo, "all four outputs are NULL");
  BHG_REQUIRE(strides, "null pointer (strides)");
  BHG_REQUIRE(!mask || mask_strides, "null pointer (mask_strides)");
  const float* in[AT_IN] = {q, k, v, go, aq, ak, av};
  const int rows_of[AT_IN] = {L, S, S, L, L, S, S};
  int vec_ok = 1;
  for (int i = 0; i < AT_IN; ++i) {
    a.in[i] = in[i];
    const long long* st = strides + 4 * i;
    BHG_REQUIRE(!in[i] || d == 1 || st[3] == 1, "the last stride of every input must be 1");
    a.st[i][0] = at_stride(st, 0, B); a.st[i][1] = at_stride(st, 1, H); a.st[i][2] = at_stride(st, 2, rows_of[i]);
    if (!in[i]) continue;
    for (int j = 0; j < 3; ++j) {
      BHG_REQUIRE(a.st[i][j] >= 0, "negative stride");
      if (a.st[i][j] % 4 != 0) vec_ok = 0;
    }
  }
  const char* bad = at_plan(&a, B, H, L, S, d, vec_ok);
  BHG_REQUIRE(!bad, bad);
  if (a.vec == 4) {
    for (const void* p : {(const void*)q, (const void*)k, (const void*)v, (const void*)go, (const void*)aq, (const void*)ak, (const void*)av,
                          (const void*)dq, (const void*)dk, (const void*)dv, (const void*)dgo})
      BHG_REQUIRE(((uintptr_t)p & 15) == 0, "inputs and outputs must be 16-byte aligned on the vector path (d and every stride a multiple of 4)");
  }
  a.mask = mask;
  if (mask) {
    const int ext[4] = {B, H, L, S};
    for (int j = 0; j < 4; ++j) {
      a.mst[j] = at_stride(mask_strides, j, ext[j]);
      BHG_REQUIRE(a.mst[j] >= 0, "negative stride");
    }
  }
  a.out[AT_DQ] = dq; a.out[AT_DK] = dk; a.out[AT_DV] = dv; a.out[AT_DGO] = dgo;
  a.causal = causal != 0;
  a.scale = scale;
  // above 64 KiB a kernel's dynamic LDS has to be allowed, once per process and device
  static bool attr_done[64] = {};
  int dev = 0;
  BHG_HIP_CHECK(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !attr_done[dev]) {
    BHG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_attn_vjp<4>), hipFuncAttributeMaxDynamicSharedMemorySize, kAtMaxLds));
    BHG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_attn_vjp<1>), hipFuncAttributeMaxDynamicSharedMemorySize, kAtMaxLds));
    if (dev >= 0 && dev < 64) attr_done[dev] = true;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (a.vec == 4)
    hipLaunchKernelGGL(k_attn_vjp<4>, dim3(B * H), dim3(kThreads), a.lds, st, a);
  else
    hipLaunchKernelGGL(k_attn_vjp<1>, dim3(B * H), dim3(kThreads), a.lds, st, a);
  BHG_HIP_CHECK(hipGetLastError());
  return BHG_OK;
}

}  // extern "C"
