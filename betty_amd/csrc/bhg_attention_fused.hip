// bhg_attention_fused.hip — the attention core's forward and FIRST backward without a score matrix in memory: the family of the tiled
// double backward (bhg_attention_tiled.hip: 1 <= L, S <= 512, 1 <= d <= 64, fp32, the same notation, tiles and operand layout).
//
// Per (batch, head):
//     forward          P = softmax_rows(s Q K^T + m)      O = P V            saved: O and, per query row, (mx, l) — row maximum and
//                                                                            softmax denominator, two floats, 8 bytes; never P
//     first backward   gP = gO V^T     D = rowsum(gO * O) = rowsum(P * gP)     gS = P * (gP - D)
//                      gq = s gS K     gk = s gS^T Q      gv = P^T gO          with P = exp(score - mx) / l recomputed tile by tile
// The score matrices exist one 64 x 32 tile (BM queries x BN keys) at a time.  THREE kernels, no atomics, no grid barrier:
//   k_attn_fused_f    grid B H ceil(L / 64): a block owns 64 query rows (Q resident in LDS) and streams the 32-key tiles of K and V
//       through registers (the next tile's global reads are issued before the current tile's products).  Wave w owns rows
//       16 w .. 16 w + 15, each lane one column of four rows (the accumulator layout of the MFMA): the score tile comes off the MFMA,
//       the running maximum moves, e = exp(score - mx) goes to an LDS tile as the A operand of e V, the denominator (fp64, per lane,
//       reduced over the sixteen lanes of a row once at the end) and the dp / 16 accumulator tiles of O are rescaled by
//       exp(mx_old - mx_new) when the maximum moved, and O is divided by l at the end.  A wave reads back only the rows of the e tile it
//       wrote itself.
//   k_attn_fused_bq   grid B H ceil(L / 64): D per row in fp64 (four threads per row, straight from memory) -> the workspace; then,
//       unless gq is NULL, Q and gO resident, the key tiles streamed as above, gS through the LDS tile, gq accumulated in registers.
//   k_attn_fused_bk   grid B H ceil(S / 32): K and V resident, the 64-row tiles of Q and gO streamed, (mx, l) and D read from memory,
//       P and gS through two LDS tiles (read transposed), gv and gk accumulated in registers.  Not launched when both are NULL.
// A tile whose keys are all masked leaves the running maximum at -inf: e is then taken against 0 (exp(-inf) = 0, not NaN) and the
// rescale of the still-empty sums is skipped, so live keys in a later tile are not poisoned.  A fully masked ROW ends with (mx, l) = (-inf, 0)
// and takes 1 / l = 0 in all three kernels: O and its row of gq are exact zeros and it adds nothing to gk and gv, as on torch's math
// path (2.10).  Under the causal flag the tiles wholly above the diagonal are skipped in all three kernels.
//
// Every product runs on the fp32-input MFMA v_mfma_f32_16x16x4_f32: exact fp32, bit for bit a k-ordered fmaf chain.  Lane
// (n = lane & 15, g = lane >> 4) supplies A[n][k] and B[k][n]; step c of a group of four uses k = 4 g + c, so a lane's four A values
// are ONE 16-byte LDS read.  Operand tiles are zero-padded in LDS to the tile shape (rows past L / S, columns past d up to dp = d
// rounded up to 16) at pitch pd = dp + 4; elements of the score tiles outside L x S are zeros; stores are masked.  Every loop is
// bounded by L, S, d.  Deterministic.  The kernels are instantiated per dp / 16 = 1 .. 4 and per global read width.
//
// Layout: fp32.  Inputs with four element strides each (last stride 1), read in place; outputs contiguous (B, H, L | S, d).
// vec = 4 (16-byte global reads) when d % 4 == 0 and every stride of an input is a multiple of 4; otherwise scalar reads.
// Row statistics: B H L pairs of floats (mx, l).  Workspace of the backward: B H L doubles (D).
#include "bhg_common.hpp"

#include <math.h>

namespace bhg {
namespace {

typedef float fu_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kFuMaxLen = 512, kFuMaxD = 64;
constexpr int kFuBM = 64, kFuBN = 32;      // query rows and keys of one score tile
constexpr int kFuPS = kFuBN + 4;           // row pitch of a score tile: 9 x 16 bytes
constexpr int kFuStatBytes = 8;            // per query row: float mx, float l
constexpr int kFuMaxLds = 160 * 1024;
enum { FU_Q = 0, FU_K, FU_V, FU_O, FU_GO, FU_IN };

struct FuArgs {
  const float* in[FU_IN];      // q k v o go (o and go: the backward only)
  long long st[FU_IN][3];      // element strides: batch, head, row
  const float* mask;           // may be NULL
  long long mst[4];            // element strides of the mask (0 = broadcast)
  float* o;                    // forward: (B, H, L, d) contiguous
  float2* stats_out;           // forward: B H L x (mx, l)
  const float2* stats;         // backward
  float *gq, *gk, *gv;         // backward, contiguous; each may be NULL
  double* ws;                  // backward: B H L (D)
  int B, H, L, S, d;
  int causal;
  float scale;
  int vec;                     // 4: 16-byte global reads; 1: scalar
  int dp, pd;                  // d rounded up to 16; row pitch of an operand tile (dp + 4: an odd number of 16-byte units)
  int nqt, nkt;                // query tiles of 64, key tiles of 32
  int lds_f, lds_q, lds_k;     // bytes of dynamic LDS of the three kernels
};

// Global -> LDS in two steps (as in the tiled sibling): fu_fetch reads this thread's NPT 16-byte pieces of a tile of NPT * 16 rows x dp
// floats into registers (zeros outside the `nrows` x d matrix), fu_put writes them to the LDS at pitch pd.
template <int NPT>
struct FuPieces {
  float4 v[NPT];
};

template <int VEC, int NPT>
__device__ __forceinline__ void fu_fetch(FuPieces<NPT>& p, const int dp, const float* __restrict__ src, const long long rs, const int row0,
                                         const int nrows, const int d) {
  const int nv = dp >> 2, n = NPT * (kThreads / 16) * nv;   // NPT * 16 rows
#pragma unroll
  for (int u = 0; u < NPT; ++u) {
    const int idx = threadIdx.x + u * kThreads;
    const int r = idx / nv, c = (idx - r * nv) << 2;
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (idx < n && row0 + r < nrows && c < d) {
      const float* g = src + (long long)(row0 + r) * rs + c;
      if (VEC == 4) {
        t = *reinterpret_cast<const float4*>(g);
      } else {
        t.x = g[0];
        if (c + 1 < d) t.y = g[1];
        if (c + 2 < d) t.z = g[2];
        if (c + 3 < d) t.w = g[3];
      }
    }
    p.v[u] = t;
  }
}

template <int NPT>
__device__ __forceinline__ void fu_put(float* __restrict__ dst, const int pd, const int dp, const FuPieces<NPT>& p) {
  const int nv = dp >> 2, n = NPT * (kThreads / 16) * nv;
#pragma unroll
  for (int u = 0; u < NPT; ++u) {
    const int idx = threadIdx.x + u * kThreads;
    const int r = idx / nv, c = (idx - r * nv) << 2;
    if (idx < n) *reinterpret_cast<float4*>(dst + r * pd + c) = p.v[u];
  }
}

template <int VEC, int NPT>
__device__ __forceinline__ void fu_load(float* __restrict__ dst, const int pd, const int dp, const float* __restrict__ src, const long long rs,
                                        const int row0, const int nrows, const int d) {
  FuPieces<NPT> p;
  fu_fetch<VEC, NPT>(p, dp, src, rs, row0, nrows, d);
  fu_put<NPT>(dst, pd, dp, p);
}

#define FU_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ void fu_zero2(fu_f32x4 (&a)[2]) {
  a[0] = fu_f32x4{0.f, 0.f, 0.f, 0.f};
  a[1] = fu_f32x4{0.f, 0.f, 0.f, 0.f};
}

// acc[ct] += A[16 w + n][:] . Bm[16 ct + n'][:]   (ct = 0, 1: the wave's 16 x 32 strip of a score tile; contraction over dp)
__device__ __forceinline__ void fu_nt(fu_f32x4 (&acc)[2], const float* __restrict__ A, const float* __restrict__ Bm, const int pd, const int dp,
                                      const int w, const int n, const int g) {
  const float* ar = A + (16 * w + n) * pd + 4 * g;
  const float* b0 = Bm + n * pd + 4 * g;
  const float* b1 = b0 + 16 * pd;
  float4 a = *reinterpret_cast<const float4*>(ar);
  float4 x = *reinterpret_cast<const float4*>(b0);
  float4 y = *reinterpret_cast<const float4*>(b1);
  for (int k = 16; k <= dp; k += 16) {
    float4 an = a, xn = x, yn = y;
    if (k < dp) {   // the next step's fragments are read while this step's MFMAs run
      an = *reinterpret_cast<const float4*>(ar + k);
      xn = *reinterpret_cast<const float4*>(b0 + k);
      yn = *reinterpret_cast<const float4*>(b1 + k);
    }
    acc[0] = FU_MFMA(a.x, x.x, acc[0]); acc[1] = FU_MFMA(a.x, y.x, acc[1]);
    acc[0] = FU_MFMA(a.y, x.y, acc[0]); acc[1] = FU_MFMA(a.y, y.y, acc[1]);
    acc[0] = FU_MFMA(a.z, x.z, acc[0]); acc[1] = FU_MFMA(a.z, y.z, acc[1]);
    acc[0] = FU_MFMA(a.w, x.w, acc[0]); acc[1] = FU_MFMA(a.w, y.w, acc[1]);
    a = an; x = xn; y = yn;
  }
}

// acc[cb] += X[16 w + n][j] M[j][16 cb + n']     (the wave's 16 rows x dp outputs; contraction over the 32 keys of the tile)
template <int NCB>
__device__ __forceinline__ void fu_nn(fu_f32x4 (&acc)[NCB], const float* __restrict__ X, const float* __restrict__ M, const int pd, const int w,
                                      const int n, const int g) {
  const float* xr = X + (16 * w + n) * kFuPS + 4 * g;
#pragma unroll
  for (int j0 = 0; j0 < kFuBN; j0 += 16) {
    const float4 a4 = *reinterpret_cast<const float4*>(xr + j0);
    const float a[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float* mr = M + (j0 + 4 * g + c) * pd + n;
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) acc[cb] = FU_MFMA(a[c], mr[16 * cb], acc[cb]);
    }
  }
}

// acc += sum_i X[i][16 kb + n] M[i][16 cb + n']   (one 16 keys x 16 columns output tile; contraction over the 64 queries of the tile)
__device__ __forceinline__ void fu_tn(fu_f32x4& acc, const float* __restrict__ X, const float* __restrict__ M, const int pd, const int kb,
                                      const int cb, const int n, const int g) {
  const float* xc = X + 16 * kb + n;
  const float* mc = M + 16 * cb + n;
#pragma unroll
  for (int i0 = 0; i0 < kFuBM; i0 += 16) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + 4 * g + c;
      acc = FU_MFMA(xc[i * kFuPS], mc[i * pd], acc);
    }
  }
}

// Score of element (i, j) from the raw product; -inf outside L x S and above the diagonal under the causal flag.
__device__ __forceinline__ float fu_score(const float raw, const FuArgs& q, const float* __restrict__ mbase, const int i, const int j) {
  if (i >= q.L || j >= q.S || (q.causal && j > i)) return -INFINITY;
  float sc = q.scale * raw;
  if (mbase) sc += mbase[(long long)i * q.mst[2] + (long long)j * q.mst[3]];
  return sc;
}

__device__ __forceinline__ float fu_max16(float v) {   // over the sixteen lanes that hold one row
  v = fmaxf(v, __shfl_xor(v, 1));
  v = fmaxf(v, __shfl_xor(v, 2));
  v = fmaxf(v, __shfl_xor(v, 4));
  v = fmaxf(v, __shfl_xor(v, 8));
  return v;
}

__device__ __forceinline__ double fu_sum16(double v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}

// out[(row0 + 4 g + r)][16 cb + n] = f[r] * acc[r], rows < nrows, columns < d; `out` is the (b, h) slice, contiguous rows of d.
__device__ __forceinline__ void fu_store(float* __restrict__ out, const fu_f32x4& acc, const float (&f)[4], const int row0, const int nrows,
                                         const int cb, const int d, const int n, const int g) {
  const int col = 16 * cb + n;
  if (col >= d) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + 4 * g + r;
    if (row < nrows) out[(long long)row * d + col] = f[r] * acc[r];
  }
}

// key tiles that hold an element on or below the diagonal for some row of the query tile at i0
__device__ __forceinline__ int fu_live_key_tiles(const FuArgs& q, const int i0) {
  if (!q.causal) return q.nkt;
  const int last = (i0 + kFuBM - 1 < q.L - 1 ? i0 + kFuBM - 1 : q.L - 1) / kFuBN + 1;
  return last < q.nkt ? last : q.nkt;
}

// grid = B * H * nqt.  Block: 64 query rows.  LDS: Q (64 x pd), K and V (32 x pd each), the e tile (64 x 36).
template <int VEC, int NCB>
__global__ __launch_bounds__(kThreads) void k_attn_fused_f(const FuArgs q) {
  extern __shared__ __attribute__((aligned(16))) float fu_lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = lane & 15, g = lane >> 4;
  constexpr int dp = 16 * NCB, pd = dp + 4;
  const int L = q.L, S = q.S, d = q.d;
  const int bh = blockIdx.x / q.nqt, qt = blockIdx.x - bh * q.nqt;
  const int b = bh / q.H, h = bh - b * q.H;
  const int i0 = qt * kFuBM;
  float* const Qs = fu_lds;
  float* const Ks = Qs + kFuBM * pd;
  float* const Vs = Ks + kFuBN * pd;
  float* const X = Vs + kFuBN * pd;
  const float* const qsrc = q.in[FU_Q] + (b * q.st[FU_Q][0] + h * q.st[FU_Q][1]);
  const float* const ksrc = q.in[FU_K] + (b * q.st[FU_K][0] + h * q.st[FU_K][1]);
  const float* const vsrc = q.in[FU_V] + (b * q.st[FU_V][0] + h * q.st[FU_V][1]);
  const float* mbase = q.mask ? q.mask + (b * q.mst[0] + h * q.mst[1]) : nullptr;
  const int nkt = fu_live_key_tiles(q, i0);

  fu_load<VEC, 4>(Qs, pd, dp, qsrc, q.st[FU_Q][2], i0, L, d);
  FuPieces<2> pk, pv;
  fu_fetch<VEC, 2>(pk, dp, ksrc, q.st[FU_K][2], 0, S, d);
  fu_fetch<VEC, 2>(pv, dp, vsrc, q.st[FU_V][2], 0, S, d);

  float mx[4];
  double a_l[4];
  fu_f32x4 acc[NCB];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    mx[r] = -INFINITY;
    a_l[r] = 0.0;
  }
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) acc[cb] = fu_f32x4{0.f, 0.f, 0.f, 0.f};

  for (int kt = 0; kt < nkt; ++kt) {
    const int j0 = kt * kFuBN;
    __syncthreads();   // the previous tile's reads are done
    fu_put<2>(Ks, pd, dp, pk);
    fu_put<2>(Vs, pd, dp, pv);
    __syncthreads();
    if (kt + 1 < nkt) {
      fu_fetch<VEC, 2>(pk, dp, ksrc, q.st[FU_K][2], j0 + kFuBN, S, d);
      fu_fetch<VEC, 2>(pv, dp, vsrc, q.st[FU_V][2], j0 + kFuBN, S, d);
    }
    fu_f32x4 s0[2];
    fu_zero2(s0);
    fu_nt(s0, Qs, Ks, pd, dp, w, n, g);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * w + 4 * g + r, i = i0 + row;
      const float sc0 = fu_score(s0[0][r], q, mbase, i, j0 + n);
      const float sc1 = fu_score(s0[1][r], q, mbase, i, j0 + 16 + n);
      const float m_old = mx[r];
      const float m_new = fmaxf(m_old, fu_max16(fmaxf(sc0, sc1)));
      const float mu = m_new == -INFINITY ? 0.f : m_new;
      if (m_old != -INFINITY && m_new != m_old) {   // (while the maximum is -inf the sums are empty: nothing to rescale)
        const float f = expf(m_old - m_new);
        a_l[r] *= (double)f;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) acc[cb][r] *= f;
      }
      mx[r] = m_new;
      const float e0 = expf(sc0 - mu), e1 = expf(sc1 - mu);
      a_l[r] += (double)e0 + (double)e1;
      X[row * kFuPS + n] = e0;
      X[row * kFuPS + 16 + n] = e1;
    }
    __syncthreads();
    fu_nn<NCB>(acc, X, Vs, pd, w, n, g);
  }
  float* const o = q.o + (long long)bh * L * d;
  float il[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double l = fu_sum16(a_l[r]);
    il[r] = l > 0.0 ? (float)(1.0 / l) : 0.f;   // a fully masked row: O = 0, saved as (mx, l) = (-inf, 0)
    const int i = i0 + 16 * w + 4 * g + r;
    if (n == 0 && i < L) q.stats_out[(long long)bh * L + i] = make_float2(mx[r], (float)l);
  }
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) fu_store(o, acc[cb], il, i0 + 16 * w, L, cb, d, n, g);
}

// P and gS of this wave's strip from the raw products and the row statistics -> the score tiles (zeros outside L x S); XP may be NULL.
__device__ __forceinline__ void fu_write_scores(const fu_f32x4 (&s0)[2], const fu_f32x4 (&gp)[2], const float (&mx)[4], const double (&il)[4],
                                                const double (&D)[4], const FuArgs& q, const float* __restrict__ mbase, float* XP, float* XG,
                                                const int i0, const int j0, const int w, const int n, const int g) {
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int j = j0 + 16 * ct + n;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * w + 4 * g + r, i = i0 + row;
      float pf = 0.f, gs = 0.f;
      if (i < q.L && j < q.S) {
        const float sc = fu_score(s0[ct][r], q, mbase, i, j);
        const float mu = mx[r] == -INFINITY ? 0.f : mx[r];
        pf = (float)((double)expf(sc - mu) * il[r]);
        gs = (float)((double)pf * ((double)gp[ct][r] - D[r]));
      }
      const int at = row * kFuPS + 16 * ct + n;
      if (XP) XP[at] = pf;
      XG[at] = gs;
    }
  }
}

// grid = B * H * nqt.  Block: 64 query rows.  LDS: Q, gO (64 x pd each), K, V (32 x pd each), the gS tile (64 x 36), D (64 doubles).
template <int VEC, int NCB>
__global__ __launch_bounds__(kThreads) void k_attn_fused_bq(const FuArgs q) {
  extern __shared__ __attribute__((aligned(16))) float fu_lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = lane & 15, g = lane >> 4;
  constexpr int dp = 16 * NCB, pd = dp + 4;
  const int L = q.L, S = q.S, d = q.d;
  const int bh = blockIdx.x / q.nqt, qt = blockIdx.x - bh * q.nqt;
  const int b = bh / q.H, h = bh - b * q.H;
  const int i0 = qt * kFuBM;
  float* const Qs = fu_lds;
  float* const GOs = Qs + kFuBM * pd;
  float* const Ks = GOs + kFuBM * pd;
  float* const Vs = Ks + kFuBN * pd;
  float* const X = Vs + kFuBN * pd;
  double* const Ds = reinterpret_cast<double*>(X + kFuBM * kFuPS);   // (an even number of floats precedes it: 8-byte aligned)
  const float* src[FU_IN];
#pragma unroll
  for (int i = 0; i < FU_IN; ++i) src[i] = q.in[i] + (b * q.st[i][0] + h * q.st[i][1]);
  const float* mbase = q.mask ? q.mask + (b * q.mst[0] + h * q.mst[1]) : nullptr;

  // D = rowsum(gO * O): four threads per row, fp64
  {
    const int row = tid >> 2, part = tid & 3, i = i0 + row;
    double sum = 0.0;
    if (i < L) {
      const float* go = src[FU_GO] + (long long)i * q.st[FU_GO][2];
      const float* o = src[FU_O] + (long long)i * q.st[FU_O][2];
      if (VEC == 4) {
        for (int c = 4 * part; c < d; c += 16) {
          const float4 x = *reinterpret_cast<const float4*>(go + c), y = *reinterpret_cast<const float4*>(o + c);
          sum += (double)x.x * (double)y.x + (double)x.y * (double)y.y + (double)x.z * (double)y.z + (double)x.w * (double)y.w;
        }
      } else {
        for (int c = part; c < d; c += 4) sum += (double)go[c] * (double)o[c];
      }
    }
    sum += __shfl_xor(sum, 1);
    sum += __shfl_xor(sum, 2);
    if (part == 0) {
      Ds[row] = sum;
      if (i < L) q.ws[(long long)bh * L + i] = sum;
    }
  }
  float* const gq = q.gq ? q.gq + (long long)bh * L * d : nullptr;
  if (!gq) return;   // uniform over the grid
  const int nkt = fu_live_key_tiles(q, i0);

  fu_load<VEC, 4>(Qs, pd, dp, src[FU_Q], q.st[FU_Q][2], i0, L, d);
  fu_load<VEC, 4>(GOs, pd, dp, src[FU_GO], q.st[FU_GO][2], i0, L, d);
  FuPieces<2> pk, pv;
  fu_fetch<VEC, 2>(pk, dp, src[FU_K], q.st[FU_K][2], 0, S, d);
  fu_fetch<VEC, 2>(pv, dp, src[FU_V], q.st[FU_V][2], 0, S, d);
  __syncthreads();   // Ds
  float mx[4];
  double il[4], D[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 16 * w + 4 * g + r, i = i0 + row;
    mx[r] = 0.f; il[r] = 1.0;
    D[r] = Ds[row];
    if (i < L) {
      const float2 st = q.stats[(long long)bh * L + i];
      mx[r] = st.x; il[r] = st.y > 0.f ? 1.0 / (double)st.y : 0.0;   // l = 0: a dead row, P = 0
    }
  }
  fu_f32x4 acc[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) acc[cb] = fu_f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kt = 0; kt < nkt; ++kt) {
    const int j0 = kt * kFuBN;
    __syncthreads();
    fu_put<2>(Ks, pd, dp, pk);
    fu_put<2>(Vs, pd, dp, pv);
    __syncthreads();
    if (kt + 1 < nkt) {
      fu_fetch<VEC, 2>(pk, dp, src[FU_K], q.st[FU_K][2], j0 + kFuBN, S, d);
      fu_fetch<VEC, 2>(pv, dp, src[FU_V], q.st[FU_V][2], j0 + kFuBN, S, d);
    }
    fu_f32x4 s0[2], gp[2];
    fu_zero2(s0); fu_zero2(gp);
    fu_nt(s0, Qs, Ks, pd, dp, w, n, g);
    fu_nt(gp, GOs, Vs, pd, dp, w, n, g);
    fu_write_scores(s0, gp, mx, il, D, q, mbase, nullptr, X, i0, j0, w, n, g);
    __syncthreads();
    fu_nn<NCB>(acc, X, Ks, pd, w, n, g);
  }
  const float f[4] = {q.scale, q.scale, q.scale, q.scale};
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) fu_store(gq, acc[cb], f, i0 + 16 * w, L, cb, d, n, g);
}

// grid = B * H * nkt.  Block: 32 keys.  LDS: Q, gO (64 x pd each, streamed), K, V (32 x pd each, resident), the P and gS tiles (64 x 36 each).
template <int VEC, int NCB>
__global__ __launch_bounds__(kThreads) void k_attn_fused_bk(const FuArgs q) {
  extern __shared__ __attribute__((aligned(16))) float fu_lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = lane & 15, g = lane >> 4;
  constexpr int dp = 16 * NCB, pd = dp + 4;
  const int L = q.L, S = q.S, d = q.d;
  const int bh = blockIdx.x / q.nkt, kt = blockIdx.x - bh * q.nkt;
  const int b = bh / q.H, h = bh - b * q.H;
  const int j0 = kt * kFuBN;
  float* const Qs = fu_lds;
  float* const GOs = Qs + kFuBM * pd;
  float* const Ks = GOs + kFuBM * pd;
  float* const Vs = Ks + kFuBN * pd;
  float* const XP = Vs + kFuBN * pd;
  float* const XG = XP + kFuBM * kFuPS;
  const float* src[FU_IN];
#pragma unroll
  for (int i = 0; i < FU_IN; ++i) src[i] = q.in[i] + (b * q.st[i][0] + h * q.st[i][1]);
  const float* mbase = q.mask ? q.mask + (b * q.mst[0] + h * q.mst[1]) : nullptr;
  float* const gk = q.gk ? q.gk + (long long)bh * S * d : nullptr;
  float* const gv = q.gv ? q.gv + (long long)bh * S * d : nullptr;
  const int qt0 = q.causal ? j0 / kFuBM : 0;   // query tiles above hold only rows i < j0: wholly above the diagonal
  // the wave's output tiles t = w and w + 4 of the 2 (key blocks) x NCB (column blocks) grid
  constexpr int ntile = 2 * NCB;
  fu_f32x4 acc_k[2], acc_v[2];
  fu_zero2(acc_k); fu_zero2(acc_v);

  fu_load<VEC, 2>(Ks, pd, dp, src[FU_K], q.st[FU_K][2], j0, S, d);
  fu_load<VEC, 2>(Vs, pd, dp, src[FU_V], q.st[FU_V][2], j0, S, d);
  FuPieces<4> pq, pgo;
  if (qt0 < q.nqt) {
    fu_fetch<VEC, 4>(pq, dp, src[FU_Q], q.st[FU_Q][2], qt0 * kFuBM, L, d);
    fu_fetch<VEC, 4>(pgo, dp, src[FU_GO], q.st[FU_GO][2], qt0 * kFuBM, L, d);
  }
  for (int qt = qt0; qt < q.nqt; ++qt) {
    const int i0 = qt * kFuBM;
    __syncthreads();
    fu_put<4>(Qs, pd, dp, pq);
    fu_put<4>(GOs, pd, dp, pgo);
    float mx[4];
    double il[4], D[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + 16 * w + 4 * g + r;
      mx[r] = 0.f; il[r] = 1.0; D[r] = 0.0;
      if (i < L) {
        const float2 st = q.stats[(long long)bh * L + i];
        mx[r] = st.x; il[r] = st.y > 0.f ? 1.0 / (double)st.y : 0.0;   // l = 0: a dead row, P = 0
        D[r] = q.ws[(long long)bh * L + i];
      }
    }
    __syncthreads();
    if (qt + 1 < q.nqt) {
      fu_fetch<VEC, 4>(pq, dp, src[FU_Q], q.st[FU_Q][2], i0 + kFuBM, L, d);
      fu_fetch<VEC, 4>(pgo, dp, src[FU_GO], q.st[FU_GO][2], i0 + kFuBM, L, d);
    }
    fu_f32x4 s0[2], gp[2];
    fu_zero2(s0); fu_zero2(gp);
    fu_nt(s0, Qs, Ks, pd, dp, w, n, g);
    if (gk) fu_nt(gp, GOs, Vs, pd, dp, w, n, g);
    fu_write_scores(s0, gp, mx, il, D, q, mbase, XP, XG, i0, j0, w, n, g);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int t = w + 4 * u;
      if (t >= ntile) break;
      const int kb = t & 1, cb = t >> 1;
      if (gv) fu_tn(acc_v[u], XP, GOs, pd, kb, cb, n, g);
      if (gk) fu_tn(acc_k[u], XG, Qs, pd, kb, cb, n, g);
    }
  }
  const float fk[4] = {q.scale, q.scale, q.scale, q.scale}, fv[4] = {1.f, 1.f, 1.f, 1.f};
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int t = w + 4 * u;
    if (t >= ntile) break;
    const int kb = t & 1, cb = t >> 1;
    if (gk) fu_store(gk, acc_k[u], fk, j0 + 16 * kb, S, cb, d, n, g);
    if (gv) fu_store(gv, acc_v[u], fv, j0 + 16 * kb, S, cb, d, n, g);
  }
}

// The launches, the plan and the workspace size refuse the same shapes, with the tiled sibling's words.
inline const char* fu_shape_error(int B, int H, int L, int S, int d) {
  if (!(B > 0 && H > 0 && L > 0 && S > 0 && d > 0)) return "empty tensor";
  if (L > kFuMaxLen) return "more than 512 queries";
  if (S > kFuMaxLen) return "more than 512 keys";
  if (d > kFuMaxD) return "more than 64 elements per head";
  const long long bh = (long long)B * H;
  if (bh * ((L + kFuBM - 1) / kFuBM) > 0x7fffffffLL || bh * ((S + kFuBN - 1) / kFuBN) > 0x7fffffffLL)
    return "a grid of more than 2^31 - 1 workgroups";
  return nullptr;
}

inline size_t fu_ws_bytes(int B, int H, int L) { return (size_t)B * H * L * sizeof(double); }

// Shape -> tiles, pitches and LDS bytes.  Operand tiles at pitch pd = dp + 4, an odd number of 16-byte units; score tiles 64 x 32 at
// pitch 36.  Forward: Q, K, V and the e tile.  Query launch: Q, gO, K, V, the gS tile and 64 doubles (D).  Key launch: Q, gO, K, V
// and two score tiles (P, gS).
inline const char* fu_plan(FuArgs* q, int B, int H, int L, int S, int d, int vec_ok) {
  const char* bad = fu_shape_error(B, H, L, S, d);
  if (bad) return bad;
  q->B = B; q->H = H; q->L = L; q->S = S; q->d = d;
  q->vec = (d % 4 == 0 && vec_ok) ? 4 : 1;
  q->dp = (d + 15) / 16 * 16;
  q->pd = q->dp + 4;
  q->nqt = (L + kFuBM - 1) / kFuBM;
  q->nkt = (S + kFuBN - 1) / kFuBN;
  const int score = kFuBM * kFuPS;
  q->lds_f = (int)sizeof(float) * ((kFuBM + 2 * kFuBN) * q->pd + score);
  q->lds_q = (int)sizeof(float) * ((2 * kFuBM + 2 * kFuBN) * q->pd + score) + kFuBM * (int)sizeof(double);
  q->lds_k = (int)sizeof(float) * ((2 * kFuBM + 2 * kFuBN) * q->pd + 2 * score);
  if (q->lds_k > kFuMaxLds) return "the plan needs more than 160 KiB of LDS";   // cannot happen for d <= 64 (70656)
  return nullptr;
}

inline long long fu_stride(const long long* st, int i, int extent) { return extent > 1 ? st[i] : 0; }

// Shared by the two entry points: shape, strides of the first `nin` inputs, read width, alignment, mask.  NULL, or the refusal.
inline const char* fu_prepare(FuArgs* a, const float* const* in, int nin, const long long* strides, const float* mask, const long long* mask_strides,
                              int causal, float scale, int B, int H, int L, int S, int d) {
  const char* bad = fu_shape_error(B, H, L, S, d);
  if (bad) return bad;
  if (!strides) return "null pointer (strides)";
  if (mask && !mask_strides) return "null pointer (mask_strides)";
  const int rows_of[FU_IN] = {L, S, S, L, L};
  int vec_ok = 1;
  for (int i = 0; i < nin; ++i) {
    if (!in[i]) return "null pointer (an input)";
    a->in[i] = in[i];
    const long long* st = strides + 4 * i;
    if (!(d == 1 || st[3] == 1)) return "the last stride of every input must be 1";
    a->st[i][0] = fu_stride(st, 0, B); a->st[i][1] = fu_stride(st, 1, H); a->st[i][2] = fu_stride(st, 2, rows_of[i]);
    for (int j = 0; j < 3; ++j) {
      if (a->st[i][j] < 0) return "negative stride";
      if (a->st[i][j] % 4 != 0) vec_ok = 0;
    }
  }
  bad = fu_plan(a, B, H, L, S, d, vec_ok);
  if (bad) return bad;
  if (a->vec == 4)
    for (int i = 0; i < nin; ++i)
      if (((uintptr_t)in[i] & 15) != 0) return "inputs and outputs must be 16-byte aligned on the vector path (d and every stride a multiple of 4)";
  a->mask = mask;
  if (mask) {
    const int ext[4] = {B, H, L, S};
    for (int j = 0; j < 4; ++j) {
      a->mst[j] = fu_stride(mask_strides, j, ext[j]);
      if (a->mst[j] < 0) return "negative stride";
    }
  }
  a->causal = causal != 0;
  a->scale = scale;
  return nullptr;
}

#undef FU_MFMA

}  // namespace
}  // namespace bhg

using namespace bhg;

extern "C" {

size_t bhg_attention_fused_ws_bytes(int B, int H, int L) {
  if (!(B > 0 && H > 0 && L > 0)) return 0;
  return fu_ws_bytes(B, H, L);
}

int bhg_attention_fused_plan(int B, int H, int L, int S, int d, int vec_ok, char* buf, size_t buf_bytes) {
  BHG_REQUIRE(buf && buf_bytes > 0, "NULL buffer");
  FuArgs q{};
  const char* bad = fu_plan(&q, B, H, L, S, d, vec_ok);
  BHG_REQUIRE(!bad, bad);
  const int len = snprintf(buf, buf_bytes,
                           "vec=%d bm=%d bn=%d ps=%d dp=%d pd=%d grid_f=%lld grid_q=%lld grid_k=%lld lds_f=%d lds_q=%d lds_k=%d stats=%d ws=%llu",
                           q.vec, kFuBM, kFuBN, kFuPS, q.dp, q.pd, (long long)B * H * q.nqt, (long long)B * H * q.nqt, (long long)B * H * q.nkt,
                           q.lds_f, q.lds_q, q.lds_k, kFuStatBytes, (unsigned long long)fu_ws_bytes(B, H, L));
  BHG_REQUIRE(len > 0 && (size_t)len < buf_bytes, "buffer too small for the plan line");
  return BHG_OK;
}

int bhg_attention_fused_forward(const float* q, const float* k, const float* v, const long long* strides, const float* mask,
                                const long long* mask_strides, int causal, float scale, int B, int H, int L, int S, int d, float* o, void* stats,
                                void* stream) {
  FuArgs a{};
  const float* in[3] = {q, k, v};
  const char* bad = fu_prepare(&a, in, 3, strides, mask, mask_strides, causal, scale, B, H, L, S, d);
  BHG_REQUIRE(!bad, bad);
  BHG_REQUIRE(o && stats, "null pointer (o and stats are required)");
  BHG_REQUIRE(a.vec != 4 || ((uintptr_t)o & 15) == 0, "inputs and outputs must be 16-byte aligned on the vector path (d and every stride a multiple of 4)");
  BHG_REQUIRE(((uintptr_t)stats & 7) == 0, "the row statistics must be 8-byte aligned");
  a.o = o;
  a.stats_out = static_cast<float2*>(stats);
  using Kernel = void (*)(const FuArgs);
  static const Kernel kf[2][4] = {{k_attn_fused_f<1, 1>, k_attn_fused_f<1, 2>, k_attn_fused_f<1, 3>, k_attn_fused_f<1, 4>},
                                  {k_attn_fused_f<4, 1>, k_attn_fused_f<4, 2>, k_attn_fused_f<4, 3>, k_attn_fused_f<4, 4>}};
  const unsigned grid = (unsigned)((long long)B * H * a.nqt);
  hipLaunchKernelGGL(kf[a.vec == 4 ? 1 : 0][a.dp / 16 - 1], dim3(grid), dim3(kThreads), a.lds_f, static_cast<hipStream_t>(stream), a);
  BHG_HIP_CHECK(hipGetLastError());
  return BHG_OK;
}

int bhg_attention_fused_backward(const float* q, const float* k, const float* v, const float* o, const float* go, const void* stats,
                                 const long long* strides, const float* mask, const long long* mask_strides, int causal, float scale, int B, int H,
                                 int L, int S, int d, float* gq, float* gk, float* gv, void* ws, size_t ws_bytes, void* stream) {
  FuArgs a{};
  const float* in[FU_IN] = {q, k, v, o, go};
  const char* bad = fu_prepare(&a, in, FU_IN, strides, mask, mask_strides, causal, scale, B, H, L, S, d);
  BHG_REQUIRE(!bad, bad);
  BHG_REQUIRE(stats, "null pointer (stats)");
  BHG_REQUIRE(((uintptr_t)stats & 7) == 0, "the row statistics must be 8-byte aligned");
  BHG_REQUIRE(gq || gk || gv, "all three outputs are NULL");
  BHG_REQUIRE(ws, "null pointer (workspace)");
  BHG_REQUIRE(ws_bytes >= fu_ws_bytes(B, H, L), "workspace too small (bhg_attention_fused_ws_bytes)");
  BHG_REQUIRE(((uintptr_t)ws & 7) == 0, "the workspace must be 8-byte aligned");
  if (a.vec == 4)
    for (const void* p : {(const void*)gq, (const void*)gk, (const void*)gv})
      BHG_REQUIRE(((uintptr_t)p & 15) == 0, "inputs and outputs must be 16-byte aligned on the vector path (d and every stride a multiple of 4)");
  a.stats = static_cast<const float2*>(stats);
  a.gq = gq; a.gk = gk; a.gv = gv;
  a.ws = static_cast<double*>(ws);
  using Kernel = void (*)(const FuArgs);
  static const Kernel kq[2][4] = {{k_attn_fused_bq<1, 1>, k_attn_fused_bq<1, 2>, k_attn_fused_bq<1, 3>, k_attn_fused_bq<1, 4>},
                                  {k_attn_fused_bq<4, 1>, k_attn_fused_bq<4, 2>, k_attn_fused_bq<4, 3>, k_attn_fused_bq<4, 4>}};
  static const Kernel kk[2][4] = {{k_attn_fused_bk<1, 1>, k_attn_fused_bk<1, 2>, k_attn_fused_bk<1, 3>, k_attn_fused_bk<1, 4>},
                                  {k_attn_fused_bk<4, 1>, k_attn_fused_bk<4, 2>, k_attn_fused_bk<4, 3>, k_attn_fused_bk<4, 4>}};
  // above 64 KiB (the key launch at dp = 64) a kernel's dynamic LDS has to be allowed, once per process and device
  static bool attr_done[64] = {};
  int dev = 0;
  BHG_HIP_CHECK(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !attr_done[dev]) {
    for (int i = 0; i < 2; ++i)
      for (int j = 0; j < 4; ++j)
        BHG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kk[i][j]), hipFuncAttributeMaxDynamicSharedMemorySize, kFuMaxLds));
    if (dev >= 0 && dev < 64) attr_done[dev] = true;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned grid_q = (unsigned)((long long)B * H * a.nqt), grid_k = (unsigned)((long long)B * H * a.nkt);
  const int vi = a.vec == 4 ? 1 : 0, ci = a.dp / 16 - 1;
  hipLaunchKernelGGL(kq[vi][ci], dim3(grid_q), dim3(kThreads), a.lds_q, st, a);
  BHG_HIP_CHECK(hipGetLastError());
  if (gk || gv) {
    hipLaunchKernelGGL(kk[vi][ci], dim3(grid_k), dim3(kThreads), a.lds_k, st, a);
    BHG_HIP_CHECK(hipGetLastError());
  }
  return BHG_OK;
}

}  // extern "C"
