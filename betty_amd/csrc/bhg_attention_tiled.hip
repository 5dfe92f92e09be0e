// bhg_attention_tiled.hip — the Hessian-vector product's share of an attention core beyond 64 tokens: the tiled sibling of
// bhg_attention.hip (same quantities, same notation, same interface plus a workspace), for 1 <= L, S <= 512 and 1 <= d <= 64.
//
// Per (batch, head), as in the sibling:
//     P = softmax_rows(s Q K^T + m)     gP = gO V^T     D = rowsum(P * gP)     gS = P * (gP - D)
//     T = s (aQ K^T + Q aK^T)           E = rowsum(P * T)                      bgP = P * (T - E)
//     bP = T * (gP - D) - gP * E + gO aV^T              R = rowsum(P * bP)     bS = P * (bP - R)
//     dgO = bgP V + P aV     dV = bgP^T gO     dQ = s (bS K + gS aK)     dK = s (bS^T Q + gS^T aQ)
// An L x S matrix no longer fits one CU, so the score matrices exist one 64 x 32 tile (BM queries x BN keys) at a time, and the five
// row quantities m (row maximum), l (softmax denominator), D, E, R come out of ONE online pass over the key tiles: with
// e = exp(score - m_running) the pass keeps five unnormalised sums per row,
//     sum e      sum e gP      sum e T      sum e T gP      sum e (gO aV^T)
// rescales them by exp(m_old - m_new) when the running maximum moves, and divides by l at the end.  R needs no second pass:
//     R = rowsum(P * T * gP) - 2 D E + rowsum(P * (gO aV^T))            (bP summed against P, with rowsum(P) = 1).
// A tile whose keys are all masked leaves the running maximum at -inf: e is then taken against 0 (exp(-inf) = 0, not NaN) and the
// rescale of the still-empty sums is skipped, so live keys in a later tile are not poisoned.  A fully masked ROW ends with l = 0 and
// is NaN, as on the math path and in the sibling.
//
// TWO launches, no atomics, no grid barrier (float64 restatement of exactly this scheme: tests/attention_tiled_ref.py):
//   k_attn_tiled_q   grid B H ceil(L / 64): a block owns 64 query rows (Q, gO, aQ resident in LDS) and sweeps the key tiles twice.
//       (a) the online pass; the five sums are fp64 and live in registers: wave w owns rows 16 w .. 16 w + 15, each lane one column of
//           four rows (the accumulator layout of the MFMA), reduced over the sixteen lanes of a row once at the end; the statistics go
//           to the workspace for the second launch and stay in registers for (b).
//       (b) recomputes the four raw products per tile, forms P, gS, bgP, bS from the finished statistics, writes them to four score
//           tiles in LDS and accumulates dQ and dgO in registers across the key tiles; stored once.  Skipped when both are NULL.
//   k_attn_tiled_k   grid B H ceil(S / 32): a block owns 32 keys (K, V, aK, aV resident), sweeps the 64-row query tiles with the
//       statistics read from the workspace, and accumulates dK and dV.  Not launched when both are NULL.
// Under the causal flag the tiles wholly above the diagonal are skipped in both launches.
//
// Every product runs on the fp32-input MFMA v_mfma_f32_16x16x4_f32: exact fp32, bit for bit a k-ordered fmaf chain.  Lane
// (n = lane & 15, g = lane >> 4) supplies A[n][k] and B[k][n]; any k <-> (g, step) assignment is valid as long as A and B agree, and
// here step c of a group of four uses k = 4 g + c, so a lane's four A values are ONE 16-byte LDS read.  Operand tiles are zero-padded
// in LDS to the tile shape (rows past L / S, columns past d up to dp = d rounded up to 16), so no product needs an edge case; elements
// of the score tiles outside L x S are written as zeros; stores are masked.  Every loop is bounded by L, S, d.  Deterministic.
// The kernels are instantiated per dp / 16 = 1 .. 4, so every product loop unrolls and its LDS reads run ahead of its MFMAs (with dp a
// run-time value the same code took 3.4 ms instead of 2.0 at 16 x 12 x 512 x 512 x 64), and the tile that streams — keys in the first
// launch, queries in the second — comes through registers: its global reads are issued before the current tile's products.
//
// Layout: fp32.  Inputs with four element strides each (last stride 1), read in place; outputs contiguous (B, H, L | S, d).
// vec = 4 (16-byte global reads) when d % 4 == 0 and every stride of a present input is a multiple of 4; otherwise scalar reads.  The LDS
// image is the same on both paths.  Workspace: B H L rows of five doubles (m, l, D, E, R), 40 bytes per query row.
#include "bhg_common.hpp"

#include <math.h>

namespace bhg {
namespace {

typedef float tl_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTlMaxLen = 512, kTlMaxD = 64;
constexpr int kTlBM = 64, kTlBN = 32;      // query rows and keys of one score tile
constexpr int kTlPS = kTlBN + 4;           // row pitch of a score tile: 9 x 16 bytes
constexpr int kTlStats = 5;                // doubles per query row in the workspace: m l D E R
constexpr int kTlMaxLds = 160 * 1024;
enum { TL_Q = 0, TL_K, TL_V, TL_GO, TL_AQ, TL_AK, TL_AV, TL_IN };
enum { TL_DQ = 0, TL_DK, TL_DV, TL_DGO, TL_OUT };

struct TlArgs {
  const float* in[TL_IN];      // q k v go aq ak av; the last three may be NULL
  long long st[TL_IN][3];      // element strides: batch, head, row
  const float* mask;           // may be NULL
  long long mst[4];            // element strides of the mask (0 = broadcast)
  float* out[TL_OUT];          // dq dk dv dgo, contiguous; each may be NULL
  double* ws;                  // B H L x 5
  int B, H, L, S, d;
  int causal;
  float scale;
  int vec;                     // 4: 16-byte global reads; 1: scalar
  int dp, pd;                  // d rounded up to 16; row pitch of an operand tile (dp + 4: an odd number of 16-byte units)
  int nqt, nkt;                // query tiles of 64, key tiles of 32
  int lds_q, lds_k;            // bytes of dynamic LDS of the two launches
};

// Global -> LDS: a tile of NPT * 16 rows x dp floats at pitch pd, rows row0 .. of the `nrows` x d matrix at src (row stride rs), zeros
// outside the matrix — in two steps, so that the global reads of the NEXT tile can be in flight while the current one is computed: tl_fetch
// reads this thread's NPT 16-byte pieces (tile rows x dp / 4 pieces, 256 threads: NPT = 2 for 32 rows, 4 for 64) into registers,
// tl_put writes them to the LDS once the previous tile's readers have passed the barrier.
template <int NPT>
struct TlPieces {
  float4 v[NPT];
};

template <int VEC, int NPT>
__device__ __forceinline__ void tl_fetch(TlPieces<NPT>& p, const int dp, const float* __restrict__ src, const long long rs, const int row0,
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
__device__ __forceinline__ void tl_put(float* __restrict__ dst, const int pd, const int dp, const TlPieces<NPT>& p) {
  const int nv = dp >> 2, n = NPT * (kThreads / 16) * nv;
#pragma unroll
  for (int u = 0; u < NPT; ++u) {
    const int idx = threadIdx.x + u * kThreads;
    const int r = idx / nv, c = (idx - r * nv) << 2;
    if (idx < n) *reinterpret_cast<float4*>(dst + r * pd + c) = p.v[u];
  }
}

// Both steps at once, for the tiles that stay resident.
template <int VEC, int NPT>
__device__ __forceinline__ void tl_load(float* __restrict__ dst, const int pd, const int dp, const float* __restrict__ src, const long long rs,
                                        const int row0, const int nrows, const int d) {
  TlPieces<NPT> p;
  tl_fetch<VEC, NPT>(p, dp, src, rs, row0, nrows, d);
  tl_put<NPT>(dst, pd, dp, p);
}

#define TL_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// acc[ct] += A[16 w + n][:] . Bm[16 ct + n'][:]   (ct = 0, 1: the wave's 16 x 32 strip of a score tile; contraction over dp)
__device__ __forceinline__ void tl_nt(tl_f32x4 (&acc)[2], const float* __restrict__ A, const float* __restrict__ Bm, const int pd, const int dp,
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
    acc[0] = TL_MFMA(a.x, x.x, acc[0]); acc[1] = TL_MFMA(a.x, y.x, acc[1]);
    acc[0] = TL_MFMA(a.y, x.y, acc[0]); acc[1] = TL_MFMA(a.y, y.y, acc[1]);
    acc[0] = TL_MFMA(a.z, x.z, acc[0]); acc[1] = TL_MFMA(a.z, y.z, acc[1]);
    acc[0] = TL_MFMA(a.w, x.w, acc[0]); acc[1] = TL_MFMA(a.w, y.w, acc[1]);
    a = an; x = xn; y = yn;
  }
}

// The four raw products of one tile for this wave's strip: S0 = Q K^T, GP = gO V^T, T = aQ K^T + Q aK^T, W = gO aV^T (unscaled).
struct TlRaw {
  tl_f32x4 s0[2], gp[2], t[2], w[2];
};

__device__ __forceinline__ void tl_zero2(tl_f32x4 (&a)[2]) {
  a[0] = tl_f32x4{0.f, 0.f, 0.f, 0.f};
  a[1] = tl_f32x4{0.f, 0.f, 0.f, 0.f};
}

__device__ __forceinline__ void tl_raw(TlRaw& r, const float* Qs, const float* GOs, const float* AQs, const float* Ks, const float* Vs,
                                       const float* AKs, const float* AVs, const bool has_aq, const bool has_ak, const bool has_av,
                                       const int pd, const int dp, const int w, const int n, const int g) {
  tl_zero2(r.s0); tl_zero2(r.gp); tl_zero2(r.t); tl_zero2(r.w);
  tl_nt(r.s0, Qs, Ks, pd, dp, w, n, g);
  tl_nt(r.gp, GOs, Vs, pd, dp, w, n, g);
  if (has_aq) tl_nt(r.t, AQs, Ks, pd, dp, w, n, g);
  if (has_ak) tl_nt(r.t, Qs, AKs, pd, dp, w, n, g);
  if (has_av) tl_nt(r.w, GOs, AVs, pd, dp, w, n, g);
}

// Score of element (i, j) from the raw product; -inf outside L x S and above the diagonal under the causal flag.
__device__ __forceinline__ float tl_score(const float raw, const TlArgs& q, const float* __restrict__ mbase, const int i, const int j) {
  if (i >= q.L || j >= q.S || (q.causal && j > i)) return -INFINITY;
  float sc = q.scale * raw;
  if (mbase) sc += mbase[(long long)i * q.mst[2] + (long long)j * q.mst[3]];
  return sc;
}

__device__ __forceinline__ float tl_max16(float v) {   // over the sixteen lanes that hold one row
  v = fmaxf(v, __shfl_xor(v, 1));
  v = fmaxf(v, __shfl_xor(v, 2));
  v = fmaxf(v, __shfl_xor(v, 4));
  v = fmaxf(v, __shfl_xor(v, 8));
  return v;
}

__device__ __forceinline__ double tl_sum16(double v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}

// The finished statistics of the four rows 4 g + r of this lane's strip.
struct TlStats {
  float m[4];
  double il[4], D[4], E[4], R[4];   // il = 1 / l
};

// P, gS, bgP, bS of this wave's strip -> the score tiles (zeros outside L x S).  X0 may be NULL (P is not needed for dK / dV).
__device__ __forceinline__ void tl_write_scores(const TlRaw& raw, const TlStats& st, const TlArgs& q, const float* __restrict__ mbase,
                                                const bool has_t, const bool has_av, float* X0, float* X1, float* X2, float* X3,
                                                const int i0, const int j0, const int w, const int n, const int g) {
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int j = j0 + 16 * ct + n;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * w + 4 * g + r, i = i0 + row;
      float pf = 0.f, gs = 0.f, bgp = 0.f, bs = 0.f;
      if (i < q.L && j < q.S) {
        const float sc = tl_score(raw.s0[ct][r], q, mbase, i, j);
        const float mu = st.m[r] == -INFINITY ? 0.f : st.m[r];
        pf = (float)((double)expf(sc - mu) * st.il[r]);
        const double p = (double)pf;
        const double gp = (double)raw.gp[ct][r];
        const double t = has_t ? (double)(q.scale * raw.t[ct][r]) : 0.0;
        const double wv = has_av ? (double)raw.w[ct][r] : 0.0;
        const double bp = t * (gp - st.D[r]) - gp * st.E[r] + wv;
        gs = (float)(p * (gp - st.D[r]));
        bgp = (float)(p * (t - st.E[r]));
        bs = (float)(p * (bp - st.R[r]));
      }
      const int at = row * kTlPS + 16 * ct + n;
      if (X0) X0[at] = pf;
      X1[at] = gs;
      X2[at] = bgp;
      X3[at] = bs;
    }
  }
}

// acc[cb] += X[16 w + n][j] M[j][16 cb + n']     (the wave's 16 rows x dp outputs; contraction over the 32 keys of the tile)
__device__ __forceinline__ void tl_nn(tl_f32x4 (&acc)[4], const float* __restrict__ X, const float* __restrict__ M, const int pd, const int ncb,
                                      const int w, const int n, const int g) {
  const float* xr = X + (16 * w + n) * kTlPS + 4 * g;
#pragma unroll
  for (int j0 = 0; j0 < kTlBN; j0 += 16) {
    const float4 a4 = *reinterpret_cast<const float4*>(xr + j0);
    const float a[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float* mr = M + (j0 + 4 * g + c) * pd + n;
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
        if (cb < ncb) acc[cb] = TL_MFMA(a[c], mr[16 * cb], acc[cb]);
    }
  }
}

// acc += sum_i X[i][16 kb + n] M[i][16 cb + n']   (one 16 keys x 16 columns output tile; contraction over the 64 queries of the tile)
__device__ __forceinline__ void tl_tn(tl_f32x4& acc, const float* __restrict__ X, const float* __restrict__ M, const int pd, const int kb,
                                      const int cb, const int n, const int g) {
  const float* xc = X + 16 * kb + n;
  const float* mc = M + 16 * cb + n;
#pragma unroll
  for (int i0 = 0; i0 < kTlBM; i0 += 16) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + 4 * g + c;
      acc = TL_MFMA(xc[i * kTlPS], mc[i * pd], acc);
    }
  }
}

// out[(row0 + 4 g + r)][16 cb + n] = f * acc[r], rows < nrows, columns < d; `out` is the (b, h) slice, contiguous rows of d.
__device__ __forceinline__ void tl_store(float* __restrict__ out, const tl_f32x4& acc, const float f, const int row0, const int nrows, const int cb,
                                         const int d, const int n, const int g) {
  const int col = 16 * cb + n;
  if (col >= d) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + 4 * g + r;
    if (row < nrows) out[(long long)row * d + col] = f * acc[r];
  }
}

struct TlLds {
  float *Qs, *GOs, *AQs, *Ks, *Vs, *AKs, *AVs, *X0, *X1, *X2, *X3;
};

__device__ __forceinline__ TlLds tl_carve(float* base, const int pd, const bool with_p) {
  TlLds s;
  s.Qs = base;
  s.GOs = s.Qs + kTlBM * pd;
  s.AQs = s.GOs + kTlBM * pd;
  s.Ks = s.AQs + kTlBM * pd;
  s.Vs = s.Ks + kTlBN * pd;
  s.AKs = s.Vs + kTlBN * pd;
  s.AVs = s.AKs + kTlBN * pd;
  s.X1 = s.AVs + kTlBN * pd;
  s.X2 = s.X1 + kTlBM * kTlPS;
  s.X3 = s.X2 + kTlBM * kTlPS;
  s.X0 = with_p ? s.X3 + kTlBM * kTlPS : nullptr;
  return s;
}

// grid = B * H * nqt.  Block: 64 query rows.
template <int VEC, int NCB>
__global__ __launch_bounds__(kThreads) void k_attn_tiled_q(const TlArgs q) {
  extern __shared__ __attribute__((aligned(16))) float tl_lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = lane & 15, g = lane >> 4;
  constexpr int dp = 16 * NCB, pd = dp + 4;   // compile-time: every product loop unrolls, its LDS reads run ahead of the MFMAs
  const int L = q.L, S = q.S, d = q.d;
  const int bh = blockIdx.x / q.nqt, qt = blockIdx.x - bh * q.nqt;
  const int b = bh / q.H, h = bh - b * q.H;
  const int i0 = qt * kTlBM;
  const TlLds s = tl_carve(tl_lds, pd, true);
  const float* src[TL_IN];
#pragma unroll
  for (int i = 0; i < TL_IN; ++i) src[i] = q.in[i] ? q.in[i] + (b * q.st[i][0] + h * q.st[i][1]) : nullptr;
  const bool has_aq = src[TL_AQ] != nullptr, has_ak = src[TL_AK] != nullptr, has_av = src[TL_AV] != nullptr;
  const bool has_t = has_aq || has_ak;
  const float* mbase = q.mask ? q.mask + (b * q.mst[0] + h * q.mst[1]) : nullptr;
  // key tiles that hold an element on or below the diagonal for some row of this block
  int nkt = q.nkt;
  if (q.causal) {
    const int last = (i0 + kTlBM - 1 < L - 1 ? i0 + kTlBM - 1 : L - 1) / kTlBN + 1;
    nkt = last < nkt ? last : nkt;
  }

  tl_load<VEC, 4>(s.Qs, pd, dp, src[TL_Q], q.st[TL_Q][2], i0, L, d);
  tl_load<VEC, 4>(s.GOs, pd, dp, src[TL_GO], q.st[TL_GO][2], i0, L, d);
  if (has_aq) tl_load<VEC, 4>(s.AQs, pd, dp, src[TL_AQ], q.st[TL_AQ][2], i0, L, d);

  // the key tiles come through registers: the next tile's global reads are issued before the current tile's products
  TlPieces<2> pk, pv, pak, pav;
  auto fetch_keys = [&](const int j0) {
    tl_fetch<VEC, 2>(pk, dp, src[TL_K], q.st[TL_K][2], j0, S, d);
    tl_fetch<VEC, 2>(pv, dp, src[TL_V], q.st[TL_V][2], j0, S, d);
    if (has_ak) tl_fetch<VEC, 2>(pak, dp, src[TL_AK], q.st[TL_AK][2], j0, S, d);
    if (has_av) tl_fetch<VEC, 2>(pav, dp, src[TL_AV], q.st[TL_AV][2], j0, S, d);
  };
  auto put_keys = [&]() {
    tl_put<2>(s.Ks, pd, dp, pk);
    tl_put<2>(s.Vs, pd, dp, pv);
    if (has_ak) tl_put<2>(s.AKs, pd, dp, pak);
    if (has_av) tl_put<2>(s.AVs, pd, dp, pav);
  };
  fetch_keys(0);

  // (a) the online pass
  TlStats st;
  double a_l[4], a_gp[4], a_t[4], a_tgp[4], a_w[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    st.m[r] = -INFINITY;
    a_l[r] = a_gp[r] = a_t[r] = a_tgp[r] = a_w[r] = 0.0;
  }
  for (int kt = 0; kt < nkt; ++kt) {
    const int j0 = kt * kTlBN;
    __syncthreads();   // the previous tile's reads are done
    put_keys();
    __syncthreads();
    if (kt + 1 < nkt) fetch_keys(j0 + kTlBN);
    TlRaw raw;
    tl_raw(raw, s.Qs, s.GOs, s.AQs, s.Ks, s.Vs, s.AKs, s.AVs, has_aq, has_ak, has_av, pd, dp, w, n, g);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + 16 * w + 4 * g + r;
      const float sc0 = tl_score(raw.s0[0][r], q, mbase, i, j0 + n);
      const float sc1 = tl_score(raw.s0[1][r], q, mbase, i, j0 + 16 + n);
      const float m_old = st.m[r];
      const float m_new = fmaxf(m_old, tl_max16(fmaxf(sc0, sc1)));
      const float mu = m_new == -INFINITY ? 0.f : m_new;
      if (m_old != -INFINITY && m_new != m_old) {   // (while the maximum is -inf the sums are empty: nothing to rescale)
        const double f = (double)expf(m_old - m_new);
        a_l[r] *= f; a_gp[r] *= f; a_t[r] *= f; a_tgp[r] *= f; a_w[r] *= f;
      }
      st.m[r] = m_new;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const double e = (double)expf((ct ? sc1 : sc0) - mu);
        const double gp = (double)raw.gp[ct][r];
        const double t = has_t ? (double)(q.scale * raw.t[ct][r]) : 0.0;
        const double wv = has_av ? (double)raw.w[ct][r] : 0.0;
        a_l[r] += e;
        a_gp[r] += e * gp;
        a_t[r] += e * t;
        a_tgp[r] += e * (t * gp);
        a_w[r] += e * wv;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double l = tl_sum16(a_l[r]);
    const double D = tl_sum16(a_gp[r]) / l, E = tl_sum16(a_t[r]) / l;
    const double R = tl_sum16(a_tgp[r]) / l - 2.0 * D * E + tl_sum16(a_w[r]) / l;
    st.il[r] = 1.0 / l; st.D[r] = D; st.E[r] = E; st.R[r] = R;
    const int i = i0 + 16 * w + 4 * g + r;
    if (n == 0 && i < L) {
      double* o = q.ws + ((long long)bh * L + i) * kTlStats;
      o[0] = (double)st.m[r]; o[1] = l; o[2] = D; o[3] = E; o[4] = R;
    }
  }

  // (b) dQ and dgO
  float* const dq = q.out[TL_DQ] ? q.out[TL_DQ] + (long long)bh * L * d : nullptr;
  float* const dgo = q.out[TL_DGO] ? q.out[TL_DGO] + (long long)bh * L * d : nullptr;
  if (!dq && !dgo) return;   // uniform over the grid
  constexpr int ncb = NCB;
  tl_f32x4 acc_q[4], acc_o[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) acc_q[cb] = acc_o[cb] = tl_f32x4{0.f, 0.f, 0.f, 0.f};
  fetch_keys(0);
  for (int kt = 0; kt < nkt; ++kt) {
    const int j0 = kt * kTlBN;
    __syncthreads();
    put_keys();
    __syncthreads();
    if (kt + 1 < nkt) fetch_keys(j0 + kTlBN);
    TlRaw raw;
    tl_raw(raw, s.Qs, s.GOs, s.AQs, s.Ks, s.Vs, s.AKs, s.AVs, has_aq, has_ak, has_av, pd, dp, w, n, g);
    tl_write_scores(raw, st, q, mbase, has_t, has_av, s.X0, s.X1, s.X2, s.X3, i0, j0, w, n, g);
    __syncthreads();
    if (dq) {
      tl_nn(acc_q, s.X3, s.Ks, pd, ncb, w, n, g);
      if (has_ak) tl_nn(acc_q, s.X1, s.AKs, pd, ncb, w, n, g);
    }
    if (dgo) {
      if (has_t) tl_nn(acc_o, s.X2, s.Vs, pd, ncb, w, n, g);
      if (has_av) tl_nn(acc_o, s.X0, s.AVs, pd, ncb, w, n, g);
    }
  }
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    if (cb >= ncb) break;
    if (dq) tl_store(dq, acc_q[cb], q.scale, i0 + 16 * w, L, cb, d, n, g);
    if (dgo) tl_store(dgo, acc_o[cb], 1.f, i0 + 16 * w, L, cb, d, n, g);
  }
}

// grid = B * H * nkt.  Block: 32 keys.
template <int VEC, int NCB>
__global__ __launch_bounds__(kThreads) void k_attn_tiled_k(const TlArgs q) {
  extern __shared__ __attribute__((aligned(16))) float tl_lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = lane & 15, g = lane >> 4;
  constexpr int dp = 16 * NCB, pd = dp + 4;   // compile-time: every product loop unrolls, its LDS reads run ahead of the MFMAs
  const int L = q.L, S = q.S, d = q.d;
  const int bh = blockIdx.x / q.nkt, kt = blockIdx.x - bh * q.nkt;
  const int b = bh / q.H, h = bh - b * q.H;
  const int j0 = kt * kTlBN;
  const TlLds s = tl_carve(tl_lds, pd, false);
  const float* src[TL_IN];
#pragma unroll
  for (int i = 0; i < TL_IN; ++i) src[i] = q.in[i] ? q.in[i] + (b * q.st[i][0] + h * q.st[i][1]) : nullptr;
  const bool has_aq = src[TL_AQ] != nullptr, has_ak = src[TL_AK] != nullptr, has_av = src[TL_AV] != nullptr;
  const bool has_t = has_aq || has_ak;
  const float* mbase = q.mask ? q.mask + (b * q.mst[0] + h * q.mst[1]) : nullptr;
  float* const dk = q.out[TL_DK] ? q.out[TL_DK] + (long long)bh * S * d : nullptr;
  float* const dv = q.out[TL_DV] ? q.out[TL_DV] + (long long)bh * S * d : nullptr;
  const int qt0 = q.causal ? j0 / kTlBM : 0;   // query tiles above hold only rows i < j0: wholly above the diagonal
  // the wave's output tiles t = w and w + 4 of the 2 (key blocks) x ncb (column blocks) grid
  constexpr int ntile = 2 * NCB;
  tl_f32x4 acc_k[2], acc_v[2];
  tl_zero2(acc_k); tl_zero2(acc_v);

  tl_load<VEC, 2>(s.Ks, pd, dp, src[TL_K], q.st[TL_K][2], j0, S, d);
  tl_load<VEC, 2>(s.Vs, pd, dp, src[TL_V], q.st[TL_V][2], j0, S, d);
  if (has_ak) tl_load<VEC, 2>(s.AKs, pd, dp, src[TL_AK], q.st[TL_AK][2], j0, S, d);
  if (has_av) tl_load<VEC, 2>(s.AVs, pd, dp, src[TL_AV], q.st[TL_AV][2], j0, S, d);
  // the query tiles come through registers: the next tile's global reads are issued before the current tile's products
  TlPieces<4> pq, pgo, paq;
  auto fetch_queries = [&](const int i0) {
    tl_fetch<VEC, 4>(pq, dp, src[TL_Q], q.st[TL_Q][2], i0, L, d);
    tl_fetch<VEC, 4>(pgo, dp, src[TL_GO], q.st[TL_GO][2], i0, L, d);
    if (has_aq) tl_fetch<VEC, 4>(paq, dp, src[TL_AQ], q.st[TL_AQ][2], i0, L, d);
  };
  if (qt0 < q.nqt) fetch_queries(qt0 * kTlBM);
  for (int qt = qt0; qt < q.nqt; ++qt) {
    const int i0 = qt * kTlBM;
    __syncthreads();
    tl_put<4>(s.Qs, pd, dp, pq);
    tl_put<4>(s.GOs, pd, dp, pgo);
    if (has_aq) tl_put<4>(s.AQs, pd, dp, paq);
    TlStats st;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + 16 * w + 4 * g + r;
      st.m[r] = 0.f; st.il[r] = 1.0; st.D[r] = st.E[r] = st.R[r] = 0.0;
      if (i < L) {
        const double* o = q.ws + ((long long)bh * L + i) * kTlStats;
        st.m[r] = (float)o[0]; st.il[r] = 1.0 / o[1]; st.D[r] = o[2]; st.E[r] = o[3]; st.R[r] = o[4];
      }
    }
    __syncthreads();
    if (qt + 1 < q.nqt) fetch_queries(i0 + kTlBM);
    TlRaw raw;
    tl_raw(raw, s.Qs, s.GOs, s.AQs, s.Ks, s.Vs, s.AKs, s.AVs, has_aq, has_ak, has_av, pd, dp, w, n, g);
    tl_write_scores(raw, st, q, mbase, has_t, has_av, nullptr, s.X1, s.X2, s.X3, i0, j0, w, n, g);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int t = w + 4 * u;
      if (t >= ntile) break;
      const int kb = t & 1, cb = t >> 1;
      if (dv && has_t) tl_tn(acc_v[u], s.X2, s.GOs, pd, kb, cb, n, g);
      if (dk) {
        tl_tn(acc_k[u], s.X3, s.Qs, pd, kb, cb, n, g);
        if (has_aq) tl_tn(acc_k[u], s.X1, s.AQs, pd, kb, cb, n, g);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int t = w + 4 * u;
    if (t >= ntile) break;
    const int kb = t & 1, cb = t >> 1;
    if (dk) tl_store(dk, acc_k[u], q.scale, j0 + 16 * kb, S, cb, d, n, g);
    if (dv) tl_store(dv, acc_v[u], 1.f, j0 + 16 * kb, S, cb, d, n, g);
  }
}

// Why the launch does not take a shape, or NULL where it does: the launch, the plan and the workspace size refuse the same shapes.
// (The refusal is at 2^31 - 1 workgroups, the limit of gridDim.x.  The runtime itself rejects a launch whose gridDim.x * blockDim.x
// reaches 2^32 — 2^24 workgroups of 256 threads, B H >= 2^21 at 512 queries — and that comes back as a HIP error from the launch, not
// as this refusal; the same holds for bhg_attention_backward_vjp.)
inline const char* tl_shape_error(int B, int H, int L, int S, int d) {
  if (!(B > 0 && H > 0 && L > 0 && S > 0 && d > 0)) return "empty tensor";
  if (L > kTlMaxLen) return "more than 512 queries";
  if (S > kTlMaxLen) return "more than 512 keys";
  if (d > kTlMaxD) return "more than 64 elements per head";
  const long long bh = (long long)B * H;
  if (bh * ((L + kTlBM - 1) / kTlBM) > 0x7fffffffLL || bh * ((S + kTlBN - 1) / kTlBN) > 0x7fffffffLL)
    return "a grid of more than 2^31 - 1 workgroups";
  return nullptr;
}

inline size_t tl_ws_bytes(int B, int H, int L) { return (size_t)B * H * L * kTlStats * sizeof(double); }

// Shape -> tiles, pitches and LDS bytes.  Operand tiles: three of 64 rows (Q, gO, aQ) and four of 32 rows (K, V, aK, aV) at pitch
// pd = dp + 4, an odd number of 16-byte units (the sixteen rows of one 16-byte fragment read lie on sixteen different bank groups).
// Score tiles: 64 x 32 at pitch 36; four for the query launch (P, gS, bgP, bS), three for the key launch (no P).
inline const char* tl_plan(TlArgs* q, int B, int H, int L, int S, int d, int vec_ok) {
  const char* bad = tl_shape_error(B, H, L, S, d);
  if (bad) return bad;
  q->B = B; q->H = H; q->L = L; q->S = S; q->d = d;
  q->vec = (d % 4 == 0 && vec_ok) ? 4 : 1;
  q->dp = (d + 15) / 16 * 16;
  q->pd = q->dp + 4;
  q->nqt = (L + kTlBM - 1) / kTlBM;
  q->nkt = (S + kTlBN - 1) / kTlBN;
  const int operands = (3 * kTlBM + 4 * kTlBN) * q->pd;
  q->lds_q = (int)sizeof(float) * (operands + 4 * kTlBM * kTlPS);
  q->lds_k = (int)sizeof(float) * (operands + 3 * kTlBM * kTlPS);
  if (q->lds_q > kTlMaxLds) return "the plan needs more than 160 KiB of LDS";   // cannot happen for d <= 64 (123904)
  return nullptr;
}

inline long long tl_stride(const long long* st, int i, int extent) { return extent > 1 ? st[i] : 0; }

#undef TL_MFMA

}  // namespace
}  // namespace bhg

using namespace bhg;

extern "C" {

size_t bhg_attention_tiled_ws_bytes(int B, int H, int L) {
  if (!(B > 0 && H > 0 && L > 0)) return 0;
  return tl_ws_bytes(B, H, L);
}

int bhg_attention_tiled_plan(int B, int H, int L, int S, int d, int vec_ok, char* buf, size_t buf_bytes) {
  BHG_REQUIRE(buf && buf_bytes > 0, "NULL buffer");
  TlArgs q{};
  const char* bad = tl_plan(&q, B, H, L, S, d, vec_ok);
  BHG_REQUIRE(!bad, bad);
  const int len = snprintf(buf, buf_bytes,
                           "vec=%d bm=%d bn=%d dp=%d pd=%d ps=%d grid_q=%lld grid_k=%lld lds_q=%d lds_k=%d max_lds=%d ws=%llu", q.vec, kTlBM,
                           kTlBN, q.dp, q.pd, kTlPS, (long long)B * H * q.nqt, (long long)B * H * q.nkt, q.lds_q, q.lds_k, kTlMaxLds,
                           (unsigned long long)tl_ws_bytes(B, H, L));
  BHG_REQUIRE(len > 0 && (size_t)len < buf_bytes, "buffer too small for the plan line");
  return BHG_OK;
}

int bhg_attention_tiled_backward_vjp(const float* q, const float* k, const float* v, const float* go, const float* aq, const float* ak,
                                     const float* av, const long long* strides, const float* mask, const long long* mask_strides, int causal,
                                     float scale, int B, int H, int L, int S, int d, float* dq, float* dk, float* dv, float* dgo, void* ws,
                                     size_t ws_bytes, void* stream) {
  TlArgs a{};
  {
    const char* bad = tl_shape_error(B, H, L, S, d);
    BHG_REQUIRE(!bad, bad);
  }
  BHG_REQUIRE(q && k && v && go, "null pointer (q, k, v and go are required)");
  BHG_REQUIRE(aq || ak || av, "all three cotangents are NULL");
  BHG_REQUIRE(dq || dk || dv || dgo, "all four outputs are NULL");
  BHG_REQUIRE(strides, "null pointer (strides)");
  BHG_REQUIRE(!mask || mask_strides, "null pointer (mask_strides)");
  BHG_REQUIRE(ws, "null pointer (workspace)");
  BHG_REQUIRE(ws_bytes >= tl_ws_bytes(B, H, L), "workspace too small (bhg_attention_tiled_ws_bytes)");
  BHG_REQUIRE(((uintptr_t)ws & 7) == 0, "the workspace must be 8-byte aligned");
  const float* in[TL_IN] = {q, k, v, go, aq, ak, av};
  const int rows_of[TL_IN] = {L, S, S, L, L, S, S};
  int vec_ok = 1;
  for (int i = 0; i < TL_IN; ++i) {
    a.in[i] = in[i];
    const long long* st = strides + 4 * i;
    BHG_REQUIRE(!in[i] || d == 1 || st[3] == 1, "the last stride of every input must be 1");
    a.st[i][0] = tl_stride(st, 0, B); a.st[i][1] = tl_stride(st, 1, H); a.st[i][2] = tl_stride(st, 2, rows_of[i]);
    if (!in[i]) continue;
    for (int j = 0; j < 3; ++j) {
      BHG_REQUIRE(a.st[i][j] >= 0, "negative stride");
      if (a.st[i][j] % 4 != 0) vec_ok = 0;
    }
  }
  const char* bad = tl_plan(&a, B, H, L, S, d, vec_ok);
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
      a.mst[j] = tl_stride(mask_strides, j, ext[j]);
      BHG_REQUIRE(a.mst[j] >= 0, "negative stride");
    }
  }
  a.out[TL_DQ] = dq; a.out[TL_DK] = dk; a.out[TL_DV] = dv; a.out[TL_DGO] = dgo;
  a.ws = static_cast<double*>(ws);
  a.causal = causal != 0;
  a.scale = scale;
  // above 64 KiB a kernel's dynamic LDS has to be allowed, once per process and device
  static bool attr_done[64] = {};
  int dev = 0;
  BHG_HIP_CHECK(hipGetDevice(&dev));
  using Kernel = void (*)(const TlArgs);
  static const Kernel kq[2][4] = {{k_attn_tiled_q<1, 1>, k_attn_tiled_q<1, 2>, k_attn_tiled_q<1, 3>, k_attn_tiled_q<1, 4>},
                                  {k_attn_tiled_q<4, 1>, k_attn_tiled_q<4, 2>, k_attn_tiled_q<4, 3>, k_attn_tiled_q<4, 4>}};
  static const Kernel kk[2][4] = {{k_attn_tiled_k<1, 1>, k_attn_tiled_k<1, 2>, k_attn_tiled_k<1, 3>, k_attn_tiled_k<1, 4>},
                                  {k_attn_tiled_k<4, 1>, k_attn_tiled_k<4, 2>, k_attn_tiled_k<4, 3>, k_attn_tiled_k<4, 4>}};
  if (dev < 0 || dev >= 64 || !attr_done[dev]) {
    for (int i = 0; i < 2; ++i)
      for (int j = 0; j < 4; ++j) {
        BHG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kq[i][j]), hipFuncAttributeMaxDynamicSharedMemorySize, kTlMaxLds));
        BHG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kk[i][j]), hipFuncAttributeMaxDynamicSharedMemorySize, kTlMaxLds));
      }
    if (dev >= 0 && dev < 64) attr_done[dev] = true;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned grid_q = (unsigned)((long long)B * H * a.nqt), grid_k = (unsigned)((long long)B * H * a.nkt);
  const int vi = a.vec == 4 ? 1 : 0, ci = a.dp / 16 - 1;   // the instance: global read width, d rounded up to 16
  hipLaunchKernelGGL(kq[vi][ci], dim3(grid_q), dim3(kThreads), a.lds_q, st, a);
  BHG_HIP_CHECK(hipGetLastError());
  if (dk || dv) {
    hipLaunchKernelGGL(kk[vi][ci], dim3(grid_k), dim3(kThreads), a.lds_k, st, a);
    BHG_HIP_CHECK(hipGetLastError());
  }
  return BHG_OK;
}

}  // extern "C"
