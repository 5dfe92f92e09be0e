// bhg_attention_gqa.hip — the Hessian-vector product's share of an attention core with GROUPED-QUERY heads: Hq = g Hkv query heads, query
// head h reading key/value head h / g (torch's enable_gqa, i.e. repeat_interleave(g, dim = 1)), for 1 <= L, S <= 512, 1 <= d <= 64,
// g >= 2 and g L <= 4096.  The sibling of bhg_attention_tiled.hip: the same quantities, notation, tiles and arithmetic,
//     P = softmax_rows(s Q K^T + m)     gP = gO V^T     D = rowsum(P * gP)     gS = P * (gP - D)
//     T = s (aQ K^T + Q aK^T)           E = rowsum(P * T)                      bgP = P * (T - E)
//     bP = T * (gP - D) - gP * E + gO aV^T              R = rowsum(P * bP)     bS = P * (bP - R)
//     dgO = bgP V + P aV     dV = bgP^T gO     dQ = s (bS K + gS aK)     dK = s (bS^T Q + gS^T aQ)
// with q, go, aq of shape (B, Hq, L, d) and k, v, ak, av of shape (B, Hkv, S, d); dK and dV are summed over the g query heads of a group.
//
// THE GROUP IS PACKED INTO THE QUERY ROWS.  Within one (batch, kv head) the g query heads share K and V, so they are ONE attention with
// g L query rows: packed row r = j L + i is row i of query head g kvh + j.  Everything below works on packed rows:
//   k_attn_gqa_q   grid B Hkv ceil(g L / 64): a block owns 64 PACKED rows (Q, gO, aQ resident in LDS) and sweeps the key tiles twice, as
//       the sibling does: (a) the online pass for m, l, D, E, R (fp64 sums in registers, rescaled when the running maximum moves; the
//       statistics go to the workspace), (b) the second sweep that forms P, gS, bgP, bS per tile and accumulates dQ and dgO in registers.
//       A 64-row tile may span several query heads — g = 8, L = 20 is 3 tiles where head-by-head launches have 8 quarter-empty ones.
//   k_attn_gqa_k   grid B Hkv ceil(S / 32): a block owns 32 keys (K, V, aK, aV resident, loaded ONCE per group), sweeps all
//       ceil(g L / 64) packed query tiles with the statistics read from the workspace, and accumulates dK and dV in registers over the
//       whole group: no atomics, no g-fold partial results, no reduction pass, bitwise repeatable.  Not launched when both are NULL.
// What packing changes against the sibling, and nothing else does:
//   * a packed row's global address is two-level, head = g kvh + r / L and row = r % L, each with its own stride ((Hq, L) need not be
//     contiguous: the common input is a transposed view of (B, L, Hq, d)); the loaders split r once per 16-byte piece;
//   * the mask element of a packed row is taken at (b, head, row, .);
//   * the causal bound of a packed row is its `row`, not r; a query tile's skip bound is the largest `row` among its packed rows, which
//     is L - 1 as soon as the tile crosses a head boundary; the key launch therefore tests every packed tile (they are not monotone);
//   * dq, dgo (B, Hq, L, d) contiguous ARE (B, Hkv, g L, d): packed rows store contiguously, and so do their statistics in the workspace
//     (B Hq L rows of five doubles m, l, D, E, R: the sibling's layout, 40 bytes per query row).
// Fully masked rows end with m = -inf, l = 0: P = 0, D = E = R = 0, exact zeros in their rows of dq and dgo (as in the sibling).
//
// Every product runs on the fp32-input MFMA v_mfma_f32_16x16x4_f32 (exact fp32).  Lane (n = lane & 15, g4 = lane >> 4) supplies A[n][k]
// and B[k][n] with k = 4 g4 + c at step c, so a lane's four A values are one 16-byte LDS read.  Operand tiles are zero-padded in LDS to
// the tile shape (rows past g L / S, columns past d up to dp = d rounded up to 16) at pitch dp + 4; score tiles are 64 x 32 at pitch 36.
// Instantiated per dp / 16 = 1 .. 4 and per global read width.  The LDS plan is the sibling's: 123904 bytes at dp = 64.
//
// Layout: fp32.  Inputs with four element strides each (last stride 1), read in place; outputs contiguous.  vec = 4 (16-byte global
// reads) when d % 4 == 0 and every stride of a present input is a multiple of 4; otherwise scalar reads.
#include "bhg_common.hpp"

#include <math.h>

namespace bhg {
namespace {

typedef float gq_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kGqMaxLen = 512, kGqMaxD = 64, kGqMaxRows = 4096;
constexpr int kGqBM = 64, kGqBN = 32;      // packed query rows and keys of one score tile
constexpr int kGqPS = kGqBN + 4;           // row pitch of a score tile: 9 x 16 bytes
constexpr int kGqStats = 5;                // doubles per query row in the workspace: m l D E R
constexpr int kGqMaxLds = 160 * 1024;
enum { GQ_Q = 0, GQ_K, GQ_V, GQ_GO, GQ_AQ, GQ_AK, GQ_AV, GQ_IN };
enum { GQ_DQ = 0, GQ_DK, GQ_DV, GQ_DGO, GQ_OUT };

struct GqArgs {
  const float* in[GQ_IN];      // q k v go aq ak av; the last three may be NULL
  long long st[GQ_IN][3];      // element strides: batch, head (query head for q go aq, kv head for the others), row
  const float* mask;           // may be NULL
  long long mst[4];            // element strides of the mask viewed as (B, Hq, L, S) (0 = broadcast)
  float* out[GQ_OUT];          // dq dk dv dgo, contiguous; each may be NULL
  double* ws;                  // B Hq L x 5
  int B, Hq, Hkv, G, L, S, d;
  int rows;                    // G * L: packed query rows of one (batch, kv head)
  int causal;
  float scale;
  int vec;                     // 4: 16-byte global reads; 1: scalar
  int dp, pd;                  // d rounded up to 16; row pitch of an operand tile
  int nqt, nkt;                // packed query tiles of 64, key tiles of 32
  int lds_q, lds_k;            // bytes of dynamic LDS of the two launches
};

// This thread's NPT 16-byte pieces of a tile of NPT * 16 rows x dp floats (256 threads: NPT = 2 for 32 rows, 4 for 64).
template <int NPT>
struct GqPieces {
  float4 v[NPT];
};

// Where the rows of this thread's pieces of a PACKED tile lie: query head within the group and row within the head; hd < 0: no such row.
template <int NPT>
struct GqPieceRows {
  int hd[NPT], rw[NPT];
};

template <int NPT>
__device__ __forceinline__ void gq_piece_rows(GqPieceRows<NPT>& pr, const int dp, const int row0, const int rows, const int L) {
  const int nv = dp >> 2, n = NPT * (kThreads / 16) * nv;
#pragma unroll
  for (int u = 0; u < NPT; ++u) {
    const int idx = threadIdx.x + u * kThreads;
    const int p = row0 + idx / nv;
    pr.hd[u] = -1; pr.rw[u] = 0;
    if (idx < n && p < rows) {
      pr.hd[u] = p / L;
      pr.rw[u] = p - pr.hd[u] * L;
    }
  }
}

__device__ __forceinline__ float4 gq_read4(const float* __restrict__ g, const int c, const int d, const bool vec) {
  float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
  if (vec) {
    t = *reinterpret_cast<const float4*>(g);
  } else {
    t.x = g[0];
    if (c + 1 < d) t.y = g[1];
    if (c + 2 < d) t.z = g[2];
    if (c + 3 < d) t.w = g[3];
  }
  return t;
}

// Global -> registers, packed query rows: `src` is the (batch, first query head of the group) slice, hs / rs its head and row strides.
template <int VEC, int NPT>
__device__ __forceinline__ void gq_fetch_packed(GqPieces<NPT>& p, const int dp, const float* __restrict__ src, const long long hs,
                                                const long long rs, const GqPieceRows<NPT>& pr, const int d) {
  const int nv = dp >> 2;
#pragma unroll
  for (int u = 0; u < NPT; ++u) {
    const int idx = threadIdx.x + u * kThreads;
    const int c = (idx - (idx / nv) * nv) << 2;
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (pr.hd[u] >= 0 && c < d) t = gq_read4(src + pr.hd[u] * hs + pr.rw[u] * rs + c, c, d, VEC == 4);
    p.v[u] = t;
  }
}

// Global -> registers, keys: rows row0 .. of the S x d matrix at src (row stride rs), zeros outside.
template <int VEC, int NPT>
__device__ __forceinline__ void gq_fetch(GqPieces<NPT>& p, const int dp, const float* __restrict__ src, const long long rs, const int row0,
                                         const int nrows, const int d) {
  const int nv = dp >> 2, n = NPT * (kThreads / 16) * nv;
#pragma unroll
  for (int u = 0; u < NPT; ++u) {
    const int idx = threadIdx.x + u * kThreads;
    const int r = idx / nv, c = (idx - r * nv) << 2;
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (idx < n && row0 + r < nrows && c < d) t = gq_read4(src + (long long)(row0 + r) * rs + c, c, d, VEC == 4);
    p.v[u] = t;
  }
}

template <int NPT>
__device__ __forceinline__ void gq_put(float* __restrict__ dst, const int pd, const int dp, const GqPieces<NPT>& p) {
  const int nv = dp >> 2, n = NPT * (kThreads / 16) * nv;
#pragma unroll
  for (int u = 0; u < NPT; ++u) {
    const int idx = threadIdx.x + u * kThreads;
    const int r = idx / nv, c = (idx - r * nv) << 2;
    if (idx < n) *reinterpret_cast<float4*>(dst + r * pd + c) = p.v[u];
  }
}

#define GQ_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// acc[ct] += A[16 w + n][:] . Bm[16 ct + n'][:]   (ct = 0, 1: the wave's 16 x 32 strip of a score tile; contraction over dp)
__device__ __forceinline__ void gq_nt(gq_f32x4 (&acc)[2], const float* __restrict__ A, const float* __restrict__ Bm, const int pd, const int dp,
                                      const int w, const int n, const int g4) {
  const float* ar = A + (16 * w + n) * pd + 4 * g4;
  const float* b0 = Bm + n * pd + 4 * g4;
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
    acc[0] = GQ_MFMA(a.x, x.x, acc[0]); acc[1] = GQ_MFMA(a.x, y.x, acc[1]);
    acc[0] = GQ_MFMA(a.y, x.y, acc[0]); acc[1] = GQ_MFMA(a.y, y.y, acc[1]);
    acc[0] = GQ_MFMA(a.z, x.z, acc[0]); acc[1] = GQ_MFMA(a.z, y.z, acc[1]);
    acc[0] = GQ_MFMA(a.w, x.w, acc[0]); acc[1] = GQ_MFMA(a.w, y.w, acc[1]);
    a = an; x = xn; y = yn;
  }
}

// The four raw products of one tile for this wave's strip: S0 = Q K^T, GP = gO V^T, T = aQ K^T + Q aK^T, W = gO aV^T (unscaled).
struct GqRaw {
  gq_f32x4 s0[2], gp[2], t[2], w[2];
};

__device__ __forceinline__ void gq_zero2(gq_f32x4 (&a)[2]) {
  a[0] = gq_f32x4{0.f, 0.f, 0.f, 0.f};
  a[1] = gq_f32x4{0.f, 0.f, 0.f, 0.f};
}

struct GqLds {
  float *Qs, *GOs, *AQs, *Ks, *Vs, *AKs, *AVs, *X0, *X1, *X2, *X3;
};

__device__ __forceinline__ GqLds gq_carve(float* base, const int pd, const bool with_p) {
  GqLds s;
  s.Qs = base;
  s.GOs = s.Qs + kGqBM * pd;
  s.AQs = s.GOs + kGqBM * pd;
  s.Ks = s.AQs + kGqBM * pd;
  s.Vs = s.Ks + kGqBN * pd;
  s.AKs = s.Vs + kGqBN * pd;
  s.AVs = s.AKs + kGqBN * pd;
  s.X1 = s.AVs + kGqBN * pd;
  s.X2 = s.X1 + kGqBM * kGqPS;
  s.X3 = s.X2 + kGqBM * kGqPS;
  s.X0 = with_p ? s.X3 + kGqBM * kGqPS : nullptr;
  return s;
}

__device__ __forceinline__ void gq_raw(GqRaw& r, const GqLds& s, const bool has_aq, const bool has_ak, const bool has_av, const int pd,
                                       const int dp, const int w, const int n, const int g4) {
  gq_zero2(r.s0); gq_zero2(r.gp); gq_zero2(r.t); gq_zero2(r.w);
  gq_nt(r.s0, s.Qs, s.Ks, pd, dp, w, n, g4);
  gq_nt(r.gp, s.GOs, s.Vs, pd, dp, w, n, g4);
  if (has_aq) gq_nt(r.t, s.AQs, s.Ks, pd, dp, w, n, g4);
  if (has_ak) gq_nt(r.t, s.Qs, s.AKs, pd, dp, w, n, g4);
  if (has_av) gq_nt(r.w, s.GOs, s.AVs, pd, dp, w, n, g4);
}

// The lane's four packed rows 16 w + 4 g4 + r of a tile, unpacked: row within its head (-1: past g L) and, with a mask, the mask's row
// (b, head, row, 0).  Four consecutive packed rows: one division, then steps.
struct GqRows {
  int rw[4];
  const float* m[4];
};

__device__ __forceinline__ void gq_rows(GqRows& o, const GqArgs& q, const float* __restrict__ mgroup, const int p0) {
  int hd = p0 / q.L, rw = p0 - hd * q.L;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const bool in = p0 + r < q.rows;
    o.rw[r] = in ? rw : -1;
    o.m[r] = (mgroup && in) ? mgroup + hd * q.mst[1] + rw * q.mst[2] : nullptr;
    if (++rw == q.L) { rw = 0; ++hd; }
  }
}

// Score of (packed row with in-head row rw, key j) from the raw product; -inf outside g L x S and above the diagonal of ITS head.
__device__ __forceinline__ float gq_score(const float raw, const GqArgs& q, const float* __restrict__ mrow, const int rw, const int j) {
  if (rw < 0 || j >= q.S || (q.causal && j > rw)) return -INFINITY;
  float sc = q.scale * raw;
  if (mrow) sc += mrow[(long long)j * q.mst[3]];
  return sc;
}

// The largest in-head row among the packed rows row0 .. row0 + 63: the causal skip bound of a packed query tile.
__device__ __forceinline__ int gq_tile_max_row(const int row0, const int rows, const int L) {
  const int last = row0 + kGqBM - 1 < rows - 1 ? row0 + kGqBM - 1 : rows - 1;
  const int h0 = row0 / L, h1 = last / L;
  return h0 == h1 ? last - h1 * L : L - 1;
}

__device__ __forceinline__ float gq_max16(float v) {   // over the sixteen lanes that hold one row
  v = fmaxf(v, __shfl_xor(v, 1));
  v = fmaxf(v, __shfl_xor(v, 2));
  v = fmaxf(v, __shfl_xor(v, 4));
  v = fmaxf(v, __shfl_xor(v, 8));
  return v;
}

__device__ __forceinline__ double gq_sum16(double v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}

// The finished statistics of the four rows 4 g4 + r of this lane's strip.
struct GqStats {
  float m[4];
  double il[4], D[4], E[4], R[4];   // il = 1 / l
};

// P, gS, bgP, bS of this wave's strip -> the score tiles (zeros outside g L x S).  X0 may be NULL (P is not needed for dK / dV).
__device__ __forceinline__ void gq_write_scores(const GqRaw& raw, const GqStats& st, const GqArgs& q, const GqRows& rows, const bool has_t,
                                                const bool has_av, float* X0, float* X1, float* X2, float* X3, const int j0, const int w,
                                                const int n, const int g4) {
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int j = j0 + 16 * ct + n;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * w + 4 * g4 + r;
      float pf = 0.f, gs = 0.f, bgp = 0.f, bs = 0.f;
      if (rows.rw[r] >= 0 && j < q.S) {
        const float sc = gq_score(raw.s0[ct][r], q, rows.m[r], rows.rw[r], j);
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
      const int at = row * kGqPS + 16 * ct + n;
      if (X0) X0[at] = pf;
      X1[at] = gs;
      X2[at] = bgp;
      X3[at] = bs;
    }
  }
}

// acc[cb] += X[16 w + n][j] M[j][16 cb + n']     (the wave's 16 rows x dp outputs; contraction over the 32 keys of the tile)
__device__ __forceinline__ void gq_nn(gq_f32x4 (&acc)[4], const float* __restrict__ X, const float* __restrict__ M, const int pd, const int ncb,
                                      const int w, const int n, const int g4) {
  const float* xr = X + (16 * w + n) * kGqPS + 4 * g4;
#pragma unroll
  for (int j0 = 0; j0 < kGqBN; j0 += 16) {
    const float4 a4 = *reinterpret_cast<const float4*>(xr + j0);
    const float a[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float* mr = M + (j0 + 4 * g4 + c) * pd + n;
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
        if (cb < ncb) acc[cb] = GQ_MFMA(a[c], mr[16 * cb], acc[cb]);
    }
  }
}

// acc += sum_i X[i][16 kb + n] M[i][16 cb + n']   (one 16 keys x 16 columns output tile; contraction over the 64 packed rows of the tile)
__device__ __forceinline__ void gq_tn(gq_f32x4& acc, const float* __restrict__ X, const float* __restrict__ M, const int pd, const int kb,
                                      const int cb, const int n, const int g4) {
  const float* xc = X + 16 * kb + n;
  const float* mc = M + 16 * cb + n;
#pragma unroll
  for (int i0 = 0; i0 < kGqBM; i0 += 16) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + 4 * g4 + c;
      acc = GQ_MFMA(xc[i * kGqPS], mc[i * pd], acc);
    }
  }
}

// out[(row0 + 4 g4 + r)][16 cb + n] = f * acc[r], rows < nrows, columns < d; `out` is a contiguous nrows x d slice.
__device__ __forceinline__ void gq_store(float* __restrict__ out, const gq_f32x4& acc, const float f, const int row0, const int nrows, const int cb,
                                         const int d, const int n, const int g4) {
  const int col = 16 * cb + n;
  if (col >= d) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + 4 * g4 + r;
    if (row < nrows) out[(long long)row * d + col] = f * acc[r];
  }
}

// The (batch, kv head) slices of the seven inputs: the first query head of the group for q, go, aq.
__device__ __forceinline__ void gq_sources(const float* (&src)[GQ_IN], const GqArgs& q, const int b, const int kvh) {
#pragma unroll
  for (int i = 0; i < GQ_IN; ++i) {
    const bool packed = i == GQ_Q || i == GQ_GO || i == GQ_AQ;
    src[i] = q.in[i] ? q.in[i] + (b * q.st[i][0] + (long long)(packed ? q.G * kvh : kvh) * q.st[i][1]) : nullptr;
  }
}

// grid = B * Hkv * nqt.  Block: 64 packed query rows.
template <int VEC, int NCB>
__global__ __launch_bounds__(kThreads) void k_attn_gqa_q(const GqArgs q) {
  extern __shared__ __attribute__((aligned(16))) float gq_lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = lane & 15, g4 = lane >> 4;
  constexpr int dp = 16 * NCB, pd = dp + 4;   // compile-time: every product loop unrolls, its LDS reads run ahead of the MFMAs
  const int L = q.L, S = q.S, d = q.d, rows = q.rows;
  const int bk = blockIdx.x / q.nqt, qt = blockIdx.x - bk * q.nqt;
  const int b = bk / q.Hkv, kvh = bk - b * q.Hkv;
  const int r0 = qt * kGqBM;
  const GqLds s = gq_carve(gq_lds, pd, true);
  const float* src[GQ_IN];
  gq_sources(src, q, b, kvh);
  const bool has_aq = src[GQ_AQ] != nullptr, has_ak = src[GQ_AK] != nullptr, has_av = src[GQ_AV] != nullptr;
  const bool has_t = has_aq || has_ak;
  const float* mgroup = q.mask ? q.mask + (b * q.mst[0] + (long long)q.G * kvh * q.mst[1]) : nullptr;
  GqRows mine;
  gq_rows(mine, q, mgroup, r0 + 16 * w + 4 * g4);
  // key tiles that hold an element on or below the diagonal of some packed row of this block
  int nkt = q.nkt;
  if (q.causal) {
    const int last = gq_tile_max_row(r0, rows, L) / kGqBN + 1;
    nkt = last < nkt ? last : nkt;
  }

  {
    GqPieceRows<4> pr;
    gq_piece_rows<4>(pr, dp, r0, rows, L);
    GqPieces<4> p;
    gq_fetch_packed<VEC, 4>(p, dp, src[GQ_Q], q.st[GQ_Q][1], q.st[GQ_Q][2], pr, d);
    gq_put<4>(s.Qs, pd, dp, p);
    gq_fetch_packed<VEC, 4>(p, dp, src[GQ_GO], q.st[GQ_GO][1], q.st[GQ_GO][2], pr, d);
    gq_put<4>(s.GOs, pd, dp, p);
    if (has_aq) {
      gq_fetch_packed<VEC, 4>(p, dp, src[GQ_AQ], q.st[GQ_AQ][1], q.st[GQ_AQ][2], pr, d);
      gq_put<4>(s.AQs, pd, dp, p);
    }
  }

  // the key tiles come through registers: the next tile's global reads are issued before the current tile's products
  GqPieces<2> pk, pv, pak, pav;
  auto fetch_keys = [&](const int j0) {
    gq_fetch<VEC, 2>(pk, dp, src[GQ_K], q.st[GQ_K][2], j0, S, d);
    gq_fetch<VEC, 2>(pv, dp, src[GQ_V], q.st[GQ_V][2], j0, S, d);
    if (has_ak) gq_fetch<VEC, 2>(pak, dp, src[GQ_AK], q.st[GQ_AK][2], j0, S, d);
    if (has_av) gq_fetch<VEC, 2>(pav, dp, src[GQ_AV], q.st[GQ_AV][2], j0, S, d);
  };
  auto put_keys = [&]() {
    gq_put<2>(s.Ks, pd, dp, pk);
    gq_put<2>(s.Vs, pd, dp, pv);
    if (has_ak) gq_put<2>(s.AKs, pd, dp, pak);
    if (has_av) gq_put<2>(s.AVs, pd, dp, pav);
  };
  fetch_keys(0);

  // (a) the online pass
  GqStats st;
  double a_l[4], a_gp[4], a_t[4], a_tgp[4], a_w[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    st.m[r] = -INFINITY;
    a_l[r] = a_gp[r] = a_t[r] = a_tgp[r] = a_w[r] = 0.0;
  }
  for (int kt = 0; kt < nkt; ++kt) {
    const int j0 = kt * kGqBN;
    __syncthreads();   // the previous tile's reads are done
    put_keys();
    __syncthreads();
    if (kt + 1 < nkt) fetch_keys(j0 + kGqBN);
    GqRaw raw;
    gq_raw(raw, s, has_aq, has_ak, has_av, pd, dp, w, n, g4);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float sc0 = gq_score(raw.s0[0][r], q, mine.m[r], mine.rw[r], j0 + n);
      const float sc1 = gq_score(raw.s0[1][r], q, mine.m[r], mine.rw[r], j0 + 16 + n);
      const float m_old = st.m[r];
      const float m_new = fmaxf(m_old, gq_max16(fmaxf(sc0, sc1)));
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
    const double l = gq_sum16(a_l[r]);
    // A fully masked row (or one past g L) has e = 0 throughout: l = 0 and the four other sums are 0 as well.  Divided by 1 instead of
    // by 0 they give D = E = R = 0, and P = exp(-inf) * 1 = 0 with them gS = bgP = bS = 0: zeros, where 0 / 0 was NaN.
    const double ld = l > 0.0 ? l : 1.0;
    const double D = gq_sum16(a_gp[r]) / ld, E = gq_sum16(a_t[r]) / ld;
    const double R = gq_sum16(a_tgp[r]) / ld - 2.0 * D * E + gq_sum16(a_w[r]) / ld;
    st.il[r] = 1.0 / ld; st.D[r] = D; st.E[r] = E; st.R[r] = R;
    const int p = r0 + 16 * w + 4 * g4 + r;
    if (n == 0 && p < rows) {   // (b, g kvh + p / L, p % L) of (B, Hq, L) is packed row p of (B, Hkv, g L)
      double* o = q.ws + ((long long)bk * rows + p) * kGqStats;
      o[0] = (double)st.m[r]; o[1] = l; o[2] = D; o[3] = E; o[4] = R;
    }
  }

  // (b) dQ and dgO
  float* const dq = q.out[GQ_DQ] ? q.out[GQ_DQ] + (long long)bk * rows * d : nullptr;
  float* const dgo = q.out[GQ_DGO] ? q.out[GQ_DGO] + (long long)bk * rows * d : nullptr;
  if (!dq && !dgo) return;   // uniform over the grid
  constexpr int ncb = NCB;
  gq_f32x4 acc_q[4], acc_o[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) acc_q[cb] = acc_o[cb] = gq_f32x4{0.f, 0.f, 0.f, 0.f};
  fetch_keys(0);
  for (int kt = 0; kt < nkt; ++kt) {
    const int j0 = kt * kGqBN;
    __syncthreads();
    put_keys();
    __syncthreads();
    if (kt + 1 < nkt) fetch_keys(j0 + kGqBN);
    GqRaw raw;
    gq_raw(raw, s, has_aq, has_ak, has_av, pd, dp, w, n, g4);
    gq_write_scores(raw, st, q, mine, has_t, has_av, s.X0, s.X1, s.X2, s.X3, j0, w, n, g4);
    __syncthreads();
    if (dq) {
      gq_nn(acc_q, s.X3, s.Ks, pd, ncb, w, n, g4);
      if (has_ak) gq_nn(acc_q, s.X1, s.AKs, pd, ncb, w, n, g4);
    }
    if (dgo) {
      if (has_t) gq_nn(acc_o, s.X2, s.Vs, pd, ncb, w, n, g4);
      if (has_av) gq_nn(acc_o, s.X0, s.AVs, pd, ncb, w, n, g4);
    }
  }
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    if (cb >= ncb) break;
    if (dq) gq_store(dq, acc_q[cb], q.scale, r0 + 16 * w, rows, cb, d, n, g4);
    if (dgo) gq_store(dgo, acc_o[cb], 1.f, r0 + 16 * w, rows, cb, d, n, g4);
  }
}

// grid = B * Hkv * nkt.  Block: 32 keys, the whole group of query heads.
template <int VEC, int NCB>
__global__ __launch_bounds__(kThreads) void k_attn_gqa_k(const GqArgs q) {
  extern __shared__ __attribute__((aligned(16))) float gq_lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = lane & 15, g4 = lane >> 4;
  constexpr int dp = 16 * NCB, pd = dp + 4;
  const int L = q.L, S = q.S, d = q.d, rows = q.rows;
  const int bk = blockIdx.x / q.nkt, kt = blockIdx.x - bk * q.nkt;
  const int b = bk / q.Hkv, kvh = bk - b * q.Hkv;
  const int j0 = kt * kGqBN;
  const GqLds s = gq_carve(gq_lds, pd, false);
  const float* src[GQ_IN];
  gq_sources(src, q, b, kvh);
  const bool has_aq = src[GQ_AQ] != nullptr, has_ak = src[GQ_AK] != nullptr, has_av = src[GQ_AV] != nullptr;
  const bool has_t = has_aq || has_ak;
  const float* mgroup = q.mask ? q.mask + (b * q.mst[0] + (long long)q.G * kvh * q.mst[1]) : nullptr;
  float* const dk = q.out[GQ_DK] ? q.out[GQ_DK] + (long long)bk * S * d : nullptr;
  float* const dv = q.out[GQ_DV] ? q.out[GQ_DV] + (long long)bk * S * d : nullptr;
  // the wave's output tiles t = w and w + 4 of the 2 (key blocks) x ncb (column blocks) grid
  constexpr int ntile = 2 * NCB;
  gq_f32x4 acc_k[2], acc_v[2];
  gq_zero2(acc_k); gq_zero2(acc_v);

  {
    GqPieces<2> p;
    gq_fetch<VEC, 2>(p, dp, src[GQ_K], q.st[GQ_K][2], j0, S, d);
    gq_put<2>(s.Ks, pd, dp, p);
    gq_fetch<VEC, 2>(p, dp, src[GQ_V], q.st[GQ_V][2], j0, S, d);
    gq_put<2>(s.Vs, pd, dp, p);
    if (has_ak) {
      gq_fetch<VEC, 2>(p, dp, src[GQ_AK], q.st[GQ_AK][2], j0, S, d);
      gq_put<2>(s.AKs, pd, dp, p);
    }
    if (has_av) {
      gq_fetch<VEC, 2>(p, dp, src[GQ_AV], q.st[GQ_AV][2], j0, S, d);
      gq_put<2>(s.AVs, pd, dp, p);
    }
  }
  // the packed query tiles come through registers: the next live tile's global reads are issued before the current tile's products
  GqPieces<4> pq, pgo, paq;
  auto fetch_queries = [&](const int r0) {
    GqPieceRows<4> pr;
    gq_piece_rows<4>(pr, dp, r0, rows, L);
    gq_fetch_packed<VEC, 4>(pq, dp, src[GQ_Q], q.st[GQ_Q][1], q.st[GQ_Q][2], pr, d);
    gq_fetch_packed<VEC, 4>(pgo, dp, src[GQ_GO], q.st[GQ_GO][1], q.st[GQ_GO][2], pr, d);
    if (has_aq) gq_fetch_packed<VEC, 4>(paq, dp, src[GQ_AQ], q.st[GQ_AQ][1], q.st[GQ_AQ][2], pr, d);
  };
  // Under the causal flag a packed tile whose largest in-head row is below j0 lies wholly above the diagonal.  Each head of the group
  // starts again at row 0, so live and dead tiles alternate: the next live one is searched (uniform over the block).
  auto next_live = [&](int qt) {
    while (qt < q.nqt && q.causal && gq_tile_max_row(qt * kGqBM, rows, L) < j0) ++qt;
    return qt;
  };
  int qt = next_live(0);
  if (qt < q.nqt) fetch_queries(qt * kGqBM);
  while (qt < q.nqt) {
    const int r0 = qt * kGqBM, nx = next_live(qt + 1);
    __syncthreads();
    gq_put<4>(s.Qs, pd, dp, pq);
    gq_put<4>(s.GOs, pd, dp, pgo);
    if (has_aq) gq_put<4>(s.AQs, pd, dp, paq);
    const int p0 = r0 + 16 * w + 4 * g4;
    GqRows mine;
    gq_rows(mine, q, mgroup, p0);
    GqStats st;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      st.m[r] = 0.f; st.il[r] = 1.0; st.D[r] = st.E[r] = st.R[r] = 0.0;
      if (p0 + r < rows) {
        const double* o = q.ws + ((long long)bk * rows + p0 + r) * kGqStats;
        st.m[r] = (float)o[0]; st.il[r] = o[1] > 0.0 ? 1.0 / o[1] : 0.0; st.D[r] = o[2]; st.E[r] = o[3]; st.R[r] = o[4];   // l = 0: a dead row, P = 0
      }
    }
    __syncthreads();
    if (nx < q.nqt) fetch_queries(nx * kGqBM);
    GqRaw raw;
    gq_raw(raw, s, has_aq, has_ak, has_av, pd, dp, w, n, g4);
    gq_write_scores(raw, st, q, mine, has_t, has_av, nullptr, s.X1, s.X2, s.X3, j0, w, n, g4);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int t = w + 4 * u;
      if (t >= ntile) break;
      const int kb = t & 1, cb = t >> 1;
      if (dv && has_t) gq_tn(acc_v[u], s.X2, s.GOs, pd, kb, cb, n, g4);
      if (dk) {
        gq_tn(acc_k[u], s.X3, s.Qs, pd, kb, cb, n, g4);
        if (has_aq) gq_tn(acc_k[u], s.X1, s.AQs, pd, kb, cb, n, g4);
      }
    }
    qt = nx;
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int t = w + 4 * u;
    if (t >= ntile) break;
    const int kb = t & 1, cb = t >> 1;
    if (dk) gq_store(dk, acc_k[u], q.scale, j0 + 16 * kb, S, cb, d, n, g4);
    if (dv) gq_store(dv, acc_v[u], 1.f, j0 + 16 * kb, S, cb, d, n, g4);
  }
}

// Why the launch does not take a shape, or NULL where it does: the launch, the plan and the workspace size refuse the same shapes.  The
// tiled sibling's refusals come first and in its words.
inline const char* gq_shape_error(int B, int Hq, int Hkv, int L, int S, int d) {
  if (!(B > 0 && Hq > 0 && Hkv > 0 && L > 0 && S > 0 && d > 0)) return "empty tensor";
  if (L > kGqMaxLen) return "more than 512 queries";
  if (S > kGqMaxLen) return "more than 512 keys";
  if (d > kGqMaxD) return "more than 64 elements per head";
  if (Hq % Hkv != 0) return "the number of query heads is not a multiple of the number of key/value heads";
  const int g = Hq / Hkv;
  if (g < 2) return "one query head per key/value head (g = 1) is the family of bhg_attention_tiled_backward_vjp";
  if ((long long)g * L > kGqMaxRows) return "more than 4096 packed query rows (g L)";
  const long long bk = (long long)B * Hkv;
  if (bk * (((long long)g * L + kGqBM - 1) / kGqBM) > 0x7fffffffLL || bk * ((S + kGqBN - 1) / kGqBN) > 0x7fffffffLL)
    return "a grid of more than 2^31 - 1 workgroups";
  return nullptr;
}

inline size_t gq_ws_bytes(int B, int Hq, int L) { return (size_t)B * Hq * L * kGqStats * sizeof(double); }

// Shape -> tiles, pitches and LDS bytes: the sibling's plan over g L packed rows.  Operand tiles: three of 64 rows (Q, gO, aQ) and four
// of 32 rows (K, V, aK, aV) at pitch pd = dp + 4, an odd number of 16-byte units.  Score tiles: 64 x 32 at pitch 36; four for the query
// launch (P, gS, bgP, bS), three for the key launch (no P).
inline const char* gq_plan(GqArgs* q, int B, int Hq, int Hkv, int L, int S, int d, int vec_ok) {
  const char* bad = gq_shape_error(B, Hq, Hkv, L, S, d);
  if (bad) return bad;
  q->B = B; q->Hq = Hq; q->Hkv = Hkv; q->G = Hq / Hkv; q->L = L; q->S = S; q->d = d;
  q->rows = q->G * L;
  q->vec = (d % 4 == 0 && vec_ok) ? 4 : 1;
  q->dp = (d + 15) / 16 * 16;
  q->pd = q->dp + 4;
  q->nqt = (q->rows + kGqBM - 1) / kGqBM;
  q->nkt = (S + kGqBN - 1) / kGqBN;
  const int operands = (3 * kGqBM + 4 * kGqBN) * q->pd;
  q->lds_q = (int)sizeof(float) * (operands + 4 * kGqBM * kGqPS);
  q->lds_k = (int)sizeof(float) * (operands + 3 * kGqBM * kGqPS);
  if (q->lds_q > kGqMaxLds) return "the plan needs more than 160 KiB of LDS";   // cannot happen for d <= 64 (123904)
  return nullptr;
}

inline long long gq_stride(const long long* st, int i, int extent) { return extent > 1 ? st[i] : 0; }

#undef GQ_MFMA

}  // namespace
}  // namespace bhg

using namespace bhg;

extern "C" {

size_t bhg_attention_gqa_ws_bytes(int B, int Hq, int L) {
  if (!(B > 0 && Hq > 0 && L > 0)) return 0;
  return gq_ws_bytes(B, Hq, L);
}

int bhg_attention_gqa_plan(int B, int Hq, int Hkv, int L, int S, int d, int vec_ok, char* buf, size_t buf_bytes) {
  BHG_REQUIRE(buf && buf_bytes > 0, "NULL buffer");
  GqArgs q{};
  const char* bad = gq_plan(&q, B, Hq, Hkv, L, S, d, vec_ok);
  BHG_REQUIRE(!bad, bad);
  const int len = snprintf(buf, buf_bytes,
                           "g=%d rows=%d vec=%d bm=%d bn=%d dp=%d pd=%d ps=%d grid_q=%lld grid_k=%lld lds_q=%d lds_k=%d max_lds=%d ws=%llu", q.G,
                           q.rows, q.vec, kGqBM, kGqBN, q.dp, q.pd, kGqPS, (long long)B * Hkv * q.nqt, (long long)B * Hkv * q.nkt, q.lds_q,
                           q.lds_k, kGqMaxLds, (unsigned long long)gq_ws_bytes(B, Hq, L));
  BHG_REQUIRE(len > 0 && (size_t)len < buf_bytes, "buffer too small for the plan line");
  return BHG_OK;
}

int bhg_attention_gqa_backward_vjp(const float* q, const float* k, const float* v, const float* go, const float* aq, const float* ak,
                                   const float* av, const long long* strides, const float* mask, const long long* mask_strides, int causal,
                                   float scale, int B, int Hq, int Hkv, int L, int S, int d, float* dq, float* dk, float* dv, float* dgo,
                                   void* ws, size_t ws_bytes, void* stream) {
  GqArgs a{};
  {
    const char* bad = gq_shape_error(B, Hq, Hkv, L, S, d);
    BHG_REQUIRE(!bad, bad);
  }
  BHG_REQUIRE(q && k && v && go, "null pointer (q, k, v and go are required)");
  BHG_REQUIRE(aq || ak || av, "all three cotangents are NULL");
  BHG_REQUIRE(dq || dk || dv || dgo, "all four outputs are NULL");
  BHG_REQUIRE(strides, "null pointer (strides)");
  BHG_REQUIRE(!mask || mask_strides, "null pointer (mask_strides)");
  BHG_REQUIRE(ws, "null pointer (workspace)");
  BHG_REQUIRE(ws_bytes >= gq_ws_bytes(B, Hq, L), "workspace too small (bhg_attention_gqa_ws_bytes)");
  BHG_REQUIRE(((uintptr_t)ws & 7) == 0, "the workspace must be 8-byte aligned");
  const float* in[GQ_IN] = {q, k, v, go, aq, ak, av};
  const int heads_of[GQ_IN] = {Hq, Hkv, Hkv, Hq, Hq, Hkv, Hkv};
  const int rows_of[GQ_IN] = {L, S, S, L, L, S, S};
  int vec_ok = 1;
  for (int i = 0; i < GQ_IN; ++i) {
    a.in[i] = in[i];
    const long long* st = strides + 4 * i;
    BHG_REQUIRE(!in[i] || d == 1 || st[3] == 1, "the last stride of every input must be 1");
    a.st[i][0] = gq_stride(st, 0, B); a.st[i][1] = gq_stride(st, 1, heads_of[i]); a.st[i][2] = gq_stride(st, 2, rows_of[i]);
    if (!in[i]) continue;
    for (int j = 0; j < 3; ++j) {
      BHG_REQUIRE(a.st[i][j] >= 0, "negative stride");
      if (a.st[i][j] % 4 != 0) vec_ok = 0;
    }
  }
  const char* bad = gq_plan(&a, B, Hq, Hkv, L, S, d, vec_ok);
  BHG_REQUIRE(!bad, bad);
  if (a.vec == 4) {
    for (const void* p : {(const void*)q, (const void*)k, (const void*)v, (const void*)go, (const void*)aq, (const void*)ak, (const void*)av,
                          (const void*)dq, (const void*)dk, (const void*)dv, (const void*)dgo})
      BHG_REQUIRE(((uintptr_t)p & 15) == 0, "inputs and outputs must be 16-byte aligned on the vector path (d and every stride a multiple of 4)");
  }
  a.mask = mask;
  if (mask) {
    const int ext[4] = {B, Hq, L, S};
    for (int j = 0; j < 4; ++j) {
      a.mst[j] = gq_stride(mask_strides, j, ext[j]);
      BHG_REQUIRE(a.mst[j] >= 0, "negative stride");
    }
  }
  a.out[GQ_DQ] = dq; a.out[GQ_DK] = dk; a.out[GQ_DV] = dv; a.out[GQ_DGO] = dgo;
  a.ws = static_cast<double*>(ws);
  a.causal = causal != 0;
  a.scale = scale;
  // above 64 KiB a kernel's dynamic LDS has to be allowed, once per process and device
  static bool attr_done[64] = {};
  int dev = 0;
  BHG_HIP_CHECK(hipGetDevice(&dev));
  using Kernel = void (*)(const GqArgs);
  static const Kernel kq[2][4] = {{k_attn_gqa_q<1, 1>, k_attn_gqa_q<1, 2>, k_attn_gqa_q<1, 3>, k_attn_gqa_q<1, 4>},
                                  {k_attn_gqa_q<4, 1>, k_attn_gqa_q<4, 2>, k_attn_gqa_q<4, 3>, k_attn_gqa_q<4, 4>}};
  static const Kernel kk[2][4] = {{k_attn_gqa_k<1, 1>, k_attn_gqa_k<1, 2>, k_attn_gqa_k<1, 3>, k_attn_gqa_k<1, 4>},
                                  {k_attn_gqa_k<4, 1>, k_attn_gqa_k<4, 2>, k_attn_gqa_k<4, 3>, k_attn_gqa_k<4, 4>}};
  if (dev < 0 || dev >= 64 || !attr_done[dev]) {
    for (int i = 0; i < 2; ++i)
      for (int j = 0; j < 4; ++j) {
        BHG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kq[i][j]), hipFuncAttributeMaxDynamicSharedMemorySize, kGqMaxLds));
        BHG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kk[i][j]), hipFuncAttributeMaxDynamicSharedMemorySize, kGqMaxLds));
      }
    if (dev >= 0 && dev < 64) attr_done[dev] = true;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned grid_q = (unsigned)((long long)B * Hkv * a.nqt), grid_k = (unsigned)((long long)B * Hkv * a.nkt);
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
