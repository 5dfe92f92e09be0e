// bhg_attention_wide.hip — the Hessian-vector product's share of an attention core for head widths 65 .. 128: the wide sibling of
// bhg_attention_tiled.hip (same quantities, same notation, same interface, same workspace), for 1 <= L, S <= 512 and 65 <= d <= 128.
//
// Per (batch, head), as in the siblings:
//     P = softmax_rows(s Q K^T + m)     gP = gO V^T     D = rowsum(P * gP)     gS = P * (gP - D)
//     T = s (aQ K^T + Q aK^T)           E = rowsum(P * T)                      bgP = P * (T - E)
//     bP = T * (gP - D) - gP * E + gO aV^T              R = rowsum(P * bP)     bS = P * (bP - R)
//     dgO = bgP V + P aV     dV = bgP^T gO     dQ = s (bS K + gS aK)     dK = s (bS^T Q + gS^T aQ)
// The mathematics and the two-launch scheme are those of the tiled sibling (float64 restatement: tests/attention_tiled_ref.py): one
// online pass over the key tiles keeps, with e = exp(score - m_running), the five unnormalised fp64 sums
//     sum e      sum e gP      sum e T      sum e T gP      sum e (gO aV^T)
// per row, rescaled by exp(m_old - m_new) when the running maximum moves, and R = rowsum(P * T * gP) - 2 D E + rowsum(P * (gO aV^T)).
// A tile whose keys are all masked leaves the maximum at -inf: e is then taken against 0 and the rescale of the still-empty sums is
// skipped, so live keys in a later tile are not poisoned.  A fully masked ROW ends with m = -inf, l = 0 and all five sums 0; divided by 1
// instead they give D = E = R = 0 and P = exp(-inf) = 0: its probabilities are zero, as on torch's math path (2.10), and its rows of dQ and dgO are exact zeros.
//
// THE TILING, and why.  At dp = 128 an operand row is 132 floats (pitch dp + 4, an odd number of 16-byte units), 528 bytes, so the
// sibling's three 64-row and four 32-row tiles alone are 168 960 bytes: more than a CU has.  The two launches have different needs, so
// they get different tiles:
//   k_attn_wide_q   grid B H ceil(L / 64): 64 queries x 16 keys.  The online pass wants a row's statistics in ONE wave (the sixteen
//       lanes that hold a row of the MFMA accumulator reduce by four shuffles; with 32-row blocks of two column strips a row would be
//       spread over two waves and its running maximum and five sums would have to be combined through LDS once per key tile), and
//       the outputs dQ, dgO (2 x 8 accumulator tiles per wave at dp = 128) amortise best over many resident rows.  So Q, gO, aQ stay
//       resident with 64 rows, wave w owns rows 16 w .. 16 w + 15 as in the sibling, and the streamed key tile shrinks to 16 keys:
//       LDS = 4 ((3 64 + 4 16) 132 + 4 64 20) = 155 648 bytes.
//   k_attn_wide_k   grid B H ceil(S / 32): 32 keys x 32 queries.  Here the statistics are READ (from the workspace), so nothing
//       has to be combined and a score tile can be split over the waves freely: wave w owns the 16 x 16 block (w >> 1, w & 1) of the
//       32 x 32 score tile.  32 resident keys halve the number of times Q, gO, aQ stream past (against 16), and the wave's four
//       output tiles of dK and of dV share one A fragment: LDS = 4 ((3 32 + 4 32) 132 + 3 32 36) = 132 096 bytes.
// Both are below the 163 840 bytes one workgroup may take; one workgroup per CU, four waves with 512 registers each.
// Under the causal flag the tiles wholly above the diagonal are skipped in both launches.
//
// Every product runs on the fp32-input MFMA v_mfma_f32_16x16x4_f32: exact fp32.  Lane (n = lane & 15, g = lane >> 4) supplies
// A[n][k] and B[k][n]; step c of a group of four uses k = 4 g + c, so a lane's four A values are ONE 16-byte LDS read.  The raw products
// of a tile (Q K^T, gO V^T, aQ K^T + Q aK^T, gO aV^T) run as ONE loop over d with independent accumulators interleaved.  Operand tiles
// are zero-padded in LDS to the tile shape (rows past L / S, columns past d up to dp = d rounded up to 16) and the tile of an ABSENT
// cotangent is zeros, so no product has an edge case or a branch; score-tile elements outside L x S are zeros; stores are masked.  The
// kernels are instantiated per dp / 16 = 5 .. 8 and per global read width, so every product loop unrolls, and the tile that streams —
// keys in the first launch, queries in the second — comes through registers: its global reads are issued before the current tile's
// products.  Every loop is bounded by L, S, d.  No atomics, no grid barrier: deterministic.
//
// Layout: fp32.  Inputs with four element strides each (last stride 1), read in place; outputs contiguous (B, H, L | S, d).
// vec = 4 (16-byte global reads) when d % 4 == 0 and every stride of a present input is a multiple of 4; otherwise scalar reads.  The LDS
// image is the same on both paths.  Workspace: B H L rows of five doubles (m, l, D, E, R), 40 bytes per query row.
#include "bhg_common.hpp"

#include <math.h>

namespace bhg {
namespace {

typedef float wd_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWdMaxLen = 512, kWdMinD = 65, kWdMaxD = 128;
constexpr int kWdQM = 64, kWdQN = 16, kWdQPS = kWdQN + 4;   // query launch: rows, keys and row pitch (5 x 16 bytes) of a score tile
constexpr int kWdKM = 32, kWdKN = 32, kWdKPS = kWdKN + 4;   // key launch: queries, keys and row pitch (9 x 16 bytes) of a score tile
constexpr int kWdStats = 5;                                 // doubles per query row in the workspace: m l D E R
constexpr int kWdMaxLds = 160 * 1024;
enum { WD_Q = 0, WD_K, WD_V, WD_GO, WD_AQ, WD_AK, WD_AV, WD_IN };
enum { WD_DQ = 0, WD_DK, WD_DV, WD_DGO, WD_OUT };

struct WdArgs {
  const float* in[WD_IN];      // q k v go aq ak av; the last three may be NULL
  long long st[WD_IN][3];      // element strides: batch, head, row
  const float* mask;           // may be NULL
  long long mst[4];            // element strides of the mask (0 = broadcast)
  float* out[WD_OUT];          // dq dk dv dgo, contiguous; each may be NULL
  double* ws;                  // B H L x 5
  int B, H, L, S, d;
  int causal;
  float scale;
  int vec;                     // 4: 16-byte global reads; 1: scalar
  int dp, pd;                  // d rounded up to 16; row pitch of an operand tile (dp + 4)
  int q_nqt, q_nkt;            // query launch: query tiles of 64, key tiles of 16
  int k_nqt, k_nkt;            // key launch: query tiles of 32, key tiles of 32
  int lds_q, lds_k;            // bytes of dynamic LDS of the two launches
};

// Global -> LDS: a tile of ROWS rows x dp floats at pitch dp + 4, rows row0 .. of the `nrows` x d matrix at src (row stride rs), zeros
// outside the matrix and everywhere when src is NULL — in two steps: wd_fetch reads this thread's 16-byte pieces into registers,
// wd_put writes them to the LDS once the previous tile's readers have passed the barrier.
template <int ROWS, int NCB>
struct WdPieces {
  static constexpr int kN = (ROWS * 4 * NCB + kThreads - 1) / kThreads;
  float4 v[kN];
};

template <int VEC, int ROWS, int NCB>
__device__ __forceinline__ void wd_fetch(WdPieces<ROWS, NCB>& p, const float* __restrict__ src, const long long rs, const int row0,
                                         const int nrows, const int d) {
  constexpr int nv = 4 * NCB, n = ROWS * nv;
#pragma unroll
  for (int u = 0; u < WdPieces<ROWS, NCB>::kN; ++u) {
    const int idx = threadIdx.x + u * kThreads;
    const int r = idx / nv, c = (idx - r * nv) << 2;
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (src && idx < n && row0 + r < nrows && c < d) {
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

template <int ROWS, int NCB>
__device__ __forceinline__ void wd_put(float* __restrict__ dst, const WdPieces<ROWS, NCB>& p) {
  constexpr int nv = 4 * NCB, n = ROWS * nv, pd = 16 * NCB + 4;
#pragma unroll
  for (int u = 0; u < WdPieces<ROWS, NCB>::kN; ++u) {
    const int idx = threadIdx.x + u * kThreads;
    const int r = idx / nv, c = (idx - r * nv) << 2;
    if (idx < n) *reinterpret_cast<float4*>(dst + r * pd + c) = p.v[u];
  }
}

// Both steps at once, for the tiles that stay resident.
template <int VEC, int ROWS, int NCB>
__device__ __forceinline__ void wd_load(float* __restrict__ dst, const float* __restrict__ src, const long long rs, const int row0,
                                        const int nrows, const int d) {
  WdPieces<ROWS, NCB> p;
  wd_fetch<VEC, ROWS, NCB>(p, src, rs, row0, nrows, d);
  wd_put<ROWS, NCB>(dst, p);
}

#define WD_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// The four raw products of one 16 x 16 block: S0 = Q K^T, GP = gO V^T, T = aQ K^T + Q aK^T, W = gO aV^T (unscaled).
struct WdRaw {
  wd_f32x4 s0, gp, t, w;
};

// One loop over d for all of them, four independent accumulators interleaved.  The pointers are this lane's fragment rows: query-side
// row n of the block at column 4 g, key-side likewise.
template <int NCB>
__device__ __forceinline__ void wd_raw(WdRaw& r, const float* __restrict__ qa, const float* __restrict__ goa, const float* __restrict__ aqa,
                                       const float* __restrict__ kb, const float* __restrict__ vb, const float* __restrict__ akb,
                                       const float* __restrict__ avb) {
  r.s0 = r.gp = r.t = r.w = wd_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kk = 0; kk < NCB; ++kk) {
    const float4 fq = *reinterpret_cast<const float4*>(qa + 16 * kk), fgo = *reinterpret_cast<const float4*>(goa + 16 * kk);
    const float4 faq = *reinterpret_cast<const float4*>(aqa + 16 * kk), fk = *reinterpret_cast<const float4*>(kb + 16 * kk);
    const float4 fv = *reinterpret_cast<const float4*>(vb + 16 * kk), fak = *reinterpret_cast<const float4*>(akb + 16 * kk);
    const float4 fav = *reinterpret_cast<const float4*>(avb + 16 * kk);
#define WD_STEP(c)                          \
  r.s0 = WD_MFMA(fq.c, fk.c, r.s0);         \
  r.gp = WD_MFMA(fgo.c, fv.c, r.gp);        \
  r.t = WD_MFMA(faq.c, fk.c, r.t);          \
  r.w = WD_MFMA(fgo.c, fav.c, r.w);         \
  r.t = WD_MFMA(fq.c, fak.c, r.t);
    WD_STEP(x) WD_STEP(y) WD_STEP(z) WD_STEP(w)
#undef WD_STEP
  }
}

// Score of element (i, j) from the raw product; -inf outside L x S and above the diagonal under the causal flag.
__device__ __forceinline__ float wd_score(const float raw, const WdArgs& q, const float* __restrict__ mbase, const int i, const int j) {
  if (i >= q.L || j >= q.S || (q.causal && j > i)) return -INFINITY;
  float sc = q.scale * raw;
  if (mbase) sc += mbase[(long long)i * q.mst[2] + (long long)j * q.mst[3]];
  return sc;
}

__device__ __forceinline__ float wd_max16(float v) {   // over the sixteen lanes that hold one row
  v = fmaxf(v, __shfl_xor(v, 1));
  v = fmaxf(v, __shfl_xor(v, 2));
  v = fmaxf(v, __shfl_xor(v, 4));
  v = fmaxf(v, __shfl_xor(v, 8));
  return v;
}

__device__ __forceinline__ double wd_sum16(double v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}

// The finished statistics of the four rows 4 g + r of this lane's block.
struct WdStats {
  float m[4];
  double il[4], D[4], E[4], R[4];   // il = 1 / l
};

// P, gS, bgP, bS of this wave's 16 x 16 block -> the score tiles (zeros outside L x S).  `at0` is the block's first element in a
// tile of pitch `ps`; (i0, j0) its first row and column in the matrix.  X0 may be NULL (P is not needed for dK / dV).
__device__ __forceinline__ void wd_write_scores(const WdRaw& raw, const WdStats& st, const WdArgs& q, const float* __restrict__ mbase,
                                                float* X0, float* X1, float* X2, float* X3, const int at0, const int ps, const int i0,
                                                const int j0, const int n, const int g) {
  const int j = j0 + n;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + 4 * g + r;
    float pf = 0.f, gs = 0.f, bgp = 0.f, bs = 0.f;
    if (i < q.L && j < q.S) {
      const float sc = wd_score(raw.s0[r], q, mbase, i, j);
      const float mu = st.m[r] == -INFINITY ? 0.f : st.m[r];
      pf = (float)((double)expf(sc - mu) * st.il[r]);
      const double p = (double)pf;
      const double gp = (double)raw.gp[r];
      const double t = (double)(q.scale * raw.t[r]);
      const double wv = (double)raw.w[r];
      const double bp = t * (gp - st.D[r]) - gp * st.E[r] + wv;
      gs = (float)(p * (gp - st.D[r]));
      bgp = (float)(p * (t - st.E[r]));
      bs = (float)(p * (bp - st.R[r]));
    }
    const int at = at0 + (4 * g + r) * ps + n;
    if (X0) X0[at] = pf;
    X1[at] = gs;
    X2[at] = bgp;
    X3[at] = bs;
  }
}

// Query launch: acc[cb] += X[16 w + n][j] M[j][16 cb + n']   (the wave's 16 rows x dp outputs; contraction over the 16 keys of the tile)
template <int NCB>
__device__ __forceinline__ void wd_nn(wd_f32x4 (&acc)[NCB], const float* __restrict__ X, const float* __restrict__ M, const int w, const int n,
                                      const int g) {
  constexpr int pd = 16 * NCB + 4;
  const float4 a4 = *reinterpret_cast<const float4*>(X + (16 * w + n) * kWdQPS + 4 * g);
  const float a[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float* mr = M + (4 * g + c) * pd + n;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) acc[cb] = WD_MFMA(a[c], mr[16 * cb], acc[cb]);
  }
}

// Key launch: acc[u] += sum_i X[i][16 kb + n] M[i][16 (cb0 + 2 u) + n']   (the wave's output tiles share the key block kb, hence the A
// fragment; contraction over the 32 queries of the tile)
template <int NCB>
__device__ __forceinline__ void wd_tn(wd_f32x4 (&acc)[4], const float* __restrict__ X, const float* __restrict__ M, const int kb, const int cb0,
                                      const int n, const int g) {
  constexpr int pd = 16 * NCB + 4;
  const float* xc = X + 16 * kb + n;
  const float* mc = M + 16 * cb0 + n;
#pragma unroll
  for (int i0 = 0; i0 < kWdKM; i0 += 16) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + 4 * g + c;
      const float a = xc[i * kWdKPS];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (cb0 + 2 * u < NCB) acc[u] = WD_MFMA(a, mc[i * pd + 32 * u], acc[u]);   // (uniform over the wave)
    }
  }
}

// out[(row0 + 4 g + r)][16 cb + n] = f * acc[r], rows < nrows, columns < d; `out` is the (b, h) slice, contiguous rows of d.
__device__ __forceinline__ void wd_store(float* __restrict__ out, const wd_f32x4& acc, const float f, const int row0, const int nrows, const int cb,
                                         const int d, const int n, const int g) {
  const int col = 16 * cb + n;
  if (col >= d) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + 4 * g + r;
    if (row < nrows) out[(long long)row * d + col] = f * acc[r];
  }
}

// grid = B * H * q_nqt.  Block: 64 query rows; key tiles of 16.
template <int VEC, int NCB>
__global__ __launch_bounds__(kThreads) void k_attn_wide_q(const WdArgs q) {
  extern __shared__ __attribute__((aligned(16))) float wd_lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = lane & 15, g = lane >> 4;
  constexpr int pd = 16 * NCB + 4;
  const int L = q.L, S = q.S, d = q.d;
  const int bh = blockIdx.x / q.q_nqt, qt = blockIdx.x - bh * q.q_nqt;
  const int b = bh / q.H, h = bh - b * q.H;
  const int i0 = qt * kWdQM;
  float* const Qs = wd_lds;
  float* const GOs = Qs + kWdQM * pd;
  float* const AQs = GOs + kWdQM * pd;
  float* const Ks = AQs + kWdQM * pd;
  float* const Vs = Ks + kWdQN * pd;
  float* const AKs = Vs + kWdQN * pd;
  float* const AVs = AKs + kWdQN * pd;
  float* const X0 = AVs + kWdQN * pd;
  float* const X1 = X0 + kWdQM * kWdQPS;
  float* const X2 = X1 + kWdQM * kWdQPS;
  float* const X3 = X2 + kWdQM * kWdQPS;
  const float* src[WD_IN];
#pragma unroll
  for (int i = 0; i < WD_IN; ++i) src[i] = q.in[i] ? q.in[i] + (b * q.st[i][0] + h * q.st[i][1]) : nullptr;
  const bool has_ak = src[WD_AK] != nullptr, has_av = src[WD_AV] != nullptr;
  const bool has_t = src[WD_AQ] != nullptr || has_ak;
  const float* mbase = q.mask ? q.mask + (b * q.mst[0] + h * q.mst[1]) : nullptr;
  // key tiles that hold an element on or below the diagonal for some row of this block
  int nkt = q.q_nkt;
  if (q.causal) {
    const int last = (i0 + kWdQM - 1 < L - 1 ? i0 + kWdQM - 1 : L - 1) / kWdQN + 1;
    nkt = last < nkt ? last : nkt;
  }

  wd_load<VEC, kWdQM, NCB>(Qs, src[WD_Q], q.st[WD_Q][2], i0, L, d);
  wd_load<VEC, kWdQM, NCB>(GOs, src[WD_GO], q.st[WD_GO][2], i0, L, d);
  wd_load<VEC, kWdQM, NCB>(AQs, src[WD_AQ], q.st[WD_AQ][2], i0, L, d);   // zeros when aq is absent

  // the key tiles come through registers: the next tile's global reads are issued before the current tile's products
  WdPieces<kWdQN, NCB> pk, pv, pak, pav;
  auto fetch_keys = [&](const int j0) {
    wd_fetch<VEC, kWdQN, NCB>(pk, src[WD_K], q.st[WD_K][2], j0, S, d);
    wd_fetch<VEC, kWdQN, NCB>(pv, src[WD_V], q.st[WD_V][2], j0, S, d);
    wd_fetch<VEC, kWdQN, NCB>(pak, src[WD_AK], q.st[WD_AK][2], j0, S, d);
    wd_fetch<VEC, kWdQN, NCB>(pav, src[WD_AV], q.st[WD_AV][2], j0, S, d);
  };
  auto put_keys = [&]() {
    wd_put<kWdQN, NCB>(Ks, pk);
    wd_put<kWdQN, NCB>(Vs, pv);
    wd_put<kWdQN, NCB>(AKs, pak);
    wd_put<kWdQN, NCB>(AVs, pav);
  };
  // this lane's fragment rows
  const float* const qa = Qs + (16 * w + n) * pd + 4 * g;
  const float* const goa = GOs + (16 * w + n) * pd + 4 * g;
  const float* const aqa = AQs + (16 * w + n) * pd + 4 * g;
  const float* const kb = Ks + n * pd + 4 * g;
  const float* const vb = Vs + n * pd + 4 * g;
  const float* const akb = AKs + n * pd + 4 * g;
  const float* const avb = AVs + n * pd + 4 * g;
  fetch_keys(0);

  // (a) the online pass
  WdStats st;
  double a_l[4], a_gp[4], a_t[4], a_tgp[4], a_w[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    st.m[r] = -INFINITY;
    a_l[r] = a_gp[r] = a_t[r] = a_tgp[r] = a_w[r] = 0.0;
  }
  for (int kt = 0; kt < nkt; ++kt) {
    const int j0 = kt * kWdQN;
    __syncthreads();   // the previous tile's reads are done
    put_keys();
    __syncthreads();
    if (kt + 1 < nkt) fetch_keys(j0 + kWdQN);
    WdRaw raw;
    wd_raw<NCB>(raw, qa, goa, aqa, kb, vb, akb, avb);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + 16 * w + 4 * g + r;
      const float sc = wd_score(raw.s0[r], q, mbase, i, j0 + n);
      const float m_old = st.m[r];
      const float m_new = fmaxf(m_old, wd_max16(sc));
      const float mu = m_new == -INFINITY ? 0.f : m_new;
      if (m_old != -INFINITY && m_new != m_old) {   // (while the maximum is -inf the sums are empty: nothing to rescale)
        const double f = (double)expf(m_old - m_new);
        a_l[r] *= f; a_gp[r] *= f; a_t[r] *= f; a_tgp[r] *= f; a_w[r] *= f;
      }
      st.m[r] = m_new;
      const double e = (double)expf(sc - mu);
      const double gp = (double)raw.gp[r];
      const double t = (double)(q.scale * raw.t[r]);
      const double wv = (double)raw.w[r];
      a_l[r] += e;
      a_gp[r] += e * gp;
      a_t[r] += e * t;
      a_tgp[r] += e * (t * gp);
      a_w[r] += e * wv;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double l = wd_sum16(a_l[r]);
    // A fully masked row (or one past L) has e = 0 throughout: l = 0 and the four other sums are 0 as well.  Divided by 1 instead of by
    // 0 they give D = E = R = 0, and P = exp(-inf) * 1 = 0 with them gS = bgP = bS = 0: zeros, where 0 / 0 was NaN.
    const double ld = l > 0.0 ? l : 1.0;
    const double D = wd_sum16(a_gp[r]) / ld, E = wd_sum16(a_t[r]) / ld;
    const double R = wd_sum16(a_tgp[r]) / ld - 2.0 * D * E + wd_sum16(a_w[r]) / ld;
    st.il[r] = 1.0 / ld; st.D[r] = D; st.E[r] = E; st.R[r] = R;
    const int i = i0 + 16 * w + 4 * g + r;
    if (n == 0 && i < L) {
      double* o = q.ws + ((long long)bh * L + i) * kWdStats;
      o[0] = (double)st.m[r]; o[1] = l; o[2] = D; o[3] = E; o[4] = R;
    }
  }

  // (b) dQ and dgO
  float* const dq = q.out[WD_DQ] ? q.out[WD_DQ] + (long long)bh * L * d : nullptr;
  float* const dgo = q.out[WD_DGO] ? q.out[WD_DGO] + (long long)bh * L * d : nullptr;
  if (!dq && !dgo) return;   // uniform over the grid
  wd_f32x4 acc_q[NCB], acc_o[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) acc_q[cb] = acc_o[cb] = wd_f32x4{0.f, 0.f, 0.f, 0.f};
  fetch_keys(0);
  for (int kt = 0; kt < nkt; ++kt) {
    const int j0 = kt * kWdQN;
    __syncthreads();   // the previous tile's operand and score reads are done
    put_keys();
    __syncthreads();
    if (kt + 1 < nkt) fetch_keys(j0 + kWdQN);
    WdRaw raw;
    wd_raw<NCB>(raw, qa, goa, aqa, kb, vb, akb, avb);
    wd_write_scores(raw, st, q, mbase, X0, X1, X2, X3, 16 * w * kWdQPS, kWdQPS, i0 + 16 * w, j0, n, g);
    __syncthreads();
    if (dq) {
      wd_nn<NCB>(acc_q, X3, Ks, w, n, g);
      if (has_ak) wd_nn<NCB>(acc_q, X1, AKs, w, n, g);
    }
    if (dgo) {
      if (has_t) wd_nn<NCB>(acc_o, X2, Vs, w, n, g);
      if (has_av) wd_nn<NCB>(acc_o, X0, AVs, w, n, g);
    }
  }
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) {
    if (dq) wd_store(dq, acc_q[cb], q.scale, i0 + 16 * w, L, cb, d, n, g);
    if (dgo) wd_store(dgo, acc_o[cb], 1.f, i0 + 16 * w, L, cb, d, n, g);
  }
}

// grid = B * H * k_nkt.  Block: 32 keys; query tiles of 32.
template <int VEC, int NCB>
__global__ __launch_bounds__(kThreads) void k_attn_wide_k(const WdArgs q) {
  extern __shared__ __attribute__((aligned(16))) float wd_lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = lane & 15, g = lane >> 4;
  constexpr int pd = 16 * NCB + 4;
  const int L = q.L, S = q.S, d = q.d;
  const int bh = blockIdx.x / q.k_nkt, kt = blockIdx.x - bh * q.k_nkt;
  const int b = bh / q.H, h = bh - b * q.H;
  const int j0 = kt * kWdKN;
  float* const Ks = wd_lds;
  float* const Vs = Ks + kWdKN * pd;
  float* const AKs = Vs + kWdKN * pd;
  float* const AVs = AKs + kWdKN * pd;
  float* const Qs = AVs + kWdKN * pd;
  float* const GOs = Qs + kWdKM * pd;
  float* const AQs = GOs + kWdKM * pd;
  float* const X1 = AQs + kWdKM * pd;
  float* const X2 = X1 + kWdKM * kWdKPS;
  float* const X3 = X2 + kWdKM * kWdKPS;
  const float* src[WD_IN];
#pragma unroll
  for (int i = 0; i < WD_IN; ++i) src[i] = q.in[i] ? q.in[i] + (b * q.st[i][0] + h * q.st[i][1]) : nullptr;
  const bool has_aq = src[WD_AQ] != nullptr;
  const bool has_t = has_aq || src[WD_AK] != nullptr;
  const float* mbase = q.mask ? q.mask + (b * q.mst[0] + h * q.mst[1]) : nullptr;
  float* const dk = q.out[WD_DK] ? q.out[WD_DK] + (long long)bh * S * d : nullptr;
  float* const dv = q.out[WD_DV] ? q.out[WD_DV] + (long long)bh * S * d : nullptr;
  const int qt0 = q.causal ? j0 / kWdKM : 0;   // query tiles above hold only rows i < j0: wholly above the diagonal
  // the wave's block of the score tile, and its output tiles: key block okb, column blocks ocb0 + 2 u
  const int rb = w >> 1, sb = w & 1;
  const int okb = w & 1, ocb0 = w >> 1;
  wd_f32x4 acc_k[4], acc_v[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) acc_k[u] = acc_v[u] = wd_f32x4{0.f, 0.f, 0.f, 0.f};

  wd_load<VEC, kWdKN, NCB>(Ks, src[WD_K], q.st[WD_K][2], j0, S, d);
  wd_load<VEC, kWdKN, NCB>(Vs, src[WD_V], q.st[WD_V][2], j0, S, d);
  wd_load<VEC, kWdKN, NCB>(AKs, src[WD_AK], q.st[WD_AK][2], j0, S, d);   // zeros when absent
  wd_load<VEC, kWdKN, NCB>(AVs, src[WD_AV], q.st[WD_AV][2], j0, S, d);
  // the query tiles come through registers: the next tile's global reads are issued before the current tile's products
  WdPieces<kWdKM, NCB> pq, pgo, paq;
  auto fetch_queries = [&](const int i0) {
    wd_fetch<VEC, kWdKM, NCB>(pq, src[WD_Q], q.st[WD_Q][2], i0, L, d);
    wd_fetch<VEC, kWdKM, NCB>(pgo, src[WD_GO], q.st[WD_GO][2], i0, L, d);
    wd_fetch<VEC, kWdKM, NCB>(paq, src[WD_AQ], q.st[WD_AQ][2], i0, L, d);
  };
  const float* const qa = Qs + (16 * rb + n) * pd + 4 * g;
  const float* const goa = GOs + (16 * rb + n) * pd + 4 * g;
  const float* const aqa = AQs + (16 * rb + n) * pd + 4 * g;
  const float* const kb = Ks + (16 * sb + n) * pd + 4 * g;
  const float* const vb = Vs + (16 * sb + n) * pd + 4 * g;
  const float* const akb = AKs + (16 * sb + n) * pd + 4 * g;
  const float* const avb = AVs + (16 * sb + n) * pd + 4 * g;
  if (qt0 < q.k_nqt) fetch_queries(qt0 * kWdKM);
  for (int qt = qt0; qt < q.k_nqt; ++qt) {
    const int i0 = qt * kWdKM;
    __syncthreads();   // the previous tile's operand and score reads are done
    wd_put<kWdKM, NCB>(Qs, pq);
    wd_put<kWdKM, NCB>(GOs, pgo);
    wd_put<kWdKM, NCB>(AQs, paq);
    WdStats st;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + 16 * rb + 4 * g + r;
      st.m[r] = 0.f; st.il[r] = 1.0; st.D[r] = st.E[r] = st.R[r] = 0.0;
      if (i < L) {
        const double* o = q.ws + ((long long)bh * L + i) * kWdStats;
        st.m[r] = (float)o[0]; st.il[r] = o[1] > 0.0 ? 1.0 / o[1] : 0.0; st.D[r] = o[2]; st.E[r] = o[3]; st.R[r] = o[4];   // l = 0: a dead row, P = 0
      }
    }
    __syncthreads();
    if (qt + 1 < q.k_nqt) fetch_queries(i0 + kWdKM);
    WdRaw raw;
    wd_raw<NCB>(raw, qa, goa, aqa, kb, vb, akb, avb);
    wd_write_scores(raw, st, q, mbase, nullptr, X1, X2, X3, 16 * rb * kWdKPS + 16 * sb, kWdKPS, i0 + 16 * rb, j0 + 16 * sb, n, g);
    __syncthreads();
    if (dv && has_t) wd_tn<NCB>(acc_v, X2, GOs, okb, ocb0, n, g);
    if (dk) {
      wd_tn<NCB>(acc_k, X3, Qs, okb, ocb0, n, g);
      if (has_aq) wd_tn<NCB>(acc_k, X1, AQs, okb, ocb0, n, g);
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int cb = ocb0 + 2 * u;
    if (cb >= NCB) break;
    if (dk) wd_store(dk, acc_k[u], q.scale, j0 + 16 * okb, S, cb, d, n, g);
    if (dv) wd_store(dv, acc_v[u], 1.f, j0 + 16 * okb, S, cb, d, n, g);
  }
}

// The launch, the plan and the workspace size refuse the same shapes with the same words.
inline const char* wd_shape_error(int B, int H, int L, int S, int d) {
  if (!(B > 0 && H > 0 && L > 0 && S > 0 && d > 0)) return "empty tensor";
  if (L > kWdMaxLen) return "more than 512 queries";
  if (S > kWdMaxLen) return "more than 512 keys";
  if (d < kWdMinD)
    return "fewer than 65 elements per head (bhg_attention_backward_vjp and bhg_attention_tiled_backward_vjp take d <= 64)";
  if (d > kWdMaxD) return "more than 128 elements per head";
  const long long bh = (long long)B * H;
  if (bh * ((L + kWdQM - 1) / kWdQM) > 0x7fffffffLL || bh * ((S + kWdKN - 1) / kWdKN) > 0x7fffffffLL)
    return "a grid of more than 2^31 - 1 workgroups";
  return nullptr;
}

inline size_t wd_ws_bytes(int B, int H, int L) { return (size_t)B * H * L * kWdStats * sizeof(double); }

// Shape -> tiles, pitches and LDS bytes (the header of this file says what lies where).
inline const char* wd_plan(WdArgs* q, int B, int H, int L, int S, int d, int vec_ok) {
  const char* bad = wd_shape_error(B, H, L, S, d);
  if (bad) return bad;
  q->B = B; q->H = H; q->L = L; q->S = S; q->d = d;
  q->vec = (d % 4 == 0 && vec_ok) ? 4 : 1;
  q->dp = (d + 15) / 16 * 16;
  q->pd = q->dp + 4;
  q->q_nqt = (L + kWdQM - 1) / kWdQM;
  q->q_nkt = (S + kWdQN - 1) / kWdQN;
  q->k_nqt = (L + kWdKM - 1) / kWdKM;
  q->k_nkt = (S + kWdKN - 1) / kWdKN;
  q->lds_q = (int)sizeof(float) * ((3 * kWdQM + 4 * kWdQN) * q->pd + 4 * kWdQM * kWdQPS);
  q->lds_k = (int)sizeof(float) * ((3 * kWdKM + 4 * kWdKN) * q->pd + 3 * kWdKM * kWdKPS);
  if (q->lds_q > kWdMaxLds || q->lds_k > kWdMaxLds) return "the plan needs more than 160 KiB of LDS";   // cannot happen for d <= 128 (155648)
  return nullptr;
}

inline long long wd_stride(const long long* st, int i, int extent) { return extent > 1 ? st[i] : 0; }

#undef WD_MFMA

}  // namespace
}  // namespace bhg

using namespace bhg;

extern "C" {

size_t bhg_attention_wide_ws_bytes(int B, int H, int L) {
  if (!(B > 0 && H > 0 && L > 0)) return 0;
  return wd_ws_bytes(B, H, L);
}

int bhg_attention_wide_plan(int B, int H, int L, int S, int d, int vec_ok, char* buf, size_t buf_bytes) {
  BHG_REQUIRE(buf && buf_bytes > 0, "NULL buffer");
  WdArgs q{};
  const char* bad = wd_plan(&q, B, H, L, S, d, vec_ok);
  BHG_REQUIRE(!bad, bad);
  const int len = snprintf(buf, buf_bytes,
                           "vec=%d bm=%d bn=%d ps=%d kbm=%d kbn=%d kps=%d dp=%d pd=%d grid_q=%lld grid_k=%lld lds_q=%d lds_k=%d max_lds=%d "
                           "ws=%llu",
                           q.vec, kWdQM, kWdQN, kWdQPS, kWdKM, kWdKN, kWdKPS, q.dp, q.pd, (long long)B * H * q.q_nqt,
                           (long long)B * H * q.k_nkt, q.lds_q, q.lds_k, kWdMaxLds, (unsigned long long)wd_ws_bytes(B, H, L));
  BHG_REQUIRE(len > 0 && (size_t)len < buf_bytes, "buffer too small for the plan line");
  return BHG_OK;
}

int bhg_attention_wide_backward_vjp(const float* q, const float* k, const float* v, const float* go, const float* aq, const float* ak,
                                    const float* av, const long long* strides, const float* mask, const long long* mask_strides, int causal,
                                    float scale, int B, int H, int L, int S, int d, float* dq, float* dk, float* dv, float* dgo, void* ws,
                                    size_t ws_bytes, void* stream) {
  WdArgs a{};
  {
    const char* bad = wd_shape_error(B, H, L, S, d);
    BHG_REQUIRE(!bad, bad);
  }
  BHG_REQUIRE(q && k && v && go, "null pointer (q, k, v and go are required)");
  BHG_REQUIRE(aq || ak || av, "all three cotangents are NULL");
  BHG_REQUIRE(dq || dk || dv || dgo, "all four outputs are NULL");
  BHG_REQUIRE(strides, "null pointer (strides)");
  BHG_REQUIRE(!mask || mask_strides, "null pointer (mask_strides)");
  BHG_REQUIRE(ws, "null pointer (workspace)");
  BHG_REQUIRE(ws_bytes >= wd_ws_bytes(B, H, L), "workspace too small (bhg_attention_wide_ws_bytes)");
  BHG_REQUIRE(((uintptr_t)ws & 7) == 0, "the workspace must be 8-byte aligned");
  const float* in[WD_IN] = {q, k, v, go, aq, ak, av};
  const int rows_of[WD_IN] = {L, S, S, L, L, S, S};
  int vec_ok = 1;
  for (int i = 0; i < WD_IN; ++i) {
    a.in[i] = in[i];
    const long long* st = strides + 4 * i;
    BHG_REQUIRE(!in[i] || st[3] == 1, "the last stride of every input must be 1");
    a.st[i][0] = wd_stride(st, 0, B); a.st[i][1] = wd_stride(st, 1, H); a.st[i][2] = wd_stride(st, 2, rows_of[i]);
    if (!in[i]) continue;
    for (int j = 0; j < 3; ++j) {
      BHG_REQUIRE(a.st[i][j] >= 0, "negative stride");
      if (a.st[i][j] % 4 != 0) vec_ok = 0;
    }
  }
  const char* bad = wd_plan(&a, B, H, L, S, d, vec_ok);
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
      a.mst[j] = wd_stride(mask_strides, j, ext[j]);
      BHG_REQUIRE(a.mst[j] >= 0, "negative stride");
    }
  }
  a.out[WD_DQ] = dq; a.out[WD_DK] = dk; a.out[WD_DV] = dv; a.out[WD_DGO] = dgo;
  a.ws = static_cast<double*>(ws);
  a.causal = causal != 0;
  a.scale = scale;
  // above 64 KiB a kernel's dynamic LDS has to be allowed, once per process and device
  static bool attr_done[64] = {};
  int dev = 0;
  BHG_HIP_CHECK(hipGetDevice(&dev));
  using Kernel = void (*)(const WdArgs);
  static const Kernel kq[2][4] = {{k_attn_wide_q<1, 5>, k_attn_wide_q<1, 6>, k_attn_wide_q<1, 7>, k_attn_wide_q<1, 8>},
                                  {k_attn_wide_q<4, 5>, k_attn_wide_q<4, 6>, k_attn_wide_q<4, 7>, k_attn_wide_q<4, 8>}};
  static const Kernel kk[2][4] = {{k_attn_wide_k<1, 5>, k_attn_wide_k<1, 6>, k_attn_wide_k<1, 7>, k_attn_wide_k<1, 8>},
                                  {k_attn_wide_k<4, 5>, k_attn_wide_k<4, 6>, k_attn_wide_k<4, 7>, k_attn_wide_k<4, 8>}};
  if (dev < 0 || dev >= 64 || !attr_done[dev]) {
    for (int i = 0; i < 2; ++i)
      for (int j = 0; j < 4; ++j) {
        BHG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kq[i][j]), hipFuncAttributeMaxDynamicSharedMemorySize, kWdMaxLds));
        BHG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kk[i][j]), hipFuncAttributeMaxDynamicSharedMemorySize, kWdMaxLds));
      }
    if (dev >= 0 && dev < 64) attr_done[dev] = true;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned grid_q = (unsigned)((long long)B * H * a.q_nqt), grid_k = (unsigned)((long long)B * H * a.k_nkt);
  const int vi = a.vec == 4 ? 1 : 0, ci = a.dp / 16 - 5;   // the instance: global read width, d rounded up to 16
  hipLaunchKernelGGL(kq[vi][ci], dim3(grid_q), dim3(kThreads), a.lds_q, st, a);
  BHG_HIP_CHECK(hipGetLastError());
  if (dk || dv) {
    hipLaunchKernelGGL(kk[vi][ci], dim3(grid_k), dim3(kThreads), a.lds_k, st, a);
    BHG_HIP_CHECK(hipGetLastError());
  }
  return BHG_OK;
}

}  // extern "C"
