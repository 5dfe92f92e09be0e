// bhg_groupnorm.hip — the Hessian-vector product's share of a group-normalisation layer, fused.
//
// Where it sits on the path: betty/hypergradient/cg.py:39-41 / neumann.py:62 take H p as the DOUBLE BACKWARD
// `torch.autograd.grad(in_grad, params, grad_outputs=p)`.  nn.GroupNorm is the normalisation of bilevel ResNets whose inner batches are
// too small for batch norm, and ATen's derivative formula for it switches to infinitely_differentiable_native_group_norm_backward as soon
// as grad mode is on: under create_graph=True even the FIRST backward is a chain of element-wise operators, the double backward a longer one.
//
// x is [N, C, *spatial], HW = prod(spatial), G | C, Cg = C / G.  Row (n, g) is the D = Cg * HW contiguous elements of the channels
// g * Cg .. g * Cg + Cg - 1; the channel of row element j is ch(j) = g * Cg + j / HW.  xh = (x - mean_ng) * rstd_ng, y = gamma_ch * xh + beta_ch.
// The backward is the map
//     F : (x, gy, gamma) -> (gx, ggamma, gbeta)
//         g = gamma_ch * gy        m1 = mean_j g        m2 = mean_j (g * xh)
//         gx = rstd * (g - m1 - xh * m2)        ggamma_c = sum_{n,hw} gy * xh        gbeta_c = sum_{n,hw} gy
// and one Hessian-vector product needs its VECTOR-JACOBIAN product: given cotangents (a, b, c) of (gx, ggamma, gbeta), the gradients of
//     Phi = <a, gx> + <b, ggamma> + <c, gbeta>
// with respect to x, gy and gamma — mean and rstd being functions of x.  With the per-row means
//     A0 = mean a     A1 = mean (a * xh)     Sag = mean (a * g)     B0 = mean (b_ch * gy)     B1 = mean (b_ch * gy * xh)
// and at = a - A0 - xh * A1 they are (float64 restatement and its check against autograd: tests/groupnorm_ref.py)
//     dgy      = gamma_ch * rstd * at + b_ch * xh + c_ch
//     dgamma_c = sum_{n,hw} gy * rstd * at
//     q        = -rstd * (g * A1 + m2 * a) + b_ch * gy            t = rstd * (Sag - m1 * A0 - m2 * A1)
//     dx       = rstd * (q - mean q - xh * mean (q * xh)) - rstd * xh * t
//     mean q = -rstd * (m1 * A1 + m2 * A0) + B0        mean (q * xh) = -2 * rstd * m2 * A1 + B1
// mean xh = 0 and mean xh^2 = 1 are NOT used (they hold only to rounding for the fp32 statistics the forward saved): these are layer
// norm's seven row sums (bhg_layernorm.hip) with the per-column parameters replaced by per-channel ones.
//
// TWO launches.  The row pass takes the N * G rows in two regimes:
//   resident (D <= 8192), k_gn_vjp_rows<VEC, NV>: a row lives in registers between its sums and its outputs — x, gy, a read once, dx, dgy
//     written once, 20 algorithmic bytes per element; short rows sit side by side in a workgroup.  One workgroup per row group: the grid is
//     the row groups themselves, no slice bound.
//   streamed (8192 < D <= 2^20), k_gn_vjp_rows_streamed<VEC>: one workgroup per row makes two rounds over it in tiles of 2048 elements —
//     sums, then outputs; the second round rereads x, gy, a: 32 bytes per element.
// dgamma: the row pass leaves every term gy * rstd * at of a row (resp. tile) in LDS as fp64, adds the terms of each channel's segment in
// a fixed order (gn_piece_sums: a tree of 16-element chunks, laid out by the shape alone) and writes fp64 partials part[n][c];
// k_gn_vjp_combine adds part[0 .. N-1][c] in sample order.  Not launched, and nothing staged or written, when dgamma is not wanted.
// No atomics, no grid barrier: bitwise run-to-run deterministic, like the rest of the library.
//
// Layout: fp32, contiguous.  D % 4 == 0: every access of the row tensors is a 16-byte vector (a vector may hold lanes of two or more
// channels when HW % 4 != 0: the channel is worked out per lane); otherwise scalar accesses.  gamma, b, c: scalar loads.
#include "bhg_common.hpp"

#include <limits.h>

namespace bhg {
namespace {

constexpr int kGnResidentD = 8192;   // 32 elements per thread and array at 256 threads per row
constexpr int kGnMaxD = 1 << 20;     // one workgroup per row: a longer row would want several (a grid rendezvous: not in this library)
constexpr int kGnTile = 2048;        // elements per tile of the streamed regime: 16 KiB of fp64 terms in LDS
constexpr int kGnSums = 7;
constexpr int kGnChunk = 16, kGnChunkLog = 4;   // gn_piece_sums: every pass shortens a channel's list of terms sixteenfold

struct GnArgs {
  const float* x; const float* gy; const float* a;      // a may be NULL (cotangent of gx not defined: treated as zero)
  const float* gamma;                                   // [C], may be NULL (affine = False: gamma = 1)
  const float* mean; const float* rstd;                 // [N * G]
  const float* b; const float* c;                       // [C], may be NULL (zero)
  float* dx; float* dgy; float* dgamma;                 // dgamma may be NULL (no terms staged, no partials, no combine pass)
  double* part;                                         // [N][C] = [N * G][Cg]
  long long N, NG;                                      // samples, rows
  int C, G, Cg, HW, D;
  float inv_hw;                                         // 1 / HW in fp32: j / HW is a multiplication and a correction (gn_div)
  int streamed;                                         // 0: resident, 1: streamed
  int vec;                                              // 4: 16-byte accesses (D % 4 == 0); 1: scalar
  int tpr, ltpr;                                        // threads per row (a power of two <= 256) and its log2
  int rows;                                             // 256 / tpr rows side by side: one row group = one workgroup
  int nv;                                               // vectors per thread: ceil((D / vec) / tpr)
  int inst;                                             // resident: the kernel instance's vectors per thread; streamed: those per tile
  long long groups;                                     // row groups = workgroups of the row pass, none empty
};

template <int VEC>
__device__ __forceinline__ void gn_load(const float* __restrict__ p, float* v) {
  if (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = p[0];
  }
}
template <int VEC>
__device__ __forceinline__ void gn_store(float* __restrict__ p, const float* v) {
  if (VEC == 4)
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else
    p[0] = v[0];
}

// The three register-pressure devices of bhg_layernorm.hip (no instruction each): a fence that keeps the gamma / b / c fetches of a whole
// row from gathering in front of the arithmetic, and a value the compiler cannot trace, so that addresses are computed where they are used.
__device__ __forceinline__ void gn_fence() { asm volatile("" ::: "memory"); }
__device__ __forceinline__ int gn_opaque(int v) { asm volatile("" : "+v"(v)); return v; }

// j / d for 0 <= j < 2^21, 1 <= d < 2^21, inv = fl(1 / d): both operands are exact in fp32, the product is off by less than 1/2, so the
// truncated quotient is off by at most one in either direction: one correction.  No integer division per element.
__device__ __forceinline__ int gn_div(const int j, const int d, const float inv) {
  const int q = (int)((float)j * inv);
  const int r = j - q * d;
  return q + (r >= d ? 1 : 0) - (r < 0 ? 1 : 0);
}

// Column of element e (vector e / VEC, lane e % VEC) of thread tv of a row: may lie past the row's end (the caller masks).
template <int VEC>
__device__ __forceinline__ int gn_col(const int e, const int tv, const int tpr) { return (tv + (e / VEC) * tpr) * VEC + e % VEC; }

// The kGnSums sums over the tpr threads of a row, valid in every thread of the row, as ln_row_sums: tpr < 64: a butterfly inside the wave
// (both partners add the same two numbers: the same bits); tpr >= 64: the wave sum, then the row's waves in wave order through LDS.
// Contains barriers when tpr > 64: every thread of the workgroup calls it.
__device__ __forceinline__ void gn_row_sums(double (&s)[kGnSums], const int tpr, double* red) {
  if (tpr >= 64) {
#pragma unroll
    for (int i = 0; i < kGnSums; ++i) s[i] = wave_sum(s[i]);
  } else {
    for (int m = tpr >> 1; m > 0; m >>= 1) {
#pragma unroll
      for (int i = 0; i < kGnSums; ++i) s[i] += __shfl_xor(s[i], m);
    }
  }
  if (tpr > 64) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();  // protect `red` against its previous use
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < kGnSums; ++i) red[i * kWaves + wave] = s[i];
    }
    __syncthreads();
    const int nw = tpr >> 6, w0 = (wave / nw) * nw;
#pragma unroll
    for (int i = 0; i < kGnSums; ++i) {
      double t = 0.0;
      for (int j = 0; j < nw; ++j) t += red[i * kWaves + w0 + j];
      s[i] = t;
    }
  }
}

// term[0 .. len) holds one fp64 term per row element j0 .. j0 + len - 1 (visible to the nt threads that call this: a barrier lies behind
// the writes).  The channel edges (multiples of HW) cut it into np pieces: piece 0 is [0, min(e0, len)), e0 = the distance from j0 to the
// next edge, piece p > 0 starts at e0 + (p - 1) * HW.  Afterwards the sum of piece p stands at the piece's first slot.
// Every pass cuts each piece's list into chunks of 16, adds a chunk in index order and writes chunk i's sum to the piece's slot i: the
// list shrinks sixteenfold in place.  Chunk (p, i) reads slots that only chunks of the same or a higher index write, and chunks are
// handed out in index order, nt at a time, with a barrier between a round's reads and its writes: no slot is overwritten before it is
// read.  The order of every addition is a function of (j0, len, HW) alone.  All loop bounds are uniform over the workgroup (the
// barriers).  t: this thread's index among the nt.
__device__ __forceinline__ void gn_piece_sums(double* term, const int len, const int HW, const int e0, const int np, const int t, const int nt) {
  const int maxlen = HW < len ? HW : len;
  for (int cur = maxlen, sh = 0; cur > 1; cur = (cur + kGnChunk - 1) >> kGnChunkLog, sh += kGnChunkLog) {
    const int nck = (cur + kGnChunk - 1) >> kGnChunkLog;   // chunks of the longest piece
    const int total = np * nck;
    const float inck = 1.0f / (float)nck;
    for (int base = 0; base < total; base += nt) {
      const int idx = base + t;
      const bool on = idx < total;
      const int p = on ? gn_div(idx, nck, inck) : 0, i = on ? idx - p * nck : 0;
      const int start = p == 0 ? 0 : e0 + (p - 1) * HW;
      int end = e0 + p * HW;
      end = end < len ? end : len;
      const int have = (end - start + (1 << sh) - 1) >> sh;        // what the earlier passes left of this piece
      const int src = start + i * kGnChunk, cnt = on ? have - i * kGnChunk : 0;
      double v[kGnChunk];
#pragma unroll
      for (int u = 0; u < kGnChunk; ++u) {
        const int at = src + u;
        v[u] = term[at < len ? at : len - 1];
      }
      double sum = 0.0;
#pragma unroll
      for (int u = 0; u < kGnChunk; ++u)
        if (u < cnt) sum += v[u];
      __syncthreads();
      if (cnt > 0) term[start + i] = sum;
    }
    __syncthreads();
  }
}

// What an element contributes and receives, once the row's seven means are known.
struct GnRow {
  double mu, r, m2, A0, A1, Q0, Q1, t;
};
__device__ __forceinline__ GnRow gn_row(const double (&s)[kGnSums], const double mu, const double r, const double inv_d) {
  const double m1 = s[0] * inv_d, m2 = s[1] * inv_d, A0 = s[2] * inv_d, A1 = s[3] * inv_d, Sag = s[4] * inv_d;
  const double B0 = s[5] * inv_d, B1 = s[6] * inv_d;
  GnRow w;
  w.mu = mu; w.r = r; w.m2 = m2; w.A0 = A0; w.A1 = A1;
  w.Q0 = -r * (m1 * A1 + m2 * A0) + B0;    // mean q
  w.Q1 = -2.0 * r * m2 * A1 + B1;          // mean (q * xh)
  w.t = r * (Sag - m1 * A0 - m2 * A1);
  return w;
}
__device__ __forceinline__ void gn_add_sums(double (&s)[kGnSums], const double xh, const double gm, const double bb, const double gy,
                                            const double aa) {
  const double gg = gm * gy, bg = bb * gy;
  s[0] += gg;
  s[1] += gg * xh;
  s[2] += aa;
  s[3] += aa * xh;
  s[4] += aa * gg;
  s[5] += bg;
  s[6] += bg * xh;
}
// (dx, dgy, the element's term of dgamma)
__device__ __forceinline__ void gn_outputs(const GnRow& w, const double xh, const double gm, const double bb, const double cv, const double gy,
                                           const double aa, float& ox, float& og, double& term) {
  const double at = aa - w.A0 - xh * w.A1;
  og = (float)(gm * w.r * at + bb * xh + cv);
  term = gy * w.r * at;
  const double qv = -w.r * (gm * gy * w.A1 + w.m2 * aa) + bb * gy;
  ox = (float)(w.r * (qv - w.Q0 - xh * w.Q1) - w.r * xh * w.t);
}

// Row group grp: the rows grp * rows + tr, tr = thread / tpr; thread tv = thread % tpr of a row owns the vectors tv, tv + tpr, ... (< NV of
// them).  LDS: the row sums' exchange first, then — the same bytes — one fp64 term per element for dgamma.  Contains barriers: every
// thread of the workgroup calls it.
template <int VEC, int NV>
__device__ __forceinline__ void gn_row_group(const GnArgs& q, const long long grp, double* lds) {
  constexpr int E = VEC * NV;
  const int tid = threadIdx.x, tpr = q.tpr, tv = tid & (tpr - 1), tr = tid >> q.ltpr;
  const int nvec = q.D / VEC, HW = q.HW;
  const float inv_hw = q.inv_hw;
  const double inv_d = 1.0 / (double)q.D;
  const bool has_a = q.a != nullptr, want_dgamma = q.dgamma != nullptr;
  const long long row = grp * q.rows + tr;
  const bool live = row < q.NG;
  const int cb = live ? (int)(row % q.G) * q.Cg : 0;   // the row's first channel
  // An absent gamma / b / c is read as element 0 of `mean` (N * G >= 1) and the value discarded: a select per element, where a test of
  // the pointer is a branch around every fetch.
  const bool hg = q.gamma != nullptr, hb = q.b != nullptr, hc = q.c != nullptr;
  const float* __restrict__ gp = hg ? q.gamma + cb : q.mean;
  const float* __restrict__ bp = hb ? q.b + cb : q.mean;
  const float* __restrict__ cp = hc ? q.c + cb : q.mean;
  const int mg = hg ? -1 : 0, mb = hb ? -1 : 0, mc = hc ? -1 : 0;

  // addresses: a workgroup-uniform 64-bit base (the row group) plus a 32-bit offset (< 256 * 32 elements) per thread and vector
  const long long gbase = grp * q.rows * q.D;
  const float* __restrict__ xg = q.x + gbase;
  const float* __restrict__ gyg = q.gy + gbase;
  const float* __restrict__ ag = has_a ? q.a + gbase : nullptr;
  const unsigned rbase = (unsigned)(tr * q.D);
  float xv[E], gv[E], av[E];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int v = tv + k * tpr;
    const bool in = v < nvec;
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
      xv[k * VEC + u] = 0.f; gv[k * VEC + u] = 0.f; av[k * VEC + u] = 0.f;
    }
    if (in && live) {
      const unsigned off = rbase + (unsigned)(v * VEC);
      gn_load<VEC>(xg + off, xv + k * VEC);
      gn_load<VEC>(gyg + off, gv + k * VEC);
      if (has_a) gn_load<VEC>(ag + off, av + k * VEC);
    }
  }
  const double mu = live ? (double)q.mean[row] : 0.0, r = live ? (double)q.rstd[row] : 0.0;
  // elements outside the row (or rows outside the tensor) were loaded as zeros of gy and a: every term below carries one of the two
  double s[kGnSums];
#pragma unroll
  for (int i = 0; i < kGnSums; ++i) s[i] = 0.0;
  // gamma, b, c are fetched where they are used, in both passes over the row, not held: they stay in the cache.  The channel of an
  // element is worked out per lane (a 16-byte vector may straddle a channel edge).
  const int tv1 = gn_opaque(tv);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int col = gn_col<VEC>(e, tv1, tpr), cc = col < q.D ? col : 0, lc = gn_div(cc, HW, inv_hw);
    const double xh = ((double)xv[e] - mu) * r;
    const float lg = gp[lc & mg], lb = bp[lc & mb];   // fetched whether present or not
    gn_add_sums(s, xh, hg ? (double)lg : 1.0, hb ? (double)lb : 0.0, (double)gv[e], (double)av[e]);
    if (E > 8 && (e & 1) == 1) gn_fence();
  }
  gn_row_sums(s, tpr, lds);
  // The row is held as the fp32 values that were loaded, nothing else (bhg_layernorm.hip): no instruction.
#pragma unroll
  for (int e = 0; e < E; ++e) asm volatile("" : "+v"(xv[e]), "+v"(gv[e]), "+v"(av[e]));
  const GnRow w = gn_row(s, mu, r, inv_d);
  const int width = tpr * E;   // >= D: a row's share of the LDS; rows * width = kThreads * E
  double* term = lds + tr * width;
  if (want_dgamma) __syncthreads();   // uniform.  The exchange has been read: the terms may take its place
  const int tv2 = gn_opaque(tv);
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    float ox[VEC], og[VEC];
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
      const int e = k * VEC + u;
      const int col = gn_col<VEC>(e, tv2, tpr), cc = col < q.D ? col : 0, lc = gn_div(cc, HW, inv_hw);
      const double xh = ((double)xv[e] - mu) * r;
      const float lg = gp[lc & mg], lb = bp[lc & mb], lcv = cp[lc & mc];
      double tm;
      gn_outputs(w, xh, hg ? (double)lg : 1.0, hb ? (double)lb : 0.0, hc ? (double)lcv : 0.0, (double)gv[e], (double)av[e], ox[u], og[u], tm);
      if (want_dgamma) term[col] = tm;   // col < width
    }
    const int v = tv2 + k * tpr;
    if (v < nvec && live) {
      const unsigned off = rbase + (unsigned)(v * VEC);
      gn_store<VEC>(q.dx + gbase + off, ox);
      gn_store<VEC>(q.dgy + gbase + off, og);
    }
    if (E > 8 && ((k * VEC + VEC - 1) & 3) == 3) gn_fence();
  }
  if (!want_dgamma) return;   // uniform over the workgroup
  __syncthreads();
  gn_piece_sums(term, q.D, HW, HW, q.Cg, tv, tpr);   // a whole row: Cg pieces of HW, the first edge at HW
  if (live) {
    double* out = q.part + row * q.Cg;
    for (int lc = tv; lc < q.Cg; lc += tpr) out[lc] = term[lc * HW];
  }
}

// grid = row groups: one workgroup each, no slice bound.  The launch asks for exactly `groups` workgroups, so the loop runs once; it is a
// loop all the same: as straight-line code the widest scalar instance <1, 32> does not fit the register file (504 registers and a private
// segment, against 291 registers in a loop body; scripts/check_spills.py).
template <int VEC, int NV>
__global__ __launch_bounds__(kThreads) void k_gn_vjp_rows(GnArgs q) {
  __shared__ double lds[kThreads * VEC * NV];   // >= 512 doubles: holds the kGnSums * kWaves of the exchange
  for (long long grp = blockIdx.x; grp < q.groups; grp += gridDim.x) gn_row_group<VEC, NV>(q, grp, lds);
}

// grid = rows, one workgroup each.  Two rounds over the row in tiles of kGnTile elements (U vectors per thread and tile): the seven sums,
// then the outputs; the terms of dgamma tile by tile through LDS.  A channel that several tiles share is added up in tile order in its
// fp64 partial: the thread that owns the tile's first piece adds to what an earlier tile's owner wrote (barriers lie between).
template <int VEC>
__global__ __launch_bounds__(kThreads) void k_gn_vjp_rows_streamed(GnArgs q) {
  constexpr int U = kGnTile / (kThreads * VEC), E = U * VEC;
  __shared__ double red[kGnSums * kWaves];
  __shared__ double term[kGnTile];
  const int tid = threadIdx.x, D = q.D, HW = q.HW;
  const float inv_hw = q.inv_hw;
  const long long row = blockIdx.x;
  const bool has_a = q.a != nullptr, want_dgamma = q.dgamma != nullptr;
  const int cb = (int)(row % q.G) * q.Cg;
  const bool hg = q.gamma != nullptr, hb = q.b != nullptr, hc = q.c != nullptr;
  const float* __restrict__ gp = hg ? q.gamma + cb : q.mean;
  const float* __restrict__ bp = hb ? q.b + cb : q.mean;
  const float* __restrict__ cp = hc ? q.c + cb : q.mean;
  const int mg = hg ? -1 : 0, mb = hb ? -1 : 0, mc = hc ? -1 : 0;
  const long long rbase = row * D;
  const float* __restrict__ xr = q.x + rbase;
  const float* __restrict__ gyr = q.gy + rbase;
  const float* __restrict__ ar = has_a ? q.a + rbase : nullptr;
  const double mu = (double)q.mean[row], r = (double)q.rstd[row];

  double s[kGnSums];
#pragma unroll
  for (int i = 0; i < kGnSums; ++i) s[i] = 0.0;
  for (int j0 = 0; j0 < D; j0 += kGnTile) {
    float xv[E], gv[E], av[E];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int j = j0 + (tid + k * kThreads) * VEC;
#pragma unroll
      for (int u = 0; u < VEC; ++u) {
        xv[k * VEC + u] = 0.f; gv[k * VEC + u] = 0.f; av[k * VEC + u] = 0.f;
      }
      if (j < D) {   // D % VEC == 0: a vector lies inside the row or outside
        gn_load<VEC>(xr + j, xv + k * VEC);
        gn_load<VEC>(gyr + j, gv + k * VEC);
        if (has_a) gn_load<VEC>(ar + j, av + k * VEC);
      }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int j = j0 + (tid + (e / VEC) * kThreads) * VEC + e % VEC, jj = j < D ? j : 0, lc = gn_div(jj, HW, inv_hw);
      const double xh = ((double)xv[e] - mu) * r;
      const float lg = gp[lc & mg], lb = bp[lc & mb];
      gn_add_sums(s, xh, hg ? (double)lg : 1.0, hb ? (double)lb : 0.0, (double)gv[e], (double)av[e]);
    }
  }
  gn_row_sums(s, kThreads, red);
  const GnRow w = gn_row(s, mu, r, 1.0 / (double)D);

  double* out = q.part + row * q.Cg;
  for (int j0 = 0; j0 < D; j0 += kGnTile) {
    const int len = D - j0 < kGnTile ? D - j0 : kGnTile;
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int j = j0 + (tid + k * kThreads) * VEC;
      if (j < D) {
        float xv[VEC], gv[VEC], av[VEC], ox[VEC], og[VEC];
#pragma unroll
        for (int u = 0; u < VEC; ++u) av[u] = 0.f;
        gn_load<VEC>(xr + j, xv);
        gn_load<VEC>(gyr + j, gv);
        if (has_a) gn_load<VEC>(ar + j, av);
#pragma unroll
        for (int u = 0; u < VEC; ++u) {
          const int lc = gn_div(j + u, HW, inv_hw);
          const double xh = ((double)xv[u] - mu) * r;
          const float lg = gp[lc & mg], lb = bp[lc & mb], lcv = cp[lc & mc];
          double tm;
          gn_outputs(w, xh, hg ? (double)lg : 1.0, hb ? (double)lb : 0.0, hc ? (double)lcv : 0.0, (double)gv[u], (double)av[u], ox[u], og[u], tm);
          if (want_dgamma) term[j - j0 + u] = tm;
        }
        gn_store<VEC>(q.dx + rbase + j, ox);
        gn_store<VEC>(q.dgy + rbase + j, og);
      }
    }
    if (want_dgamma) {   // uniform over the workgroup
      __syncthreads();
      const int lc0 = j0 / HW;                                    // uniform: one division per tile
      const int e0 = (lc0 + 1) * HW - j0;                         // 1 .. HW: from the tile's start to the next channel edge
      const int np = (j0 + len - 1) / HW - lc0 + 1;
      gn_piece_sums(term, len, HW, e0, np, tid, kThreads);
      for (int p = tid; p < np; p += kThreads) {
        const double v = term[p == 0 ? 0 : e0 + (p - 1) * HW];
        if (p == 0 && e0 != HW) out[lc0] += v;                    // the channel began in an earlier tile
        else out[lc0 + p] = v;
      }
      __syncthreads();                                            // the sums are read before the next tile's terms arrive
    }
  }
}

// grid = ceil(C / 256): one thread per channel adds the samples' partials in sample order.
__global__ __launch_bounds__(kThreads) void k_gn_vjp_combine(const double* __restrict__ part, float* __restrict__ dgamma, const int C,
                                                             const long long N) {
  const int ch = blockIdx.x * kThreads + threadIdx.x;
  if (ch >= C) return;
  double v = 0.0;
  for (long long n = 0; n < N; ++n) v += part[n * C + ch];
  dgamma[ch] = (float)v;
}

// Why the launch does not take a shape, or NULL where it does: bhg_groupnorm_backward_vjp and bhg_groupnorm_plan refuse the same shapes.
inline const char* gn_shape_error(long long N, int C, long long HW, int G) {
  if (!(N > 0 && C > 0 && HW > 0 && G > 0)) return "empty tensor (N, C, HW and G must be positive)";
  if (C % G != 0) return "C is not a multiple of G";
  if (HW > kGnMaxD || (long long)(C / G) * HW > kGnMaxD) return "more than 2^20 elements per row";
  if (N > INT_MAX || N * G > INT_MAX) return "more than 2^31 - 1 rows (N * G): beyond what a grid holds";
  // N * C = (N * G) * (C / G) < 2^31 * 2^20: 8 * N * C and every element offset fit 64 bits with room to spare
  return nullptr;
}

// The geometry, in closed form (tpr comes from a shift loop of at most 8 steps; nothing is searched).
inline const char* gn_plan(GnArgs* q, long long N, int C, long long HW, int G) {
  const char* bad = gn_shape_error(N, C, HW, G);
  if (bad) return bad;
  q->N = N; q->NG = N * G; q->C = C; q->G = G; q->Cg = C / G; q->HW = (int)HW; q->D = q->Cg * (int)HW;
  q->inv_hw = 1.0f / (float)q->HW;
  const int D = q->D;
  q->vec = D % 4 == 0 ? 4 : 1;
  const int nvec = D / q->vec;
  q->streamed = D > kGnResidentD ? 1 : 0;
  if (q->streamed) {
    q->tpr = kThreads; q->ltpr = 8; q->rows = 1;
    q->nv = (nvec + kThreads - 1) / kThreads;
    q->inst = kGnTile / (kThreads * q->vec);
    q->groups = q->NG;
    return nullptr;
  }
  // two vectors per thread until a row takes the whole workgroup: a narrow row leaves no thread idle (256 / tpr rows side by side)
  int tpr = 1, ltpr = 0;
  while (tpr < kThreads && 2 * tpr < nvec) { tpr <<= 1; ++ltpr; }
  q->tpr = tpr; q->ltpr = ltpr;
  q->rows = kThreads / tpr;
  q->nv = (nvec + tpr - 1) / tpr;
  // supported instance counts: 16-byte path 2, 4, 8; scalar path 2, 8, 32 (D <= 8192: nv <= 8 resp. 32)
  if (q->vec == 4) q->inst = q->nv <= 2 ? 2 : q->nv <= 4 ? 4 : 8;
  else q->inst = q->nv <= 2 ? 2 : q->nv <= 8 ? 8 : 32;
  q->groups = (q->NG + q->rows - 1) / q->rows;
  return nullptr;
}

template <int VEC, int NV>
inline void gn_launch_rows(const GnArgs& q, hipStream_t st) {
  hipLaunchKernelGGL((k_gn_vjp_rows<VEC, NV>), dim3((unsigned)q.groups), dim3(kThreads), 0, st, q);
}

}  // namespace
}  // namespace bhg

using namespace bhg;

extern "C" {

size_t bhg_groupnorm_ws_bytes(long long N, int C) {
  if (!(N > 0 && C > 0) || N > (1LL << 58) / C) return 0;
  return sizeof(double) * (size_t)N * (size_t)C;
}

int bhg_groupnorm_plan(long long N, int C, long long HW, int G, char* buf, size_t buf_bytes) {
  BHG_REQUIRE(buf && buf_bytes > 0, "NULL buffer");
  GnArgs q{};
  const char* bad = gn_plan(&q, N, C, HW, G);
  BHG_REQUIRE(!bad, bad);
  const int len = snprintf(buf, buf_bytes, "regime=%d D=%d vec=%d tpr=%d rows=%d nv=%d inst=%d tile=%d groups=%lld grid=%lld ws=%lld", q.streamed,
                           q.D, q.vec, q.tpr, q.rows, q.nv, q.inst, q.streamed ? kGnTile : 0, q.groups, q.groups,
                           (long long)bhg_groupnorm_ws_bytes(N, C));
  BHG_REQUIRE(len > 0 && (size_t)len < buf_bytes, "buffer too small for the plan line");
  return BHG_OK;
}

int bhg_groupnorm_backward_vjp(const float* x, const float* gy, const float* a, const float* gamma, const float* mean, const float* rstd,
                               const float* b, const float* c, long long N, int C, long long HW, int G, float* dx, float* dgy, float* dgamma,
                               void* ws, size_t ws_bytes, void* stream) {
  BHG_REQUIRE(x && gy && mean && rstd && dx && dgy, "null pointer");
  GnArgs q{};
  const char* bad = gn_plan(&q, N, C, HW, G);
  BHG_REQUIRE(!bad, bad);
  if (dgamma) {
    BHG_REQUIRE(ws, "dgamma is wanted but there is no workspace");
    BHG_REQUIRE(ws_bytes >= bhg_groupnorm_ws_bytes(N, C), "workspace smaller than bhg_groupnorm_ws_bytes(N, C)");
    BHG_REQUIRE(((uintptr_t)ws & 7) == 0, "the workspace must be 8-byte aligned");
  }
  if (q.vec == 4)
    for (const void* p : {(const void*)x, (const void*)gy, (const void*)a, (const void*)dx, (const void*)dgy})
      BHG_REQUIRE(((uintptr_t)p & 15) == 0, "x, gy, a, dx and dgy must be 16-byte aligned when a row's length is a multiple of 4");
  q.x = x; q.gy = gy; q.a = a; q.gamma = gamma; q.mean = mean; q.rstd = rstd; q.b = b; q.c = c;
  q.dx = dx; q.dgy = dgy; q.dgamma = dgamma; q.part = static_cast<double*>(ws);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (q.streamed) {
    if (q.vec == 4) hipLaunchKernelGGL((k_gn_vjp_rows_streamed<4>), dim3((unsigned)q.groups), dim3(kThreads), 0, st, q);
    else hipLaunchKernelGGL((k_gn_vjp_rows_streamed<1>), dim3((unsigned)q.groups), dim3(kThreads), 0, st, q);
  } else {
    switch (q.vec * 100 + q.inst) {
      case 402: gn_launch_rows<4, 2>(q, st); break;
      case 404: gn_launch_rows<4, 4>(q, st); break;
      case 408: gn_launch_rows<4, 8>(q, st); break;
      case 102: gn_launch_rows<1, 2>(q, st); break;
      case 108: gn_launch_rows<1, 8>(q, st); break;
      default: gn_launch_rows<1, 32>(q, st); break;
    }
  }
  if (dgamma) hipLaunchKernelGGL(k_gn_vjp_combine, dim3((C + kThreads - 1) / kThreads), dim3(kThreads), 0, st, q.part, dgamma, C, N);
  BHG_HIP_CHECK(hipGetLastError());
  return BHG_OK;
}

}  // extern "C"
