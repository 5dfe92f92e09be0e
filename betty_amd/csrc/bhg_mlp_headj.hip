// bhg_mlp_headj.hip — the head launch of a projected CG iteration in its `head_j` form (k_headj) and the packing kernel of the
// once-per-solve J build (k_headj_pack).  See bhg_mlp_headj.hpp for the identity.  A translation unit of its own: the code object of
// bhg_mlp.o stays as the placement sweep measured it (tests/test_code_placement.py); the fragments this unit needs are #included
// here a second time, inside this unit's own anonymous namespace.
//
// k_headj: three block classes, none of which reads what another one writes.
// (16 x 16 tiles: the tiles come first, [0, nt), and the head rows follow them, [nt, nt + rows) — see k_headj.)
//   [0, rows)            head rows     k_headu's rows (mlp/head_body.inc with BHG_HEAD_J): rz through J_b and the staged row of Rh_1;
//                                      they write Rd_{L-1}, Rz, partT1, Rd_{L-2} (row-major and packed) — not Rh_{L-2}, not T2h
//   [rows, rows + nt)    pre-head tiles Rh_{L-2} = mask (Rh_1 W_2^T + Gf(r') + beta Gf(p) + c_2) on packed operands, 16 x 16 or 32 x 16 per
//                                      workgroup, the whole K inside it (no slabs); each emits its share of T2h = 2 <delta_top V, Rh_{L-2}>
//                                      in fp64.  A tile whose rows hold no sample (m0 >= B) loads nothing and stores its zeros.
//   [rows + nt, ...)     update blocks pstep_body, as in k_headu
// The head rows and the tiles read the OLD slot of Gf_{L-2}(p) (the update blocks write the other one) and beta from the granules.
#include <stdlib.h>

#include "bhg_mlp_headj.hpp"

#ifdef BHG_STAMPS   // (the stamp buffer belongs to bhg_mlp.hip: this unit's kernels carry no stamps)
#undef BHG_STAMP
#define BHG_STAMP(kid, slot) do { } while (0)
#endif

namespace bhg {
namespace {
#include "mlp/gemm.inc"
#include "mlp/outer.inc"
#include "mlp/scalars.inc"
#include "mlp/head.inc"
#include "mlp/wsk.inc"
#include "mlp/wskp.inc"
#include "mlp/recurrence.inc"
#include "mlp/proj.inc"
#include "mlp/pstep.inc"

struct HeadjArgs {
  const float* h; const float* W; const float* V; const float* cb; const float* prob; const float* sd; float* rd;
  int K, C, B, rows;
  const float* delta_top; const float* mask_prev; float* rd_prev; float* rd_prev_p;
  HeadFuse fz;                          // bias, mask, addend (Gf(r')), rh_out; no slabs
  double* partT1; float* rz_out;
  const float* addend2;                 // Gf_{L-2}(p), the OLD slot
  const unsigned long long* gran;       // beta's granules
  const float* J; const float* Rh1; int K1;
  const float* Rh1p; const float* W2p; double* partT2;
  int nt, nu;                           // tiles, update blocks
  int t2n;                              // slots of partT2 the consumer sums (>= nt: the tiles clear the rest)
  double* t2clear;                      // 16 x 16 tiles: partT2 is the pair buffer of this parity; head row b clears slot b of the other one
  alignas(64) PstepArgs ps;             // (pstep_body reads them from the kernarg segment at this offset)
};
static_assert(offsetof(HeadjArgs, ps) % 64 == 0 && sizeof(HeadjArgs) <= 3900, "kernel arguments of k_headj");

constexpr int kHjC = 12;   // classes the form takes (the head's prefetching instance)

// One (16 RBLK) x (16 CBLK) tile of Rh_{L-2}: wskp_tile's K loop (two register stages), the four waves' partial tiles met in LDS in fixed
// order, then the head kernel's combine — (sum + (Gf(r') + beta Gf(p))) + c, times the mask — and the tile's share of T2h.
// Every element is the sum of the same four per-wave partials over the same K ranges whatever the tile shape: Rh_{L-2} has the same bits.
// T2h partials.  PAIR = false: one slot of partT2 per tile; slots [nt, t2n) are cleared here, because the consumer sums t2n of them
// (t2n = B where the tiles took over the head rows' slots, nt behind the layers' own partials otherwise).  PAIR = true (16 x 16): the
// step length's one-round-trip sum takes no more partials than that, so the two row-adjacent tiles of a column tile share a slot of a
// buffer that is zero when the launch starts and add to it with one fp64 atomic each; slots the tiles do not reach stay zero.
template <int RBLK, int CBLK, int D, bool PAIR>
__device__ __forceinline__ void headj_tile(const HeadjArgs& g, const int t, float* __restrict__ sPf, float* __restrict__ sD,
                                           float* __restrict__ sV, double* __restrict__ red) {
  constexpr int TR = 16 * RBLK, TC = 16 * CBLK, TCP = TC + 1;
  static_assert(kWskpWaves * TR * TCP <= kWskpLds && TR <= 32 && TC <= 32 && (TR * TC) % (64 * kWskpWaves) == 0, "four partial tiles");
  const int RA = g.rows, RB = g.K, KT = g.K1, B = g.B, C = g.C;
  const int ntm = RA / TR, ntn = RB / TC;
  // every row tile of a column tile on ONE XCD (workgroup ids go round the eight XCDs; the tiles start at a multiple of 8): the
  // streamed weight-side operand is fetched into one L2 (wskp_body's rule)
  int tm = t % ntm, tn = t / ntm;
  if ((ntn & 7) == 0) { const int j = t >> 3; tm = j % ntm; tn = (j / ntm) * 8 + (t & 7); }
  const int m0 = TR * tm, n0 = TC * tn;
  if (m0 >= B) {   // (workgroup-uniform) no sample in these rows: their outputs are zero, T2h gets nothing from them
    for (int e = threadIdx.x; e < TR * TC; e += 64 * kWskpWaves) g.fz.rh_out[(int64_t)(m0 + e / TC) * RB + n0 + (e % TC)] = 0.f;
    if (!PAIR && threadIdx.x == 0)
      for (int z = t; z < g.t2n; z += g.nt) g.partT2[z] = 0.0;
    return;
  }
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int nct = KT / 32;
  const int c0 = (int)(((int64_t)wave * nct) / kWskpWaves), c1 = (int)(((int64_t)(wave + 1) * nct) / kWskpWaves);
  const int nch_w = c1 - c0;
  f32x4 acc[RBLK][CBLK];
#pragma unroll
  for (int a = 0; a < RBLK; ++a)
#pragma unroll
    for (int b = 0; b < CBLK; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[a][b][r] = 0.f;
  // epilogue operands of this thread's outputs: requested before the K loop, they land under it
  constexpr int kOutPer = TR * TC / (64 * kWskpWaves);
  float e_mask[kOutPer], e_bias[kOutPer], e_add[kOutPer], e_add2[kOutPer];
#pragma unroll
  for (int u = 0; u < kOutPer; ++u) {
    const int e = threadIdx.x + 64 * kWskpWaves * u;
    const int64_t idx = (int64_t)(m0 + e / TC) * RB + n0 + (e % TC);
    e_mask[u] = g.fz.mask[idx];
    e_bias[u] = g.fz.bias[n0 + (e % TC)];
    e_add[u] = g.fz.addend[idx];
    e_add2[u] = (g.addend2 ? g.addend2 : g.fz.addend)[idx];   // (unconditional load, see wskp_tile)
  }
  // delta_top of the tile's rows and V of its columns, for (delta_top V)[b][k] in the epilogue
  for (int e = threadIdx.x; e < TR * C; e += 64 * kWskpWaves) {
    const int r = e / C, c = e - r * C;
    sD[r * kHjC + c] = m0 + r < B ? g.delta_top[(int64_t)(m0 + r) * C + c] : 0.f;
  }
  for (int e = threadIdx.x; e < C * TC; e += 64 * kWskpWaves) {
    const int c = e / TC, j = e % TC;
    sV[c * TC + j] = g.V[(int64_t)c * RB + n0 + j];
  }
  if (nch_w > 0) {   // (wave-uniform)
    const int64_t sA = (int64_t)16 * RA, sB = (int64_t)16 * RB;
    const float* gA = g.Rh1p + (int64_t)(2 * c0) * sA + (m0 + li) * 16 + 4 * lk;
    const float* gB = g.W2p + (int64_t)(2 * c0) * sB + (n0 + li) * 16 + 4 * lk;
    wskp_loop<D, RBLK, CBLK>(gA, gB, sA, sB, nch_w, acc);
  }
  // C/D layout of v_mfma_f32_16x16x4_f32: col = lane & 15, row = 4 * (lane >> 4) + reg
  float* sW = sPf + wave * (TR * TCP);
#pragma unroll
  for (int rb = 0; rb < RBLK; ++rb)
#pragma unroll
    for (int cbk = 0; cbk < CBLK; ++cbk)
#pragma unroll
      for (int r = 0; r < 4; ++r) sW[(16 * rb + 4 * lk + r) * TCP + 16 * cbk + li] = acc[rb][cbk][r];
  __syncthreads();
  const float beta = g.addend2 ? poll_beta(g.gran) : 0.f;
  double t2 = 0.0;
#pragma unroll
  for (int u = 0; u < kOutPer; ++u) {
    const int e = threadIdx.x + 64 * kWskpWaves * u;
    const int row = e / TC, col = e % TC;
    const int m = m0 + row;
    const int64_t idx = (int64_t)m * RB + n0 + col;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < kWskpWaves; ++w) v += sPf[w * (TR * TCP) + row * TCP + col];
    float ad = e_add[u];
    if (g.addend2) ad = add_rn(ad, mul_rn(beta, e_add2[u]));   // the rounding of the recurrence G(p') = G(r') + beta G(p)
    v += ad;
    v = (v + e_bias[u]) * e_mask[u];
    v = m < B ? v : 0.f;
    g.fz.rh_out[idx] = v;
    float dv = 0.f;                                            // (delta_top V)[m][n], the head kernel's order and rounding
    for (int c = 0; c < C; ++c) dv += sD[row * kHjC + c] * sV[c * TC + col];
    if (m < B) t2 += (double)dv * (double)v;
  }
  t2 = wave_sum(t2);   // (fixed order: lanes by DPP, then the four waves)
  if (lane == 0) red[wave] = t2;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kWskpWaves; ++w) s += red[w];
    if constexpr (PAIR) {
      atomicAdd(g.partT2 + tn * (ntm / 2) + (tm >> 1), 2.0 * s);   // (result unused: no return value asked of the memory side)
    } else {
      g.partT2[t] = 2.0 * s;
      for (int z = t + g.nt; z < g.t2n; z += g.nt) g.partT2[z] = 0.0;   // (the consumer sums t2n slots)
    }
  }
}

// TS: the tiles' shape — 0: 32 x 32 (48 workgroups at cfg 2: 5 us of MFMAs each, the launch 17.9 us); 1: 32 x 16 (96 workgroups: the
// launch 11 us; four register stages instead of two: 1 us slower); 2: 16 x 16, T2h by pairs (192 workgroups, 24 of them without a
// sample at B = 100).  Same-box arms, profiles/head_j_ab.txt and profiles/head_j_tiles_ab.txt.
// D: register stages of the tiles' K loop (four with 16 x 16 tiles: 0.15 us slower than two, not kept).  TF: the tiles take the launch's
// first workgroups and the head rows follow them — the 16 x 16 shape's default: the tiles are the launch's critical path, and dispatched
// first they gain 0.6 us per iteration over rows first (same-box arms, profiles/head_j_tiles_ab.txt); the coarser shapes stay rows first.
template <int U, int TS, int D, bool TF>
__global__ __launch_bounds__(256) void k_headj(HeadjArgs g) {
  static_assert(64 * kWskpWaves == 256, "the tiles run in the head launch's workgroups");
  const int bx = (int)blockIdx.x;
  if (bx >= g.rows + g.nt) { pstep_body<U, (int)offsetof(HeadjArgs, ps), false>(bx - g.rows - g.nt); return; }
  if (TF ? bx < g.nt : bx >= g.rows) {
    __shared__ float sPf[kWskpLds];
    __shared__ float sD[32 * kHjC], sV[kHjC * 32];
    __shared__ double red[kWskpWaves];
    const int t = TF ? bx : bx - g.rows;
    if constexpr (TS == 0) headj_tile<2, 2, D, false>(g, t, sPf, sD, sV, red);
    else if constexpr (TS == 1) headj_tile<2, 1, D, false>(g, t, sPf, sD, sV, red);
    else headj_tile<1, 1, D, true>(g, t, sPf, sD, sV, red);
    return;
  }
  const int hrow = TF ? bx - g.nt : bx;   // this workgroup's head row
  if (TS == 2 && threadIdx.x == 0) g.t2clear[hrow] = 0.0;   // (its consumer, the closing launch of the iteration before, is long done)
  const float* __restrict__ Rh = nullptr; const float* __restrict__ h = g.h; const float* __restrict__ W = g.W;
  const float* __restrict__ V = g.V; const float* __restrict__ cb = g.cb; const float* __restrict__ prob = g.prob;
  const float* __restrict__ sd = g.sd; float* __restrict__ rd = g.rd;
  const int K = g.K, C = g.C, B = g.B;
  constexpr int mode = HEAD_JVP;
  const int64_t* __restrict__ labels = nullptr; float* __restrict__ aux = nullptr; const float* __restrict__ delta_top = g.delta_top;
  const float* __restrict__ mask_prev = g.mask_prev; float* __restrict__ rd_prev = g.rd_prev;
  const HeadFuse fz = g.fz;
  double* __restrict__ partT1 = g.partT1; double* __restrict__ partT2h = nullptr; float* __restrict__ rz_out = g.rz_out;
  double* __restrict__ rzx_acc = nullptr; const int rzx_first = 0; float* __restrict__ rd_prev_p = g.rd_prev_p;
  const float* __restrict__ lazy_addend2 = g.addend2;
  const float lazy_beta = g.addend2 ? poll_beta(g.gran) : 0.f;   // (published two launches ago: the first load returns it)
  const float* __restrict__ hj_J = g.J; const float* __restrict__ hj_Rh1 = g.Rh1; const int hj_K1 = g.K1;
  constexpr bool HAS_RH = true, FUSED = true, PF = true;
  constexpr int JMAX = 3;
  (void)Rh; (void)labels; (void)aux; (void)rzx_acc; (void)rzx_first;
#define BHG_HEAD_B (hrow)
#define BHG_HEAD_ROWS (g.rows)
#define BHG_HEAD_LAZY 1
#define BHG_HEAD_J 1
#include "mlp/head_body.inc"
#undef BHG_HEAD_B
#undef BHG_HEAD_ROWS
#undef BHG_HEAD_LAZY
#undef BHG_HEAD_J
}

// A[b C + c][k] = W_3[c][k] mask_2[b][k] in the packed layout [K / 16][RA][16]: one float4 of the output per thread (k_pack's indexing)
// Ahead of its share, workgroup 0 clears `zero` and workgroup 1 (0 in a launch of one) copies csrc to cdst: what a memset and a copy of
// the runtime did in two launches of their own on the solve's dependent chain.  Nothing in this launch reads either.
__global__ __launch_bounds__(256) void k_headj_pack(const float* __restrict__ W3, const float* __restrict__ mask2, float* __restrict__ Ap,
                                                    const int B, const int C, const int K, const int RA, double* __restrict__ zero,
                                                    const int nzero, const float* __restrict__ csrc, float* __restrict__ cdst,
                                                    const int ncopy4) {
  if (zero && blockIdx.x == 0)
    for (int i = threadIdx.x; i < nzero; i += 256) zero[i] = 0.0;
  if (csrc && blockIdx.x == (gridDim.x > 1 ? 1u : 0u))
    for (int i = threadIdx.x; i < ncopy4; i += 256)
      reinterpret_cast<f32x4*>(cdst)[i] = reinterpret_cast<const f32x4*>(csrc)[i];
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = (int64_t)RA * K / 4;
  if (idx >= total) return;
  const int c4 = (int)(idx & 3);
  const int64_t rr = idx >> 2;
  const int r = (int)(rr % RA), kb = (int)(rr / RA);
  const int k = 16 * kb + 4 * c4;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (r < B * C) {
    const int b = r / C, c = r - b * C;
    const f32x4 w = *reinterpret_cast<const f32x4*>(W3 + (int64_t)c * K + k);
    const f32x4 mk = *reinterpret_cast<const f32x4*>(mask2 + (int64_t)b * K + k);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = w[j] * mk[j];
  }
  *reinterpret_cast<f32x4*>(Ap + idx * 4) = v;
}
}  // namespace

int headj_tiles(int rows, int K, int shape) { return (rows / (shape == 2 ? 16 : 32)) * (K / (shape == 0 ? 32 : 16)); }

int launch_headj(const HeadjLaunch& a, hipStream_t st) {
  BHG_REQUIRE(a.C >= 1 && a.C <= kHjC && a.K >= 32 && a.K <= 512 && a.K % 32 == 0 && a.K1 >= 32 && a.K1 % 32 == 0 && a.rows % 32 == 0 &&
              a.B >= 1 && a.B <= a.rows, "k_headj was planned for a head it cannot run");
  BHG_REQUIRE(a.ps && a.ps_bytes == sizeof(PstepArgs) && a.nu >= 0, "the update blocks' arguments do not match this build");
  BHG_REQUIRE(a.J && a.Rh1 && a.Rh1p && a.W2p && a.rh_out && a.partT2 && a.addend && a.bias2 && a.mask2 && a.rd_prev && a.delta_top &&
              a.mask_prev, "NULL argument");
  HeadjArgs g{};
  g.h = a.h; g.W = a.W; g.V = a.V; g.cb = a.cb; g.prob = a.prob; g.sd = a.sd; g.rd = a.rd;
  g.K = a.K; g.C = a.C; g.B = a.B; g.rows = a.rows;
  g.delta_top = a.delta_top; g.mask_prev = a.mask_prev; g.rd_prev = a.rd_prev; g.rd_prev_p = a.rd_prev_p;
  g.fz = HeadFuse{nullptr, 0, a.rows * a.K, a.bias2, a.mask2, a.rh_out, a.addend};
  g.partT1 = a.partT1; g.rz_out = a.rz_out; g.addend2 = a.addend2; g.gran = a.gran;
  g.J = a.J; g.Rh1 = a.Rh1; g.K1 = a.K1; g.Rh1p = a.Rh1p; g.W2p = a.W2p; g.partT2 = a.partT2;
  g.nt = headj_tiles(a.rows, a.K, a.tile_shape); g.nu = a.nu; g.t2n = a.t2n;
  BHG_REQUIRE(a.tile_shape >= 0 && a.tile_shape <= 2, "unknown tile shape");
  if (a.tile_shape == 2) {
    BHG_REQUIRE(a.t2pair && a.t2clear && a.t2pair != a.t2clear && g.nt / 2 <= a.B, "16 x 16 tiles: one T2h slot per pair, in a buffer per parity");
    g.partT2 = a.t2pair; g.t2clear = a.t2clear;
  } else {
    BHG_REQUIRE(a.t2n >= g.nt, "fewer T2h slots than tiles");
  }
  memcpy(&g.ps, a.ps, sizeof(PstepArgs));
  const dim3 grid(a.rows + g.nt + g.nu);
  const size_t lds = (size_t)a.K * sizeof(float);
#ifdef BHG_AB   // (debug keys head_j_tile, head_j_stages4, head_j_tiles_first: the arms of the 16 x 16 shape)
  if (a.tile_shape == 0) hipLaunchKernelGGL((k_headj<4, 0, 2, false>), grid, dim3(256), lds, st, g);
  else if (a.tile_shape == 2 && a.stages4) hipLaunchKernelGGL((k_headj<4, 2, 4, false>), grid, dim3(256), lds, st, g);
  else if (a.tile_shape == 2 && !a.tiles_first) hipLaunchKernelGGL((k_headj<4, 2, 2, false>), grid, dim3(256), lds, st, g);
  else
#endif
  if (a.tile_shape == 2) hipLaunchKernelGGL((k_headj<4, 2, 2, true>), grid, dim3(256), lds, st, g);
  else hipLaunchKernelGGL((k_headj<4, 1, 2, false>), grid, dim3(256), lds, st, g);
  return BHG_OK;
}

int launch_headj_pack(const float* W3, const float* mask2, float* Ap, int B, int C, int K, int RA, double* zero, int nzero,
                      const float* csrc, float* cdst, int ncopy, hipStream_t st) {
  BHG_REQUIRE(W3 && mask2 && Ap && B >= 1 && C >= 1 && K >= 16 && K % 16 == 0 && RA >= 32 && RA % 32 == 0 && RA >= B * C, "bad arguments");
  BHG_REQUIRE(!zero || nzero >= 0, "bad size of the buffer to clear");
  BHG_REQUIRE(!csrc || (cdst && ncopy >= 0 && ncopy % 4 == 0 && (((uintptr_t)csrc | (uintptr_t)cdst) & 15) == 0),
              "the slice to copy must be 16-byte aligned, its length a multiple of 4");
  const int64_t total = (int64_t)RA * K / 4;
  hipLaunchKernelGGL(k_headj_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, W3, mask2, Ap, B, C, K, RA, zero, nzero, csrc,
                     cdst, ncopy / 4);
  return BHG_OK;
}

}  // namespace bhg
