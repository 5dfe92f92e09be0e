// bhg_mlp_headj.hpp — what bhg_mlp.hip and bhg_mlp_headj.hip share: the arguments of the head launch of a projected CG iteration in
// its `head_j` form and of the kernel that packs the operand of the once-per-solve J build.  The device code lives in
// bhg_mlp_headj.hip, a translation unit of its own (the placement of the K-loop kernels inside bhg_mlp.o is pinned, see
// tests/test_code_placement.py); bhg_mlp.hip only fills these structs and calls the launchers.
//
// The identity.  With L = 4, the head row of sample b needs the pre-head product only through the C <= 12 classes:
//     sum_k W_3[c][k] Rh_2[b][k]  =  J_b[c] . Rh_1[b]  +  sum_k W_3[c][k] mask_2[b][k] (addend[b][k] + c_2[k])
//     J_b = W_3 diag(mask_2[b]) W_2                       (C x d_2 per sample; weights and ReLU masks only: constant over a solve)
// so the head rows depend on Rh_1 (the first product's output) and no longer on the pre-head product, whose tiles — Rh_2 itself is
// still read by the closing launch — become a third block class of the head launch.
#pragma once
#include <stddef.h>

#include "bhg_common.hpp"

namespace bhg {

struct HeadjLaunch {
  // ---- head rows (one workgroup per padded batch row): k_headu's arguments ...
  const float* h; const float* W; const float* V; const float* cb; const float* prob; const float* sd; float* rd;
  int K, C, B, rows;                        // K = d_3 (last hidden width), C classes, B valid rows of `rows` (= the padded batch)
  const float* delta_top; const float* mask_prev; float* rd_prev; float* rd_prev_p;
  double* partT1; float* rz_out;
  const float* bias2; const float* mask2;   // c_2 [K], mask_2 [rows][K]
  const float* addend; const float* addend2; const unsigned long long* gran;   // Gf_2(r'), the OLD slot of Gf_2(p), beta's granules
  // ... and what replaces the pre-head product in them
  const float* J;                           // [round32(B C)][K1] row-major, row b C + c
  const float* Rh1;                         // Rh_1 [rows][K1] row-major
  int K1;                                   // d_2
  // ---- pre-head tiles (one workgroup each, the whole K1 inside the workgroup)
  const float* Rh1p; const float* W2p;      // packed operands [K1 / 16][rows][16], [K1 / 16][K][16]
  float* rh_out;                            // Rh_2 [rows][K] row-major
  double* partT2; int t2n;                  // one fp64 partial of T2h per tile; the consumer sums t2n >= tiles slots (the rest cleared)
  // ... or, with 16 x 16 tiles (shape 2), one slot per PAIR of row-adjacent tiles: t2pair != NULL is a buffer of `rows` doubles that is
  // zero when the launch starts; both tiles of a pair add their partial to slot `pair` (two addends onto an exact zero: the sum does
  // not depend on their order).  t2clear: the buffer of the other iteration parity, whose slot b head row b clears for the next launch.
  double* t2pair; double* t2clear;
  int tile_shape;                           // headj_tile_shape(), or the measurement build's debug key head_j_tile
  int stages4;                              // measurement build only (key head_j_stages4): four register stages, rows first
  int tiles_first;                          // 16 x 16 tiles: dispatched ahead of the head rows (default; key head_j_tiles_first = 0: behind them)
  // ---- update blocks: a PstepArgs (mlp/pstep.inc), copied as bytes
  const void* ps; size_t ps_bytes; int nu;
};
constexpr int kHeadjTile = 1;               // 32 x 16 tiles (0: 32 x 32; 2: 16 x 16, T2h by pairs)
constexpr int kHeadjFineMax = 192;          // the most 16 x 16 tiles the plan asks for (d_3 = 384 at 128 rows: the count it was measured at)
int headj_tiles(int rows, int K, int shape);   // workgroups of the tile class (shapes 0 and 1: = T2h partials; shape 2: two per partial)
// The shape the plan picks: 16 x 16 where their pairs fit the B slots the step length's sum reads (and no more than kHeadjFineMax
// tiles), else 32 x 16 as before
inline int headj_tile_shape(int rows, int K, int B) {
  const int nt = (rows / 16) * (K / 16);
  return (nt / 2 <= B && nt <= kHeadjFineMax) ? 2 : kHeadjTile;
}
int launch_headj(const HeadjLaunch& a, hipStream_t st);

// A[b C + c][k] = W_3[c][k] mask_2[b][k], packed [K / 16][RA][16] (RA = round32(B C); rows >= B C zero) for J = A W_2
// Two set-up chores of a solve ride in its first workgroups: zero[0 .. nzero) = 0.0 (the pair slots of T2h; NULL: not asked for) and
// cdst[0 .. ncopy) = csrc (r|b0 for iteration 0's closing launch; csrc NULL: not asked for; ncopy % 4 == 0, both 16-byte aligned)
int launch_headj_pack(const float* W3, const float* mask2, float* Ap, int B, int C, int K, int RA, double* zero, int nzero,
                      const float* csrc, float* cdst, int ncopy, hipStream_t st);

}  // namespace bhg
