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
  int tile_shape;                           // kHeadjTile, or the measurement build's debug key head_j_tile
  // ---- update blocks: a PstepArgs (mlp/pstep.inc), copied as bytes
  const void* ps; size_t ps_bytes; int nu;
};
constexpr int kHeadjTile = 1;               // 32 x 16 tiles (0: 32 x 32)
int headj_tiles(int rows, int K, int shape);   // workgroups (= T2h partials) of the tile class
int launch_headj(const HeadjLaunch& a, hipStream_t st);

// A[b C + c][k] = W_3[c][k] mask_2[b][k], packed [K / 16][RA][16] (RA = round32(B C); rows >= B C zero) for J = A W_2
int launch_headj_pack(const float* W3, const float* mask2, float* Ap, int B, int C, int K, int RA, hipStream_t st);

}  // namespace bhg
