// bhg_mlp_tail.hpp — what bhg_mlp.hip and bhg_mlp_tail.hip share: the launch that ends the LAST iteration of a fused CG solve without
// a solution vector.  The device code lives in bhg_mlp_tail.hip, a translation unit of its own (the placement of the K-loop kernels
// inside bhg_mlp.o is pinned, see tests/test_code_placement.py); bhg_mlp.hip only fills this struct and calls the launcher.
//
// The identity.  p.Hp = sum_b T1[b] + sum T2h + sum_l T2_l + shift p.p with T2_l = 2 <Gb_l(p), Rh_{l-1}(p)>: the step
// length needs the R-forward chain and the hoisted direction products Gb_l(p), not the R-backward products Rd_{l-1} — whose tile
// epilogues merely carry the T2_l partials.  Where nothing reads Rd_{l-1} (the last iteration: r', p' and x are dead) the backward
// launches reduce to these dot products.
#pragma once
#include "bhg_common.hpp"

namespace bhg {

struct T2DotsLaunch {
  int n;                                    // problems (layers), 1 .. BHG_MLP_MAX_LAYERS
  const float* gb[BHG_MLP_MAX_LAYERS];      // Gb_l(p)     [RA][RB] row-major
  const float* rh[BHG_MLP_MAX_LAYERS];      // Rh_{l-1}(p) [RA][RB] row-major
  int RA[BHG_MLP_MAX_LAYERS], RB[BHG_MLP_MAX_LAYERS];   // padded rows, width: multiples of 32
  int t2_off[BHG_MLP_MAX_LAYERS];           // first slot of the layer in partT2; it owns (RA / 32) (RB / 32) slots from there
  int B;                                    // valid rows: rows >= B are never read
  double* partT2;
};
constexpr int kT2DotsMaxWgs = 256;          // the most workgroups of the launch (one per CU)
// partT2[t2_off[i] + j] = 2 x the j-th workgroup's fp64 share of sum_{m < B, n} gb[i][m][n] rh[i][m][n]; the layer's other slots 0.0
int launch_t2_dots(const T2DotsLaunch& a, hipStream_t st);

}  // namespace bhg
