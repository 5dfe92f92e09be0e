// bhg_cross_entropy.hip — the Hessian-vector product's share of F.cross_entropy, fused.
//
// Where it sits on the path: betty/hypergradient/cg.py:39-41 / neumann.py:62 take H p as the DOUBLE BACKWARD
// `torch.autograd.grad(in_grad, params, grad_outputs=p)`.  Every opaque inner problem ends in F.cross_entropy; under create_graph=True
// its first backward is nll_loss_backward followed by _log_softmax_backward_data, and ATen differentiates those two by a chain of
// element-wise and reduction operators over the whole [N, C] logit matrix.
//
// Per row i: lsm_i = log_softmax(z_i) (ATen's own output, what the forward saved), P = exp(lsm), target y_i,
// m_i = [y_i != ignore_index and 0 <= y_i < C].  The first backward is
//     F : (z, g) -> gz        gz_ic = g_i m_i (P_ic - [c = y_i])
// (g_i the gradient that reaches row i's loss: per row under "none", the scalar g under "sum", g / sum m under "mean") and one
// Hessian-vector product needs its VECTOR-JACOBIAN product: given the cotangent a of gz, with s_i = sum_c P_ic a_ic,
//     dz_ic = g_i m_i P_ic (a_ic - s_i)        dg_i = m_i (s_i - a_{i, y_i})
// and for a scalar g, dg = sum_i dg_i (divided by sum m under "mean").  y is not differentiable and dz has no one-hot term.  Float64
// restatement and its check against autograd: tests/cross_entropy_ref.py.  P = expf(lsm) in fp32; the row sum s_i and everything after
// it in fp64; no atomics: bitwise run-to-run deterministic, like the rest of the library.
//
// THREE regimes, chosen by ce_plan (closed form; the launch path and bhg_cross_entropy_plan call the same function):
//   short  C <= 1024 (16-byte accesses) resp. 256 (scalar): 256 / tpr rows side by side in a workgroup, tpr threads per row and two
//          vectors per thread (k_ce_vjp_rows<VEC, 2>).  The classifiers of the examples.
//   row    one row per workgroup, lsm and a held in registers between the s_i reduction and the dz write: 12 bytes per element (read
//          lsm, read a, write dz).  One instance of k_ce_vjp_rows per vectors-per-thread class, up to 128 elements per thread and
//          array: rows of at most 32768 elements (16-byte accesses) resp. 32 elements: 8192 (scalar accesses).
//   split  a row longer than that, or fewer than kCeSplitBelowRows = 160 rows of more than kCeSplitMinRow = 16384 elements (the row
//          workgroups would leave too many CUs idle): the row is cut into `slices` chunks of a multiple of 1024 elements;
//          k_ce_split_sums writes the per-slice fp64 partials of s_i, k_ce_split_out adds them in slice order and writes dz and dg.
//          20 bytes per element.  The vocabulary regime.
// In short / row a workgroup walks a contiguous run of row groups and the grid is capped at what is resident at once (256 CUs times the
// workgroups a CU holds at the instance's register count).  Per-row g: ONE launch.  Scalar g with dg wanted: the workgroups' fp64 sums
// of dg_i go to the workspace and k_ce_dg_combine adds them in workgroup order (short / row), resp. one more workgroup of
// k_ce_split_out adds the rows in a fixed order (split): two launches in every case.
//
// Registers on gfx950 (-Rpass-analysis=kernel-resource-usage; NO instance has a private segment: ScratchSize 0 everywhere), and the
// workgroups of 256 threads a CU holds at that count (512 registers per lane and SIMD, one wave of a workgroup per SIMD, at most 8):
//     k_ce_vjp_rows<4, 2>    68 VGPRs            7          k_ce_vjp_rows<1, 2>    52 VGPRs   8
//     k_ce_vjp_rows<4, 4>    77 VGPRs            6          k_ce_vjp_rows<1, 8>    78 VGPRs   6
//     k_ce_vjp_rows<4, 8>   128 VGPRs            4          k_ce_vjp_rows<1, 32>  236 VGPRs   2
//     k_ce_vjp_rows<4, 16>  232 VGPRs            2          k_ce_split_sums<4>     85 VGPRs   5       k_ce_split_sums<1>  38 VGPRs   8
//     k_ce_vjp_rows<4, 32>  256 VGPRs + 156 AGPRs 1         k_ce_split_out<4>      63 VGPRs   7 (*)   k_ce_split_out<1>   33 VGPRs   8
//     k_ce_dg_combine        14 VGPRs            8          (*) the compiler's occupancy figure, at 63 VGPRs and 102 SGPRs
// The split kernels' grid-stride cap is the tightest of their four figures: 256 CUs x 5 = 1280 workgroups (k_ce_split_sums<4> with
// its loop unrolled four times: four pairs of 16-byte loads in flight per thread).
// SGPR spills (to VGPR lanes, not to memory; the counts above include those VGPRs): k_ce_vjp_rows<4, 32> 51, <1, 32> 89, every other
// kernel 0.  No VGPR spills anywhere.
// P and a of 128 elements per thread are 256 registers: the <4, 32> instance runs one wave per SIMD, without a private segment.  A
// scalar instance of 128 elements (<1, 128>) was tried and spills (1196 bytes per lane): the scalar path ends at 32 elements per thread,
// rows of 8192 elements.  Without the register pin between the two passes (the asm statement after ce_row_sum) the compiler keeps the
// first pass's fp64 products: <4, 8> 200, <4, 16> 256 + 90 AGPRs, <4, 32> 644 bytes of scratch per lane.
//
// The plan's constants, measured on one MI355X (profiles/cross_entropy_double_backward.txt; stream-synchronised calls, per-row g):
//   * the register-resident bound, 8192 rows: 2.67 / 2.63 / 3.71 ns per 1000 elements at C = 8192 / 16384 / 32768 (instances 8 / 16 / 32:
//     0.56 / 0.57 / 0.40 of 8 TB/s on 12 bytes per element) against 3.90 for the split regime at C = 32772 (4.03 with its stride at 2048 workgroups) — one wave per SIMD costs the
//     128-element instance a third of its rate, and it is still ahead of two passes over the row: the bound stays at 32768;
//   * fewer rows than CUs, C = 32768 held in registers against C = 32772 split: 64 rows 37.2 | 32.3 us, 128 rows 42.7 | 38.9 us, 256 rows
//     44.3 | 52.4 us — the split wins by 3.8 us at 128 rows and loses by 8.1 us at 256; linear interpolation puts the crossover at 169
//     rows: kCeSplitBelowRows = 160, five eighths of the CUs (the arms tried were 64 and 256: at 256, 255 rows split took 52.1 us and
//     256 rows in registers 43.4 us); at 160: 159 rows split 42.3 us, 160 rows in registers 42.7 us.  Those three runs had the split
//     kernels' stride at 2048 workgroups; at 1280 the split is faster — 128 / 159 rows 36.8 / 41.0 us (8 slices) against 160 / 256 rows
//     in registers 43.2 / 44.3 us — and its 0.135 us per row extrapolates to the rows' 43.5 us at about 178 rows.  The constant stays at
//     160: rows 160 to about 177 run up to 5 % slower than a split would; the crossover has not been located again;
//   * the row length below which that split does not pay, 8 / 16 / 32 rows: C = 8192 in one launch 24.6 / 24.7 / 24.7 us against
//     C = 8196 split in two 29.0 / 29.1 / 29.2 us — a call of one launch costs 24.6 us and one of two 29 us on the host, and a CU
//     streams a 32768-element row in 12.6 us more (37.2 - 24.6), so the second launch is paid for from about 4.4 us of row, 11 000
//     elements.  That estimate is too low: with the constant at 16384, 8 / 64 / 128 rows of 16384 in one launch take 29.2 / 29.9 /
//     32.5 us and of 16388 split 30.1 / 30.9 / 33.6 us — just above the edge the split still LOSES by about 1 us (3 %), and at 64 rows of
//     32768 it wins (37.2 | 32.3): the crossover lies between 16384 and 32768 and has not been located more closely.  kCeSplitMinRow =
//     16384 is the kernel-instance edge (16 | 32 vectors per thread) inside that bracket, at a known cost of 3 % just above it (the
//     first arm tried was 8192, where the split lost by 18 %);
//   * kCeMinChunk = 1024 (one 16-byte vector per thread) and the 1280-workgroup stride of the split kernels (the table above) are
//     derived, not measured.
//
// A limit: with a scalar g and dg wanted in the split regime, ONE workgroup of k_ce_split_out adds all N rows (thread t the rows t,
// t + 256, ..., `slices` partials each).  That is N * slices / 256 dependent fp64 loads per thread on one CU: negligible beside the two
// passes for the shapes measured (N up to 8192: 32 rows per thread), a serial tail for N in the millions, where a tree over the rows
// would be needed.  With dz NULL as well the other workgroups have nothing to do.
//
// Layout: fp32, N contiguous rows of C.  C % 4 == 0: every access of lsm, a and dz is a 16-byte vector; otherwise scalar accesses.
#include "bhg_common.hpp"

namespace bhg {
namespace {

constexpr int kCeCUs = 256;              // MI355X
constexpr int kCeMaxC = 262144;          // the family
constexpr int kCeMaxRowVec = 32768;      // register-resident bound, 16-byte accesses: 128 elements per thread and array at 256 threads
constexpr int kCeMaxRowScalar = 8192;    // and scalar accesses: 32 elements (128 spill: the header of this file)
constexpr int kCeMinChunk = 1024;        // split regime: a slice is a multiple of one 16-byte vector per thread of the workgroup, which
                                         // keeps every slice 16-byte aligned; kCeMaxC / kCeMinChunk = 256 is the most slices a row can
                                         // have, and k_ce_split_out adds them with one thread per slice
constexpr int kCeSplitWgs = 1280;        // split regime: 256 CUs x 5 workgroups, what k_ce_split_sums<4> (85 VGPRs) holds: the header's table
constexpr int kCeSplitBelowRows = 160;   // fewer rows than this, of more than kCeSplitMinRow elements, are split: measured, see the header
constexpr int kCeSplitMinRow = 16384;    // a shorter row is never split for being one of few: measured, see the header of this file

enum { kCeShort = 0, kCeRow = 1, kCeSplit = 2 };

struct CeArgs {
  const float* lsm; const long long* y; const float* g; const float* denom; const float* a;
  float* dz; float* dg;                  // each may be NULL (not computed, not written)
  double* spart;                         // split: [N][slices] partials of s_i
  double* dgpart;                        // short / row with a scalar g: [wgs] partials of dg
  long long N, ignore_index;
  int C, scalar_g;
  int regime;
  int vec;                               // 4: 16-byte accesses (C % 4 == 0); 1: scalar
  int tpr, ltpr;                         // threads per row (a power of two <= 256) and its log2
  int rows;                              // 256 / tpr rows side by side: one row group
  int nv, inst;                          // vectors per thread, and of the kernel instance that runs (0: split)
  long long groups, gps;                 // short / row: row groups, and row groups per workgroup
  int wgs, max_wgs;                      // workgroups of the first launch, and their cap
  int slices, chunk;                     // split: workgroups per row and elements per slice
  long long items;                       // split: N * slices
};

template <int VEC>
__device__ __forceinline__ void ce_load(const float* __restrict__ p, float* v) {
  if (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = p[0];
  }
}
template <int VEC>
__device__ __forceinline__ void ce_store(float* __restrict__ p, const float* v) {
  if (VEC == 4)
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else
    p[0] = v[0];
}

// Whether target t names a class: an ignored row and a target outside [0, C) are the same to every kernel here.
__device__ __forceinline__ bool ce_valid(const long long t, const long long ignore_index, const int C) {
  return t != ignore_index && t >= 0 && t < (long long)C;
}

// The gradient that reaches every row's loss when g is one element: g, or g / denom.
__device__ __forceinline__ double ce_scalar_g(const CeArgs& q) {
  if (!q.scalar_g) return 0.0;
  const double g = (double)q.g[0];
  return q.denom ? g / (double)q.denom[0] : g;
}

// The sum over the tpr threads of a row, valid in every thread of the row.  tpr < 64: a butterfly inside the wave (both partners add
// the same two numbers, so the row's threads hold the same bits); tpr >= 64: the wave sum, then the row's waves in wave order.
// Contains barriers when tpr > 64: every thread of the workgroup calls it the same number of times.
__device__ __forceinline__ double ce_row_sum(double s, const int tpr, double* red) {
  if (tpr >= 64) {
    s = wave_sum(s);
  } else {
    for (int m = tpr >> 1; m > 0; m >>= 1) s += __shfl_xor(s, m);
  }
  if (tpr > 64) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();  // protect `red` against the previous row group
    if (lane == 0) red[wave] = s;
    __syncthreads();
    const int nw = tpr >> 6, w0 = (wave / nw) * nw;
    double t = 0.0;
    for (int j = 0; j < nw; ++j) t += red[w0 + j];
    s = t;
  }
  return s;
}

// grid = wgs.  Workgroup w walks the row groups [w * gps, min((w + 1) * gps, groups)); row group g is the rows g * rows + tr,
// tr = thread / tpr; thread tv = thread % tpr of a row owns the vectors tv, tv + tpr, ... (< NV of them) of every row it meets.
template <int VEC, int NV>
__global__ __launch_bounds__(kThreads) void k_ce_vjp_rows(CeArgs q) {
  constexpr int E = VEC * NV;
  __shared__ double red[kWaves];
  __shared__ double rowdg[NV == 2 ? kThreads : 1];   // rows side by side (tpr < 256) only occur with two vectors per thread
  const int tid = threadIdx.x, tpr = q.tpr, tv = tid & (tpr - 1), tr = tid >> q.ltpr;
  const int nvec = q.C / VEC;
  const bool want_dz = q.dz != nullptr, want_dg = q.dg != nullptr;
  const double gs = ce_scalar_g(q);
  double dgacc = 0.0;   // scalar g: this thread's rows' dg_i (threads tv == 0 only), in row order

  const long long g0 = (long long)blockIdx.x * q.gps;
  const long long g1 = g0 + q.gps < q.groups ? g0 + q.gps : q.groups;
  for (long long g = g0; g < g1; ++g) {
    const long long row = g * q.rows + tr;
    const bool live = row < q.N;
    const long long yy = live ? q.y[row] : q.ignore_index;
    const bool m = live && ce_valid(yy, q.ignore_index, q.C);
    // addresses: a workgroup-uniform 64-bit base (the row group) plus a 32-bit offset (< 256 * 128 elements) per thread and vector
    const long long gbase = g * q.rows * q.C;
    const float* __restrict__ lg = q.lsm + gbase;
    const float* __restrict__ ag = q.a + gbase;
    const unsigned rbase = (unsigned)(tr * q.C);
    float pv[E], av[E];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int v = tv + k * tpr;
#pragma unroll
      for (int u = 0; u < VEC; ++u) { pv[k * VEC + u] = 0.f; av[k * VEC + u] = 0.f; }
      if (m && v < nvec) {   // an ignored row reads neither lsm nor a
        const unsigned off = rbase + (unsigned)(v * VEC);
        ce_load<VEC>(lg + off, pv + k * VEC);
        ce_load<VEC>(ag + off, av + k * VEC);
      }
    }
    // elements outside the row (and ignored rows) were loaded as zeros of a: they add nothing to s, and are not stored
    double s = 0.0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      pv[e] = expf(pv[e]);   // P replaces lsm in the registers
      s += (double)pv[e] * (double)av[e];
    }
    s = ce_row_sum(s, tpr, red);
    // The row is held as fp32 P and a, nothing else: without this the compiler keeps the first pass's fp64 intermediates alive for
    // the second pass.  No instruction.
#pragma unroll
    for (int e = 0; e < E; ++e) asm volatile("" : "+v"(pv[e]), "+v"(av[e]));
    if (want_dz && live) {
      const double gi = q.scalar_g ? gs : (m ? (double)q.g[row] : 0.0);
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        float o[VEC];
#pragma unroll
        for (int u = 0; u < VEC; ++u) {
          const int e = k * VEC + u;
          o[u] = m ? (float)(gi * (double)pv[e] * ((double)av[e] - s)) : 0.f;
        }
        const int v = tv + k * tpr;
        if (v < nvec) ce_store<VEC>(q.dz + gbase + rbase + (unsigned)(v * VEC), o);
      }
    }
    if (want_dg && live && tv == 0) {
      const double dgi = m ? s - (double)q.a[row * q.C + yy] : 0.0;
      if (q.scalar_g) dgacc += dgi;
      else q.dg[row] = (float)dgi;
    }
  }

  if (!(q.scalar_g && want_dg)) return;   // uniform over the workgroup
  if (NV == 2 && q.rows > 1) {
    // rows side by side: the threads tv == 0 of the rows tr = 0 .. rows - 1 are added in tr order
    if (tv == 0) rowdg[tr] = dgacc;
    __syncthreads();
    if (tid == 0) {
      double t = 0.0;
      for (int j = 0; j < q.rows; ++j) t += rowdg[j];
      q.dgpart[blockIdx.x] = t;
    }
  } else if (tid == 0) {
    q.dgpart[blockIdx.x] = dgacc;
  }
}

// One workgroup.  The workgroups' partials of the scalar dg, added in a fixed order (thread t adds the partials t, t + 256, ...; then
// the block sum), divided by denom where one is given.
__global__ __launch_bounds__(kThreads) void k_ce_dg_combine(const double* __restrict__ part, const int n, const float* __restrict__ denom,
                                                            float* __restrict__ dg) {
  __shared__ double red[kWaves];
  double t = 0.0;
  for (int i = threadIdx.x; i < n; i += kThreads) t += part[i];
  t = block_sum(t, red);
  if (threadIdx.x == 0) dg[0] = (float)(denom ? t / (double)denom[0] : t);
}

// Split regime, launch 1.  Work item i = row * slices + slice is the elements [slice * chunk, min(C, (slice + 1) * chunk)) of a row;
// the workgroups stride over the items.  spart[i] = the item's share of s_row (0 for an ignored row, which reads neither lsm nor a).
template <int VEC>
__global__ __launch_bounds__(kThreads) void k_ce_split_sums(CeArgs q) {
  __shared__ double red[kWaves];
  const int tid = threadIdx.x;
  for (long long item = blockIdx.x; item < q.items; item += gridDim.x) {
    const long long row = item / q.slices;
    const int sl = (int)(item - row * q.slices);
    const int c0 = sl * q.chunk, c1 = c0 + q.chunk < q.C ? c0 + q.chunk : q.C;
    double s = 0.0;
    if (ce_valid(q.y[row], q.ignore_index, q.C)) {   // uniform over the workgroup
      const float* __restrict__ lr = q.lsm + row * q.C;
      const float* __restrict__ ar = q.a + row * q.C;
#pragma unroll 4
      for (int c = c0 + tid * VEC; c < c1; c += kThreads * VEC) {
        float pv[VEC], av[VEC];
        ce_load<VEC>(lr + c, pv);
        ce_load<VEC>(ar + c, av);
#pragma unroll
        for (int u = 0; u < VEC; ++u) s += (double)expf(pv[u]) * (double)av[u];
      }
    }
    s = block_sum(s, red);
    if (tid == 0) q.spart[item] = s;
  }
}

// Split regime, launch 2.  The same work items; s_row = the row's slices added in a fixed order (thread t holds slice t, slices <= 256;
// then the block sum: every workgroup of a row computes the same bits).  With a scalar g and dg wanted the grid has ONE more workgroup,
// the last, which adds the rows' dg_i: thread t the rows t, t + 256, ... in row order, then the block sum.
template <int VEC>
__global__ __launch_bounds__(kThreads) void k_ce_split_out(CeArgs q, const int work_wgs) {
  __shared__ double red[kWaves];
  const int tid = threadIdx.x;
  const bool want_dz = q.dz != nullptr, want_dg = q.dg != nullptr;
  if ((int)blockIdx.x == work_wgs) {   // only launched for a scalar g with dg wanted
    double t = 0.0;
    for (long long row = tid; row < q.N; row += kThreads) {
      const long long yy = q.y[row];
      if (!ce_valid(yy, q.ignore_index, q.C)) continue;
      double s = 0.0;
      for (int j = 0; j < q.slices; ++j) s += q.spart[row * q.slices + j];
      t += s - (double)q.a[row * q.C + yy];
    }
    t = block_sum(t, red);
    if (tid == 0) q.dg[0] = (float)(q.denom ? t / (double)q.denom[0] : t);
    return;
  }
  const double gs = ce_scalar_g(q);
  for (long long item = blockIdx.x; item < q.items; item += work_wgs) {
    const long long row = item / q.slices;
    const int sl = (int)(item - row * q.slices);
    const long long yy = q.y[row];
    const bool m = ce_valid(yy, q.ignore_index, q.C);   // uniform over the workgroup
    if (!want_dz && (sl != 0 || q.scalar_g)) continue;  // nothing to write for this item
    double s = 0.0;
    if (m) s = block_sum(tid < q.slices ? q.spart[row * q.slices + tid] : 0.0, red);
    if (want_dz) {
      const int c0 = sl * q.chunk, c1 = c0 + q.chunk < q.C ? c0 + q.chunk : q.C;
      float* __restrict__ zr = q.dz + row * q.C;
      if (m) {
        const double gi = q.scalar_g ? gs : (double)q.g[row];
        const float* __restrict__ lr = q.lsm + row * q.C;
        const float* __restrict__ ar = q.a + row * q.C;
#pragma unroll 4
        for (int c = c0 + tid * VEC; c < c1; c += kThreads * VEC) {
          float pv[VEC], av[VEC], o[VEC];
          ce_load<VEC>(lr + c, pv);
          ce_load<VEC>(ar + c, av);
#pragma unroll
          for (int u = 0; u < VEC; ++u) o[u] = (float)(gi * (double)expf(pv[u]) * ((double)av[u] - s));
          ce_store<VEC>(zr + c, o);
        }
      } else {
        float o[VEC];
#pragma unroll
        for (int u = 0; u < VEC; ++u) o[u] = 0.f;
        for (int c = c0 + tid * VEC; c < c1; c += kThreads * VEC) ce_store<VEC>(zr + c, o);
      }
    }
    if (want_dg && !q.scalar_g && sl == 0 && tid == 0) q.dg[row] = m ? (float)(s - (double)q.a[row * q.C + yy]) : 0.f;
  }
}

// Why the launch does not take a shape, or NULL where it does: bhg_cross_entropy_backward_vjp and bhg_cross_entropy_plan refuse the
// same shapes.
inline const char* ce_shape_error(long long N, int C) {
  if (!(N > 0 && C > 0)) return "empty tensor";
  if (C > kCeMaxC) return "more than 262144 classes";
  if (N > (1LL << 40)) return "more than 2^40 rows";   // keeps every 64-bit product below far from overflow
  return nullptr;
}

// Workgroups of k_ce_vjp_rows that are resident at once: the CUs times the workgroups a CU holds at the instance's register count (the
// table in the header of this file).
inline int ce_max_wgs(int vec, int inst) {
  const int per_cu = vec == 4 ? (inst == 2 ? 7 : inst == 4 ? 6 : inst == 8 ? 4 : inst == 16 ? 2 : 1) : (inst == 2 ? 8 : inst == 8 ? 6 : 2);
  return kCeCUs * per_cu;
}

// The geometry, in closed form (nothing is searched: tpr comes from a shift loop of at most 8 steps).
inline const char* ce_plan(CeArgs* q, long long N, int C, int scalar_g) {
  const char* bad = ce_shape_error(N, C);
  if (bad) return bad;
  q->N = N; q->C = C; q->scalar_g = scalar_g ? 1 : 0;
  q->vec = C % 4 == 0 ? 4 : 1;
  const int nvec = C / q->vec;
  // two vectors per thread until a row takes the whole workgroup: a narrow row leaves no thread idle (256 / tpr rows side by side)
  int tpr = 1, ltpr = 0;
  while (tpr < kThreads && 2 * tpr < nvec) { tpr <<= 1; ++ltpr; }
  q->tpr = tpr; q->ltpr = ltpr;
  q->rows = kThreads / tpr;
  q->nv = (nvec + tpr - 1) / tpr;
  q->slices = 1; q->chunk = C; q->items = 0;
  if (tpr < kThreads) q->regime = kCeShort;
  else if (C <= (q->vec == 4 ? kCeMaxRowVec : kCeMaxRowScalar) && (N >= kCeSplitBelowRows || C <= kCeSplitMinRow)) q->regime = kCeRow;
  else q->regime = kCeSplit;
  if (q->regime != kCeSplit) {
    // supported instance counts: 16-byte path 2, 4, 8, 16, 32 (C <= 32768: nv <= 32); scalar path 2, 8, 32 (C <= 8192: nv <= 32)
    if (q->vec == 4) q->inst = q->nv <= 2 ? 2 : q->nv <= 4 ? 4 : q->nv <= 8 ? 8 : q->nv <= 16 ? 16 : 32;
    else q->inst = q->nv <= 2 ? 2 : q->nv <= 8 ? 8 : 32;
    q->groups = (N + q->rows - 1) / q->rows;
    q->max_wgs = ce_max_wgs(q->vec, q->inst);
    const long long cap = q->max_wgs;
    const long long wgs = q->groups < cap ? q->groups : cap;
    q->gps = (q->groups + wgs - 1) / wgs;
    q->wgs = (int)((q->groups + q->gps - 1) / q->gps);   // <= cap, none empty
    return nullptr;
  }
  // split: as many slices as bring the N rows to kCeSplitWgs workgroups, of at least kCeMinChunk elements each
  q->tpr = kThreads; q->ltpr = 8; q->rows = 1; q->inst = 0; q->groups = N; q->gps = 1;
  long long want = (kCeSplitWgs + N - 1) / N;
  const long long most = (C + kCeMinChunk - 1) / kCeMinChunk;
  if (want > most) want = most;
  const int per = (int)((C + want - 1) / want);
  q->chunk = (per + kCeMinChunk - 1) / kCeMinChunk * kCeMinChunk;
  q->slices = (C + q->chunk - 1) / q->chunk;   // <= want <= 256, none empty
  q->nv = q->chunk / (kThreads * q->vec);
  q->items = N * q->slices;
  q->max_wgs = kCeSplitWgs;
  q->wgs = (int)(q->items < kCeSplitWgs ? q->items : kCeSplitWgs);
  return nullptr;
}

inline size_t ce_ws_spart(const CeArgs& q) { return q.regime == kCeSplit ? sizeof(double) * (size_t)q.items : 0; }
inline size_t ce_ws_dgpart(const CeArgs& q) { return q.regime != kCeSplit && q.scalar_g ? sizeof(double) * (size_t)q.wgs : 0; }
inline int ce_launches(const CeArgs& q) { return q.regime == kCeSplit || q.scalar_g ? 2 : 1; }

template <int VEC, int NV>
inline void ce_launch_rows(const CeArgs& q, hipStream_t st) {
  hipLaunchKernelGGL((k_ce_vjp_rows<VEC, NV>), dim3(q.wgs), dim3(kThreads), 0, st, q);
}

}  // namespace
}  // namespace bhg

using namespace bhg;

extern "C" {

size_t bhg_cross_entropy_ws_bytes(long long N, int C, int g_is_scalar) {
  CeArgs q{};
  return ce_plan(&q, N, C, g_is_scalar) ? 0 : ce_ws_spart(q) + ce_ws_dgpart(q);
}

int bhg_cross_entropy_plan(long long N, int C, int g_is_scalar, char* buf, size_t buf_bytes) {
  BHG_REQUIRE(buf && buf_bytes > 0, "NULL buffer");
  CeArgs q{};
  const char* bad = ce_plan(&q, N, C, g_is_scalar);
  BHG_REQUIRE(!bad, bad);
  const int len = snprintf(buf, buf_bytes, "regime=%s vec=%d tpr=%d rows=%d nv=%d inst=%d groups=%lld gps=%lld slices=%d chunk=%d wgs=%d max_wgs=%d launches=%d ws=%lld",
                           q.regime == kCeShort ? "short" : q.regime == kCeRow ? "row" : "split", q.vec, q.tpr, q.rows, q.nv, q.inst,
                           q.groups, q.gps, q.slices, q.chunk, q.wgs, q.max_wgs, ce_launches(q), (long long)(ce_ws_spart(q) + ce_ws_dgpart(q)));
  BHG_REQUIRE(len > 0 && (size_t)len < buf_bytes, "buffer too small for the plan line");
  return BHG_OK;
}

int bhg_cross_entropy_backward_vjp(const float* lsm, const long long* y, const float* g, int g_is_scalar, const float* denom,
                                   const float* a, long long N, int C, long long ignore_index, float* dz, float* dg, void* ws,
                                   size_t ws_bytes, void* stream) {
  CeArgs q{};
  const char* bad = ce_plan(&q, N, C, g_is_scalar);
  BHG_REQUIRE(!bad, bad);
  BHG_REQUIRE(lsm && y && g && a, "null pointer");
  BHG_REQUIRE(dz || dg, "both outputs are NULL");
  BHG_REQUIRE(!denom || q.scalar_g, "denom needs a scalar g");
  // the partials of the scalar dg are only written when dg is wanted
  const size_t need = ce_ws_spart(q) + (dg ? ce_ws_dgpart(q) : 0);
  if (need > 0) {
    BHG_REQUIRE(ws, "the call needs a workspace");
    BHG_REQUIRE(ws_bytes >= need, "workspace smaller than bhg_cross_entropy_ws_bytes(N, C, g_is_scalar)");
    BHG_REQUIRE(((uintptr_t)ws & 7) == 0, "the workspace must be 8-byte aligned");
  }
  if (q.vec == 4)
    for (const void* p : {(const void*)lsm, (const void*)a, (const void*)dz})
      BHG_REQUIRE(((uintptr_t)p & 15) == 0, "lsm, a and dz must be 16-byte aligned when C is a multiple of 4");
  q.lsm = lsm; q.y = y; q.g = g; q.denom = denom; q.a = a; q.dz = dz; q.dg = dg; q.ignore_index = ignore_index;
  q.spart = static_cast<double*>(ws);
  q.dgpart = static_cast<double*>(ws);   // short / row: there are no partials of s_i in front
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (q.regime == kCeSplit) {
    const int extra = q.scalar_g && dg ? 1 : 0;
    if (q.vec == 4) {
      hipLaunchKernelGGL(k_ce_split_sums<4>, dim3(q.wgs), dim3(kThreads), 0, st, q);
      hipLaunchKernelGGL(k_ce_split_out<4>, dim3(q.wgs + extra), dim3(kThreads), 0, st, q, q.wgs);
    } else {
      hipLaunchKernelGGL(k_ce_split_sums<1>, dim3(q.wgs), dim3(kThreads), 0, st, q);
      hipLaunchKernelGGL(k_ce_split_out<1>, dim3(q.wgs + extra), dim3(kThreads), 0, st, q, q.wgs);
    }
  } else {
    switch (q.vec * 1000 + q.inst) {
      case 4002: ce_launch_rows<4, 2>(q, st); break;
      case 4004: ce_launch_rows<4, 4>(q, st); break;
      case 4008: ce_launch_rows<4, 8>(q, st); break;
      case 4016: ce_launch_rows<4, 16>(q, st); break;
      case 4032: ce_launch_rows<4, 32>(q, st); break;
      case 1002: ce_launch_rows<1, 2>(q, st); break;
      case 1008: ce_launch_rows<1, 8>(q, st); break;
      default: ce_launch_rows<1, 32>(q, st); break;
    }
    if (q.scalar_g && dg) hipLaunchKernelGGL(k_ce_dg_combine, dim3(1), dim3(kThreads), 0, st, q.dgpart, q.wgs, denom, dg);
  }
  BHG_HIP_CHECK(hipGetLastError());
  return BHG_OK;
}

}  // extern "C"
