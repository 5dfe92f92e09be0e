// Fragment of bhg_mlp.hip — #included there INSIDE `namespace bhg { namespace {`, after wsk.inc.  Not a header of its own.
// Here: skinny GEMMs on PACKED operands (round 4) — the chain through the constant weights and the B x B Gram products of the
// projected solvers, several problems per launch.
//
// Why a packed layout.  v_mfma_f32_16x16x4_f32 wants lane (li = lane & 15, lk = lane >> 4) to hold A[li][k] for four k's.  From a
// row-major [rows][K] operand that is a 16-B load per lane whose 64 lanes touch 16 rows x 64 B — sixteen HALF cache lines per
// instruction (the direct form of wsk.inc: bound by the vector cache's address path), or a coalesced load that is then transposed
// through a wave-private LDS tile (the staged form: 8 ds_write_b128 + 8 ds_read_b128 per 32 MFMAs, 26 % of its LDS cycles bank
// conflicts, the two waves of a SIMD serialised behind their own LDS round trips — SQ counters of round 3: matrix pipe busy 31 %
// of the launch).  Both operands of these products are written by kernels of this library (the weights once per solve), so the
// producer lays them out for the consumer instead:
//
//     packed(X [R][K])  =  Xp [K / 16][R][16]              Xp[((k >> 4) * R + r) * 16 + (k & 15)] = X[r][k]
//
// One wave-wide 16-B load of (16 rows) x (16 k) is then ONE contiguous KiB — eight full 128-B lines — and lands in the MFMA
// register layout as it is: lane (li, lk) reads offset li * 16 + 4 * lk of the block and owns k = 16 * kb + 4 * lk + c in the c-th
// of four MFMAs.  No LDS in the K loop, no bank conflicts, no transposition; the K loop is loads and MFMAs only.
//
// One workgroup (4 waves) owns a 32 x 32 output tile (optionally one K split of it): the waves take disjoint K ranges, the four
// partial tiles meet in LDS in fixed order (deterministic), the epilogue of wsk.inc runs before anything leaves the chip — and
// the result is stored row-major for the element-wise consumers AND packed for the next product of the chain.
// FOUR waves per workgroup, one per SIMD (probe, scripts/probes/wskp_probe.hip on the MI355X, forward product through W_1 of cfg 2:
// loads alone 8.6 us, MFMAs alone 8.1 us; together 9.7 us with 4 waves x 3 register stages — but 14.5 us with 8 waves, two per
// SIMD: 48 outstanding 16-B loads per SIMD no longer overlap with the matrix pipe, 12.2 us at 32, and the workgroup's epilogue
// waits 4 us for the SIMD's second wave).
constexpr int kWskpWaves = 4;
constexpr int kWskpMax = 8;
struct WskpProb {
  const float* Ap;      // packed M-side operand [RA][K]
  const float* Bq;      // packed N-side operand [RB][K]   (RB = N: output columns)
  int RA, RB, K;        // K % 32 == 0, RA % 32 == 0, RB % 32 == 0
  int nsplit;           // K split over workgroups (>= 1); nsplit > 1 implies raw
  int raw;              // 1: raw sums to out + split * RA * RB (rows >= B zero): Gram slabs, the slabs the head kernel combines
  int B;                // valid rows
  const float* bias;    // [RB] or NULL
  const float* mask;    // [RA][RB] or NULL
  const float* addend;  // [RA][RB] or NULL: the direction's share G_l (hoisted chain), added before bias / mask
  const float* rh;      // [RA][RB]: T2 partner of the addend (needs partT2) or NULL
  float* out;           // row-major [RA][RB] (raw: slabs)
  float* outp;          // packed copy of out, [RB / 16][RA][16], or NULL
  double* partT2;       // one partial per tile or NULL
  int nfull, nstrip;    // row tiling, filled in by wskp_tiling(): 32-row tiles, then 16 x 64 tiles over a remainder of <= 16 rows
  int pairs;            // measurement build only (key xcd_pairs): 0 = column tiles of a 64-column strip on two XCDs (the form before round 5)
  // k_wskpl only (the chain's first product by linearity, see there): product' = product + beta * zold, stored at znew (the host
  // product; a Gram rider stores it as its output); addend' = addend + beta * addend2; bias' = bias + beta * bias2;
  // beta: polled from `gran` at the epilogue (NULL: beta = 0, first iteration)
  const float* zold; float* znew; const float* addend2; const float* bias2; const unsigned long long* gran;
};
struct WskpArgs {
  WskpProb p[kWskpMax];
  int blk0[kWskpMax + 1];   // first block of every problem (multiples of 8: block -> XCD affinity survives the grouping)
  int n;
#ifdef BHG_WSKP_STAMPS      // scripts/probes only: four s_memrealtime stamps per workgroup (entry, K loop, K loop end, exit)
  unsigned long long* stamps;
#endif
};
#ifdef BHG_WSKP_STAMPS
#define BHG_WSKP_STAMP(slot) do { if (g.stamps && threadIdx.x == 0) g.stamps[4 * blockIdx.x + (slot)] = wall_clock64(); } while (0)
#else
#define BHG_WSKP_STAMP(slot) do { } while (0)
#endif
static_assert(sizeof(WskpArgs) <= 3800, "kernel arguments of k_wskp must fit the kernarg segment");

// K loop of one wave: (16 RBLK) x (16 CBLK) outputs, `nch` chunks of 32 k.  gA / gB: this lane's element of the first k-block of
// the wave's range (block 0 of the tile); sA / sB: floats per k-block (16 * R).
// (Measured, not kept: reading the granule beta is published in ONCE inside this loop, three quarters in, so that the tile epilogue's
//  poll costs no round trip — loads return in order, the agent-scope load is a round trip to the memory side and every operand load
//  behind it waits: k_wskpl 17.2 us instead of 16.4.)
template <int D, int RBLK, int CBLK>
__device__ __forceinline__ void wskp_loop(const float* __restrict__ gA, const float* __restrict__ gB, const int64_t sA,
                                          const int64_t sB, const int nch, f32x4 (&acc)[RBLK][CBLK]) {
  f32x4 sa[D][RBLK][2];   // [stage][row block][k-block of the chunk]
  f32x4 sb[D][CBLK][2];
  auto load = [&](const int d, int ch) {
    ch = min(ch, nch - 1);   // past the end: re-load the last chunk (never used), keeps the loop free of control flow
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float* pa = gA + (int64_t)(2 * ch + h) * sA;
      const float* pb = gB + (int64_t)(2 * ch + h) * sB;
#pragma unroll
      for (int rb = 0; rb < RBLK; ++rb) sa[d][rb][h] = *reinterpret_cast<const f32x4*>(pa + rb * 256);
#pragma unroll
      for (int cb = 0; cb < CBLK; ++cb) sb[d][cb][h] = *reinterpret_cast<const f32x4*>(pb + cb * 256);
    }
  };
  auto compute = [&](const int d) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int rb = 0; rb < RBLK; ++rb)
#pragma unroll
          for (int cb = 0; cb < CBLK; ++cb)
            acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(sa[d][rb][h][c], sb[d][cb][h][c], acc[rb][cb], 0, 0, 0);
      }
    }
  };
#pragma unroll
  for (int d = 0; d < D; ++d) {
    load(d, d);
    __builtin_amdgcn_sched_barrier(0);   // stage order = issue order (the waits count loads issued AFTER the needed ones)
  }
  int s = 0;
  for (; s + 2 * D <= nch; s += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      compute(d);
      __builtin_amdgcn_sched_barrier(0);
      load(d, s + D + d);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {
    if (s + d < nch) compute(d);
    if (s + D + d < nch) load(d, s + D + d);
  }
  s += D;
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (s + d < nch) compute(d);
}

// One tile of (16 RBLK) rows x (16 CBLK) columns at (m0, n0), K split `sp` of q.nsplit; t2_slot: where its T2 partial goes.
// zero_rows: this tile also clears rows [m0 + 16 RBLK, RA) of its columns (nobody else writes them; every consumer reads RA rows).
constexpr int kWskpLds = kWskpWaves * 32 * kWskPad;   // floats: four partial tiles, 32 x 33 or 16 x 65
// beta published by another workgroup of the SAME launch (k_wskpl's update blocks): 64 replicated {1 : float bits} granules, one
// per 64-byte line, written with agent-scope exchanges and polled with relaxed agent-scope loads — no fence; the poller only
// needs the scalar itself.  The granules are cleared by the launch before (k_graw).
// BOUNDED (round 5; ADVICE r4): the publisher is a workgroup of the same launch, and nothing but dispatch order guarantees that it
// runs — a host-side mistake that leaves it out (round 4 lost its last GPU minutes to exactly that) must not hang the GPU.  After
// kBetaSpinLimit polls (~1 s; the published value normally sits there at the FIRST load) the poller raises the solver's time-out word
// — the second 8-byte word of granule 0's line, never touched by publisher or clearer; bhg_mlp_timeout_flag_dev() — and returns NaN:
// the solve runs to its end with a poisoned result, the host reads the cause (HipBackend.check_health).
constexpr unsigned kBetaSpinLimit = 1u << 20;
__device__ __forceinline__ float poll_beta(const unsigned long long* gran) {
  const unsigned long long* p = gran + 8 * (blockIdx.x & 63);
  unsigned long long v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  unsigned spins = 0;
  while ((v >> 32) == 0ull) {
    __builtin_amdgcn_s_sleep(1);
    if (++spins > kBetaSpinLimit) {
      __hip_atomic_store(reinterpret_cast<unsigned*>(const_cast<unsigned long long*>(gran) + 1), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return __builtin_nanf("");
    }
    v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return __builtin_bit_cast(float, (unsigned)(v & 0xffffffffull));
}
// DOTS (round 6, the factor-exchange solver's G(raw) launch: k_wskpd): the tile also emits three fp64 partials — <X, Gr>, <X, Gp>, <X, out>
// over its 32 x 32 outputs (rows < B) — into part[slot], part[nd + slot], part[2 nd + slot]: this rank's shares of r.raw, p.raw, raw.raw
// (X = the inner products' partner: Rd_l forward, Rh_{l-1} backward).  The operands are requested with the other epilogue operands, before
// the K loop.  `red` must hold 3 * kWskpWaves doubles then.
struct WskpDots { const float* X; const float* Gr; const float* Gp; double* part; int slot0, nd; };
template <int D, int RBLK, int CBLK, class G, bool LIN = false, bool RELU = false, bool DOTS = false>
__device__ __forceinline__ void wskp_tile(const WskpProb& q, const int m0, const int n0, const int sp, const int t2_slot,
                                          const bool zero_rows, float* __restrict__ sPf, double* __restrict__ red, const G& g,
                                          const WskpDots* __restrict__ dots = nullptr, const int dot_slot = 0) {
  constexpr int TR = 16 * RBLK, TC = 16 * CBLK, TCP = TC + 1;
  static_assert(TR * TC == 1024 && kWskpWaves * TR * TCP <= kWskpLds, "tile shapes: 32 x 32 or 16 x 64");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, lk = lane >> 4;
  // K chunks (32 k each) of this workgroup's split, then of this wave: even shares, the first waves take the remainder
  const int nct = q.K / 32;
  const int cb0 = (int)(((int64_t)sp * nct) / q.nsplit), ce = (int)(((int64_t)(sp + 1) * nct) / q.nsplit);
  const int c0 = cb0 + (int)(((int64_t)wave * (ce - cb0)) / kWskpWaves), c1 = cb0 + (int)(((int64_t)(wave + 1) * (ce - cb0)) / kWskpWaves);
  const int nch_w = c1 - c0;
  f32x4 acc[RBLK][CBLK];
#pragma unroll
  for (int a = 0; a < RBLK; ++a)
#pragma unroll
    for (int b = 0; b < CBLK; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[a][b][r] = 0.f;
  // epilogue operands of this thread's outputs: requested before the K loop, they land under it
  constexpr int kOutPer = 1024 / (64 * kWskpWaves);
  float e_mask[kOutPer], e_rh[kOutPer], e_bias[kOutPer], e_add[kOutPer];
  float e_zold[LIN ? kOutPer : 1], e_add2[LIN ? kOutPer : 1], e_bias2[LIN ? kOutPer : 1];
  float e_x[DOTS ? kOutPer : 1], e_gr[DOTS ? kOutPer : 1], e_gp[DOTS ? kOutPer : 1];
#pragma unroll
  for (int u = 0; u < kOutPer; ++u) {
    const int e = threadIdx.x + 64 * kWskpWaves * u;
    const int64_t idx = (int64_t)(m0 + e / TC) * q.RB + n0 + (e % TC);
    if (DOTS) { e_x[u] = dots->X[idx]; e_gr[u] = dots->Gr[idx]; e_gp[u] = dots->Gp[idx]; }
    // (unconditional loads — an absent operand reads element 0 of the packed A operand and is discarded: behind a run-time `if`
    //  hipcc waits for each load at the end of its block, a round trip to the Infinity Cache per optional operand before the
    //  first load of the K loop goes out; probe: 0.8 us of prologue with three operands, 1.9 us with four)
    const float vm = (q.mask ? q.mask : q.Ap)[q.mask ? idx : 0];
    const float vr = (q.partT2 ? q.rh : q.Ap)[q.partT2 ? idx : 0];
    const float vb = (q.bias ? q.bias : q.Ap)[q.bias ? n0 + (e % TC) : 0];
    const float va = (q.addend ? q.addend : q.Ap)[q.addend ? idx : 0];
    e_mask[u] = q.mask ? vm : 1.f;
    e_rh[u] = q.partT2 ? vr : 0.f;
    e_bias[u] = q.bias ? vb : 0.f;
    e_add[u] = q.addend ? va : 0.f;
    if (LIN) {
      const float vz = (q.zold ? q.zold : q.Ap)[q.zold ? idx : 0];
      const float va2 = (q.addend2 ? q.addend2 : q.Ap)[q.addend2 ? idx : 0];
      const float vb2 = (q.bias2 ? q.bias2 : q.Ap)[q.bias2 ? n0 + (e % TC) : 0];
      e_zold[u] = q.zold ? vz : 0.f;
      e_add2[u] = q.addend2 ? va2 : 0.f;
      e_bias2[u] = q.bias2 ? vb2 : 0.f;
    }
  }
  BHG_WSKP_STAMP(1);
  if (LIN) { BHG_STAMP(2, 0); }
  if (nch_w > 0) {   // (wave-uniform)
    const int64_t sA = (int64_t)16 * q.RA, sB = (int64_t)16 * q.RB;
    const float* gA = q.Ap + (int64_t)(2 * c0) * sA + (m0 + li) * 16 + 4 * lk;
    const float* gB = q.Bq + (int64_t)(2 * c0) * sB + (n0 + li) * 16 + 4 * lk;
    wskp_loop<D, RBLK, CBLK>(gA, gB, sA, sB, nch_w, acc);
  }
  BHG_WSKP_STAMP(2);
  if (LIN) { BHG_STAMP(2, 1); }
  // C/D layout of v_mfma_f32_16x16x4_f32: col = lane & 15, row = 4 * (lane >> 4) + reg
  float* sW = sPf + wave * (TR * TCP);
#pragma unroll
  for (int rb = 0; rb < RBLK; ++rb)
#pragma unroll
    for (int cbk = 0; cbk < CBLK; ++cbk)
#pragma unroll
      for (int r = 0; r < 4; ++r) sW[(16 * rb + 4 * lk + r) * TCP + 16 * cbk + li] = acc[rb][cbk][r];
  __syncthreads();
  float beta_lin = 0.f;
  if (LIN) { BHG_STAMP(2, 2); }
  if (LIN && q.gran) beta_lin = poll_beta(q.gran);
  if (LIN) { BHG_STAMP(2, 3); }
  double t2 = 0.0;
  double dr = 0.0, dp = 0.0, dw = 0.0;
  float* outb = q.out + (q.raw ? (int64_t)sp * q.RA * q.RB : 0);
  float* outpb = q.outp ? q.outp + (q.raw ? (int64_t)sp * q.RA * q.RB : 0) : nullptr;   // (Gram slabs: also packed, for k_graw)
#pragma unroll
  for (int u = 0; u < kOutPer; ++u) {
    const int e = threadIdx.x + 64 * kWskpWaves * u;
    const int row = e / TC, col = e % TC;
    const int m = m0 + row, n = n0 + col;
    const int64_t idx = (int64_t)m * q.RB + n;
    float v = e_add[u];   // (0 without an addend)
    if (LIN) {   // by linearity in the direction p' = r' + beta p: product(p') = product(r') + beta product(p), and so on
      float sum = 0.f;
#pragma unroll
      for (int w = 0; w < kWskpWaves; ++w) sum += sPf[w * (TR * TCP) + row * TCP + col];
      const float z = add_rn(sum, mul_rn(beta_lin, e_zold[u]));
      if (q.znew) q.znew[idx] = m < q.B ? z : 0.f;
      v = add_rn(v, mul_rn(beta_lin, e_add2[u]));   // the rounding of the recurrence G(p') = G(r') + beta G(p)
      v += z;
      if (!q.raw) {
        if (q.bias) v += add_rn(e_bias[u], mul_rn(beta_lin, e_bias2[u]));
        if (q.mask) v *= e_mask[u];
      }
    } else {
    if (q.partT2 && m < q.B) t2 += (double)v * (double)e_rh[u];
#pragma unroll
    for (int w = 0; w < kWskpWaves; ++w) v += sPf[w * (TR * TCP) + row * TCP + col];
    if (!q.raw) {
      if (q.bias) v += e_bias[u];
      if (q.mask) v *= e_mask[u];
    }
    if constexpr (RELU) {   // forward pass of the net itself (k_wskpf): out = relu(.), the 0 / 1 mask beside it (k_reduce_mask's rule)
      g.relu_mask[idx] = (m < q.B && v > 0.f) ? 1.f : 0.f;
      v = v > 0.f ? v : 0.f;
    }
    }
    v = m < q.B ? v : 0.f;
    outb[idx] = v;
    if (outpb) outpb[((int64_t)(n >> 4) * q.RA + m) * 16 + (n & 15)] = v;
    if (DOTS && m < q.B) { dr += (double)e_x[u] * (double)e_gr[u]; dp += (double)e_x[u] * (double)e_gp[u]; dw += (double)e_x[u] * (double)v; }
  }
  if (DOTS) {   // (workgroup-uniform; fixed order: lanes by DPP, then the four waves)
    dr = wave_sum(dr); dp = wave_sum(dp); dw = wave_sum(dw);
    if (lane == 0) { red[wave] = dr; red[kWskpWaves + wave] = dp; red[2 * kWskpWaves + wave] = dw; }
    __syncthreads();
    if (threadIdx.x == 0) {
      double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
      for (int w = 0; w < kWskpWaves; ++w) { s0 += red[w]; s1 += red[kWskpWaves + w]; s2 += red[2 * kWskpWaves + w]; }
      dots->part[dot_slot] = s0; dots->part[dots->nd + dot_slot] = s1; dots->part[2 * dots->nd + dot_slot] = s2;
    }
  }
  if (zero_rows) {   // (workgroup-uniform) the padding rows below this tile
    const int rows = q.RA - (m0 + TR);
    for (int e = threadIdx.x; e < rows * TC; e += 64 * kWskpWaves) {
      const int m = m0 + TR + e / TC, n = n0 + e % TC;
      outb[(int64_t)m * q.RB + n] = 0.f;
      if constexpr (RELU) g.relu_mask[(int64_t)m * q.RB + n] = 0.f;
      if (outpb) outpb[((int64_t)(n >> 4) * q.RA + m) * 16 + (n & 15)] = 0.f;
    }
  }
  if (q.partT2) {
    t2 = wave_sum(t2);
    if (lane == 0) red[wave] = t2;
    __syncthreads();
    if (threadIdx.x == 0) {
      double s = 0.0;
#pragma unroll
      for (int w = 0; w < kWskpWaves; ++w) s += red[w];
      q.partT2[t2_slot] = 2.0 * s;
      // the alpha launch sums every slot of the layer: the slots no tile of this (ragged) tiling owns are cleared by the tiles
      const int used = q.nfull * (q.RB / 32) + q.nstrip, slots = (q.RA / 32) * (q.RB / 32);
      for (int z = t2_slot + used; z < slots; z += used) q.partT2[z] = 0.0;
    }
  }
  BHG_WSKP_STAMP(3);
  if (LIN) { BHG_STAMP(2, 4); }
}

// One workgroup: block t of problem q.  Row tiling of a problem (host: wskp_tiling): q.nfull row tiles of 32 rows cover the valid
// rows in 32 x 32 tiles; a remainder of at most 16 valid rows is covered by q.nstrip tiles of 16 rows x 64 columns instead of a
// fourth, mostly empty row of 32 x 32 tiles (B = 100: 3 x 64 + 32 workgroups instead of 4 x 64 for the product through W_1^T — the
// 32 CUs that frees run the Gram product riding in the same launch).  K-split / raw problems keep every row tile (nfull = RA / 32).
template <int D, class G, bool LIN = false, bool RELU = false, bool DOTS = false>
__device__ __forceinline__ void wskp_body(const WskpProb& q, const int t, float* __restrict__ sPf, double* __restrict__ red, const G& g,
                                          const WskpDots* __restrict__ dots = nullptr) {
  const int ntn = q.RB / 32;
  const int full = q.nfull * ntn;
  if (t >= (full + q.nstrip) * q.nsplit) return;   // padding block (block tables are rounded up to multiples of 8)
  if (t >= full && q.nstrip > 0 && q.nsplit == 1) {
    const int ts = t - full;
    wskp_tile<D, 1, 4, G, LIN, RELU>(q, 32 * q.nfull, 64 * ts, 0, t, 32 * q.nfull + 16 < q.RA, sPf, red, g);
    return;
  }
  const int tile = t % full, sp = t / full;
  // Workgroup ids go round-robin over the 8 XCDs: all row tiles of a column tile sit on ONE XCD (the streamed weight-side operand
  // is fetched into one L2), consecutive column tiles on different XCDs.
  // With strip tiles (16 x 64 over the last rows: block full + ts covers column tiles 2 ts and 2 ts + 1 and sits on XCD ts % 8) the
  // column tiles go to the XCDs in PAIRS, pair ts on XCD ts % 8: the strip finds its 64 columns of the weight in the L2 its 32 x 32
  // neighbours fetched them into instead of fetching the whole weight a second time through the fabric (round 5: FETCH_SIZE of
  // the product through W_1 40.1 -> see profiles/r05_pmc_traffic.json).  The T2 partial keeps the slot of the un-paired order, so
  // the consumer's fixed-order sum adds the same numbers in the same order.
  int tm, tn, slot = tile;
  if ((ntn & 7) == 0) {
    const int xcd = tile & 7, j = tile >> 3, c = j / q.nfull;
    tm = j % q.nfull;
    tn = c * 8 + xcd;
    bool paired = q.nstrip > 0 && (ntn & 15) == 0;
#ifdef BHG_AB
    paired = paired && q.pairs != 0;
#endif
    if (paired) {
      tn = 2 * ((c >> 1) * 8 + xcd) + (c & 1);
      slot = ((tn >> 3) * q.nfull + tm) * 8 + (tn & 7);
    }
  } else {
    tm = tile % q.nfull;
    tn = tile / q.nfull;
  }
  const bool zero_rows = q.nstrip == 0 && tm == q.nfull - 1 && 32 * q.nfull < q.RA;
  wskp_tile<D, 2, 2, G, LIN, RELU, DOTS>(q, tm * 32, tn * 32, sp, slot, zero_rows, sPf, red, g, dots, DOTS ? dots->slot0 + t : 0);
}
// Any number of problems: the descriptor is picked from the kernel arguments by a run-time index — a chain of dependent scalar
// loads (block table, then the descriptor: five round trips, 1.1 - 2.2 us before the first operand load goes out; probe
// scripts/probes/chain_probe.hip).  Used once per solve (the S_l / D_l Gram products of the first iteration) and for deep nets.
template <int D>
__global__ __launch_bounds__(64 * kWskpWaves) void k_wskp(WskpArgs g) {
  const int blk = blockIdx.x;
  BHG_WSKP_STAMP(0);
  int i = 0;
  while (i + 1 < g.n && blk >= g.blk0[i + 1]) ++i;
  const WskpProb q = g.p[i];
  __shared__ float sPf[kWskpLds];
  __shared__ double red[kWskpWaves];
  wskp_body<D>(q, blk - g.blk0[i], sPf, red, g);
}
// The factor-exchange solver's G(raw) launch (round 6): k_wskp whose tiles also emit the inner products' partials (WskpDots).
struct WskpdArgs { WskpArgs g; WskpDots d[kWskpMax]; };
static_assert(sizeof(WskpdArgs) <= 3800, "kernel arguments of k_wskpd must fit the kernarg segment");
template <int D>
__global__ __launch_bounds__(64 * kWskpWaves) void k_wskpd(WskpdArgs a) {
  const int blk = blockIdx.x;
  kernarg_warm<sizeof(WskpdArgs)>();
  int i = 0;
  while (i + 1 < a.g.n && blk >= a.g.blk0[i + 1]) ++i;
  const WskpProb q = a.g.p[i];
  const WskpDots dd = a.d[i];
  __shared__ float sPf[kWskpLds];
  __shared__ double red[3 * kWskpWaves];
  wskp_body<D, WskpArgs, false, false, true>(q, blk - a.g.blk0[i], sPf, red, a.g, &dd);
}
// The per-iteration launches: a chain product and at most TWO Gram products riding with it (B x B, one K slab each, the same K
// as their host so that they end with its tiles).  Every descriptor is a named kernel argument — no run-time index into the
// argument struct — and every field is "used" right after the selects: left alone hipcc sinks each group of scalar loads to the
// branch that needs it, a chain of dependent round trips (0.8 us before the first operand load, 1.9 us with the T2 operands;
// probe) instead of one.
struct GramRider { const float* Ap; const float* Bq; float* out; float* outp; int K, pad_; };
struct WskpcArgs {
  WskpProb a;
  GramRider r0, r1;
  int na, nr0;               // blocks of a (a multiple of 8), of rider 0 (a multiple of 8); the rest of the grid is rider 1's
#ifdef BHG_WSKP_STAMPS
  unsigned long long* stamps;
#endif
};
// (Measured, not kept: fetching the whole argument struct with four s_load_dwordx16 pinned by an in/out asm — the 64 pinned SGPRs
//  push the K loop's address arithmetic onto the VALU: K loop of the forward product through W_1 11.1 us instead of 9.0 us.)
template <int D>
__global__ __launch_bounds__(64 * kWskpWaves) void k_wskpc(WskpcArgs g) {
  const int blk = blockIdx.x;
  BHG_WSKP_STAMP(0);
  const bool fa = blk < g.na;
  const bool f0 = blk < g.na + g.nr0;
  WskpProb q;
  q.Ap = fa ? g.a.Ap : (f0 ? g.r0.Ap : g.r1.Ap);
  q.Bq = fa ? g.a.Bq : (f0 ? g.r0.Bq : g.r1.Bq);
  q.out = fa ? g.a.out : (f0 ? g.r0.out : g.r1.out);
  q.outp = fa ? g.a.outp : (f0 ? g.r0.outp : g.r1.outp);
  q.K = fa ? g.a.K : (f0 ? g.r0.K : g.r1.K);
  q.RA = g.a.RA; q.RB = fa ? g.a.RB : g.a.RA; q.B = g.a.B;
  q.nsplit = fa ? g.a.nsplit : 1; q.raw = fa ? g.a.raw : 1;
  q.bias = fa ? g.a.bias : nullptr; q.mask = fa ? g.a.mask : nullptr; q.addend = fa ? g.a.addend : nullptr;
  q.rh = fa ? g.a.rh : nullptr; q.partT2 = fa ? g.a.partT2 : nullptr;
  q.nfull = fa ? g.a.nfull : g.a.RA / 32; q.nstrip = fa ? g.a.nstrip : 0;
#ifdef BHG_AB
  q.pairs = g.a.pairs;
#endif
  asm volatile("" ::"s"(q.Ap), "s"(q.Bq), "s"(q.bias), "s"(q.mask), "s"(q.addend), "s"(q.rh), "s"(q.out), "s"(q.outp), "s"(q.partT2),
               "s"(q.RA), "s"(q.RB), "s"(q.K), "s"(q.nsplit), "s"(q.raw), "s"(q.B), "s"(q.nfull), "s"(q.nstrip));
  __shared__ float sPf[kWskpLds];
  __shared__ double red[kWskpWaves];
  wskp_body<D>(q, fa ? blk : (f0 ? blk - g.na : blk - g.na - g.nr0), sPf, red, g);
}

// Round 5: the net's own forward pass through a hidden layer on the packed operands (bhg_mlp_forward_packed): ONE product,
//   h_{l+1} = relu(h_l W_l^T + b_l)  row-major and packed for the next product,  mask_l = (pre-activation > 0)
// — the split-K GEMM + reduce pair of bhg_mlp_forward (15.4 + 4.6 us at cfg 2's second layer) as one launch of the chain's own form.
struct WskpfArgs { WskpProb a; float* relu_mask; };
template <int D>
__global__ __launch_bounds__(64 * kWskpWaves) void k_wskpf(WskpfArgs g) {
  const WskpProb q = g.a;
  __shared__ float sPf[kWskpLds];
  __shared__ double red[kWskpWaves];
  wskp_body<D, WskpfArgs, false, true>(q, blockIdx.x, sPf, red, g);
}

// ---- packing (once per solve: the weights are constants of a solve, h_l and delta_l of a step) ------------------------------------
// kind 0: X [R][K], K contiguous (a forward-chain weight W_l [d_{l+1}][d_l], an activation [Bp][d])  ->  packed [K/16][R][16]
// kind 1: X [Kr][R], R contiguous: the operand is X^T (the backward chain reads W_l as [k = d_{l+1}][n = d_l]) -> packed [Kr/16][R][16]
struct PackProb { const float* X; float* Xp; int R, K, kind; };
constexpr int kPackMax = 26;   // L <= 8 (the deepest hoistable net): 7 + 3 * 6
struct PackArgs { PackProb p[kPackMax]; int blk0[kPackMax + 1]; int n; };
static_assert(sizeof(PackArgs) <= 3800, "kernel arguments of k_pack must fit the kernarg segment");
inline int pack_blocks(const PackProb& q) { return (int)(((int64_t)q.R * q.K / 4 + 255) / 256); }
__global__ __launch_bounds__(256) void k_pack(PackArgs g) {
  const int blk = blockIdx.x;
  int i = 0;
  while (i + 1 < g.n && blk >= g.blk0[i + 1]) ++i;
  const PackProb q = g.p[i];
  const int64_t idx = (int64_t)(blk - g.blk0[i]) * 256 + threadIdx.x;   // one float4 of the OUTPUT per thread
  const int64_t total = (int64_t)q.R * q.K / 4;
  if (idx >= total) return;
  // output float4 idx: k-block kb, row r, quarter c4 (k = 16 kb + 4 c4 .. + 3)
  const int c4 = (int)(idx & 3);
  const int64_t rr = idx >> 2;
  const int r = (int)(rr % q.R), kb = (int)(rr / q.R);
  const int k = 16 * kb + 4 * c4;
  f32x4 v;
  if (q.kind == 0) {
    v = *reinterpret_cast<const f32x4*>(q.X + (int64_t)r * q.K + k);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = q.X[(int64_t)(k + j) * q.R + r];
  }
  *reinterpret_cast<f32x4*>(q.Xp + idx * 4) = v;
}
