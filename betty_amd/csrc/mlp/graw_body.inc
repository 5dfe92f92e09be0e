// Body of k_graw / k_graw64 — #included by graw.inc once per column tile width (BHG_GRAW_CT, BHG_GRAW_NAME, BHG_GRAW_WAVES_PER_EU).
// Text, not a function: the kernel arguments must be used inside the __global__ function itself — behind a reference parameter
// hipcc keeps a copy of the argument struct in scratch memory (1.9 KB per thread, check_spills.py).
template <int SMODE>   // FUSE_CG: inner products + CG epilogue of the small slices | FUSE_NEUMANN
__global__ __launch_bounds__(64 * kGrawWaves) __attribute__((amdgpu_waves_per_eu(BHG_GRAW_WAVES_PER_EU, BHG_GRAW_WAVES_PER_EU)))
void BHG_GRAW_NAME(GrawArgs g) {
  // B tiles of both operand pairs, [2][128][CT + 8] floats (40 KiB / 72 KiB); the partial tiles alias them after the MFMAs
  __shared__ __attribute__((aligned(16))) float sBf[2 * 128 * (BHG_GRAW_CT + 8)];
  const int blk = blockIdx.x;
  BHG_STAMP(0, 0);
  if (blk >= g.small0 && blk < g.small0 + g.small_blocks) {   // the small slices' outputs (head weight, biases) with their epilogue
    const int sb = blk - g.small0;
    float* smem = sBf;
    // the step length is computed INSIDE the body (every block the same partials, the same order, the same bits): requested before
    // the body's first operand load, summed after its last
    if (g.gran && sb == 0 && threadIdx.x < 64) g.gran[8 * threadIdx.x] = 0ull;   // (published anew by the next launch)
    GrawAlphaHere ah; ah.a = g.alpha; ah.do_alpha = g.do_alpha; ah.sb = sb;
    // (the one-burst forms of the small blocks hold a thread's <= 32 batch rows in registers: padded batch 128 only)
    constexpr bool kOne = BHG_GRAW_KLOOP == 0;
    if (sb < g.so.head_blocks) {
      if (g.so.head_has_rh) head_outer_body<true, SMODE, GrawAlphaHere, kOne>(g.so.head, g.so.hf, sb % g.so.head_gx, sb / g.so.head_gx, g.so.head_gx, smem, ah);
      else head_outer_body<false, SMODE, GrawAlphaHere, kOne>(g.so.head, g.so.hf, sb % g.so.head_gx, sb / g.so.head_gx, g.so.head_gx, smem, ah);
    } else {
      bias_body<SMODE, BiasArgsC, GrawAlphaHere, kOne>(g.so.ba, g.so.bf, sb - g.so.head_blocks, smem, ah);
    }
    BHG_STAMP(0, 4);
    return;
  }
  if (blk < g.blk0[0] || blk >= g.tile_end) return;   // (padding)
#if BHG_GRAW_KLOOP
  {
    // ---- round 5: K-LOOPED form — padded batch Bp a multiple of 128 larger than 128.  K = Bp is walked in chunks of 128: per chunk the
    // wave's Gram rows go into registers and both pairs' [128][CT] tiles through LDS exactly as in the one-chunk form below; the output
    // tile, its epilogue (inner products, residual step / Neumann update, Rh_0 emission) and the partials are the same.  Bp / 64 row
    // groups per column tile (blocks t, t + 8, ... of one column tile on one XCD); the emission's column sums are carried across the
    // chunks in bias_body's order (rows grp, grp + 4, ...: even trips into one sum, odd trips into the other).  No software pipeline
    // across chunks: it is the form for batches the 128-row instance cannot take, not the benchmark's.
    constexpr int CT = BHG_GRAW_CT;
    constexpr int NCB = CT / 16, TPR = CT / 4, RP = 256 / TPR, BPASS = 128 / RP, EPASS = 64 / RP, BPAD = CT + 8, PPAD = CT + 1;
    using fvec = __attribute__((ext_vector_type(NCB))) float;
    const int NG = g.Bp / 64, KC = g.Bp / 128;
    int i = 0;
#pragma unroll
    for (int j = 1; j < kHoistMax + 1; ++j) i += (j < g.n && blk >= g.blk0[j]) ? 1 : 0;
    const GrawProb q = g.p[i];
    const int t = blk - g.blk0[i];
    const int rg = (t >> 3) % NG, tn = (t / (8 * NG)) * 8 + (t & 7);
    if (tn * CT >= q.N) return;                 // (padding block)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int li = lane & 15, lk = lane >> 4;
    const int rt = wave & 1, sub = wave >> 1;
    const int m0 = rg * 64 + rt * 32, n0 = tn * CT;
    const bool two = q.A2 != nullptr;
    const float* A = (two && sub) ? q.A2 : q.A1;
    AlphaPendingT<1, 2> ap;
    if (SMODE == FUSE_CG && g.rnew) alpha_begin(g.alpha, false, ap);
    const int c0 = two ? 0 : 2 * sub, nch = two ? 4 : 2;
    const int tr = threadIdx.x / TPR, c4 = 4 * (threadIdx.x % TPR);
    f32x4 e_x[EPASS], e_r[EPASS], e_p[EPASS];
    if (SMODE == FUSE_CG || g.rnew) {
#pragma unroll
      for (int j = 0; j < EPASS; ++j) {
        const int64_t idx = (int64_t)(rg * 64 + tr + RP * j) * q.N + n0 + c4;
        e_r[j] = *reinterpret_cast<const f32x4*>(q.Gr + idx);
        e_p[j] = SMODE == FUSE_CG ? *reinterpret_cast<const f32x4*>(q.Gp + idx) : e_r[j];
      }
    }
    const bool em = g.rnew && g.rh0p != nullptr && i == g.rh0_prod;
    __shared__ float sCol[4 * BHG_GRAW_CT];
    float cs0 = 0.f, cs1 = 0.f;   // (em, threads < 4 CT) running column sums of Rd_0 over the chunks
    f32x4 acc[2][NCB];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < NCB; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[a][b][r] = 0.f;
    const int64_t sAk = (int64_t)16 * g.Bp;   // floats per k-block of a packed Gram matrix [Bp / 16][Bp][16]
    for (int kc = 0; kc < KC; ++kc) {
      f32x4 sa[4][2][2];
      {
        const float* gA = A + (int64_t)(8 * kc + 2 * c0) * sAk + (m0 + li) * 16 + 4 * lk;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int cc = c < nch ? c : nch - 1;
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) sa[c][rb][h] = *reinterpret_cast<const f32x4*>(gA + (int64_t)(2 * cc + h) * sAk + rb * 256);
        }
      }
      f32x4 rb4[2][BPASS];
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const float* Bm = (p && two) ? q.B2 : q.B1;
#pragma unroll
        for (int j = 0; j < BPASS; ++j) rb4[p][j] = *reinterpret_cast<const f32x4*>(Bm + (int64_t)(128 * kc + tr + RP * j) * q.N + n0 + c4);
      }
      if (kc > 0) __syncthreads();   // every wave is done with the previous chunk's B tiles
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int j = 0; j < BPASS; ++j) *reinterpret_cast<f32x4*>(sBf + ((p * 128) + tr + RP * j) * BPAD + c4) = rb4[p][j];
      __syncthreads();
      if (em && threadIdx.x < 4 * CT) {
        const int col = threadIdx.x % CT, grp = threadIdx.x / CT;
#pragma unroll
        for (int j = 0; j < 32; j += 2) {
          cs0 += sBf[(grp + 4 * j) * BPAD + col];
          cs1 += sBf[(grp + 4 * (j + 1)) * BPAD + col];
        }
      }
      if (SMODE == FUSE_CG && kc == (rg >> 1)) {   // (workgroup-uniform) the inner products' partner: this tile's own rows, staged now
#pragma unroll
        for (int j = 0; j < EPASS; ++j)
          e_x[j] = *reinterpret_cast<const f32x4*>(sBf + (((q.dots == 2 ? 1 : 0) * 128) + (rg & 1) * 64 + tr + RP * j) * BPAD + c4);
      }
      {
        const float* bt = sBf + (((two && sub) ? 128 : 0) + 32 * c0 + 4 * lk) * BPAD + NCB * li;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (c < nch) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
              for (int cc = 0; cc < 4; ++cc) {
                const fvec b = *reinterpret_cast<const fvec*>(bt + (32 * c + 16 * h + cc) * BPAD);
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) {
                  acc[0][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(sa[c][0][h][cc], b[cb], acc[0][cb], 0, 0, 0);
                  acc[1][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(sa[c][1][h][cc], b[cb], acc[1][cb], 0, 0, 0);
                }
              }
            }
          }
        }
      }
    }
    if (em && threadIdx.x < 4 * CT) sCol[(threadIdx.x / CT) * CT + threadIdx.x % CT] = cs0 + cs1;
    __syncthreads();   // every wave is done with the B tiles: the partial tiles take their place
    float* sP = sBf;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) sP[(wave * 32 + 16 * rb + 4 * lk + r) * PPAD + NCB * li + cb] = acc[rb][cb][r];
    __syncthreads();
    f32x4 e_m0[EPASS], rb0v, pb0v;
    if (em) {
#pragma unroll
      for (int j = 0; j < EPASS; ++j) e_m0[j] = *reinterpret_cast<const f32x4*>(g.mask0 + (int64_t)(rg * 64 + tr + RP * j) * q.N + n0 + c4);
      rb0v = *reinterpret_cast<const f32x4*>(g.rb0 + n0 + c4);
      pb0v = *reinterpret_cast<const f32x4*>(g.pb0s + n0 + c4);
    }
    float alpha_t = g.nalpha;
    if (SMODE == FUSE_CG && g.rnew) alpha_t = alpha_finish(g.alpha, false, ap);
    const float shift_t = SMODE == FUSE_CG ? g.alpha.shift : g.nshift;
    double d0 = 0.0, d1 = 0.0, d2 = 0.0;
#pragma unroll
    for (int j = 0; j < EPASS; ++j) {
      const int rl = tr + RP * j;
      const int m = rg * 64 + rl;
      const float* p0 = sP + (((rl >> 5) * 32) + (rl & 31)) * PPAD + c4;
      const float* p1 = sP + (((2 + (rl >> 5)) * 32) + (rl & 31)) * PPAD + c4;
      f32x4 v;
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = p0[u] + p1[u];
      if (m >= g.B) v = f32x4{0.f, 0.f, 0.f, 0.f};
      if (g.rnew) {
        if (m < g.B) {
          f32x4 gr;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            float hv = v[u];
            if (shift_t != 0.f) hv = add_rn(hv, mul_rn(shift_t, e_p[j][u]));
            gr[u] = sub_rn(e_r[j][u], mul_rn(alpha_t, hv));
          }
          *reinterpret_cast<f32x4*>(const_cast<float*>(q.Gr) + (int64_t)m * q.N + n0 + c4) = gr;
          if (em) {
            f32x4 o;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int c = c4 + u;
              float hb = (sCol[c] + sCol[CT + c]) + (sCol[2 * CT + c] + sCol[3 * CT + c]);
              if (shift_t != 0.f) hb = add_rn(hb, mul_rn(shift_t, pb0v[u]));
              const float rbn = sub_rn(rb0v[u], mul_rn(alpha_t, hb));
              o[u] = (gr[u] + rbn) * e_m0[j][u];
            }
            *reinterpret_cast<f32x4*>(g.rh0p + ((int64_t)((n0 + c4) >> 4) * g.Bp + m) * 16 + ((n0 + c4) & 15)) = o;
            if (SMODE != FUSE_CG && g.rh0) *reinterpret_cast<f32x4*>(g.rh0 + (int64_t)m * q.N + n0 + c4) = o;
          }
        } else if (em) {
          *reinterpret_cast<f32x4*>(g.rh0p + ((int64_t)((n0 + c4) >> 4) * g.Bp + m) * 16 + ((n0 + c4) & 15)) = f32x4{0.f, 0.f, 0.f, 0.f};
          if (SMODE != FUSE_CG && g.rh0) *reinterpret_cast<f32x4*>(g.rh0 + (int64_t)m * q.N + n0 + c4) = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      } else {
        *reinterpret_cast<f32x4*>(q.Graw + (int64_t)m * q.N + n0 + c4) = v;
      }
      if (SMODE == FUSE_CG && q.dots && m < g.B) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          d0 += (double)e_x[j][u] * (double)e_r[j][u];
          d1 += (double)e_x[j][u] * (double)e_p[j][u];
          d2 += (double)e_x[j][u] * (double)v[u];
        }
      }
    }
    if (SMODE == FUSE_CG && q.dots) {
      __shared__ double red[3][kGrawWaves];
      const double w0 = wave_sum(d0), w1 = wave_sum(d1), w2 = wave_sum(d2);
      if (lane == 0) { red[0][wave] = w0; red[1][wave] = w1; red[2][wave] = w2; }
      __syncthreads();
      if (threadIdx.x == 0) {
        double t0 = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll
        for (int w = 0; w < kGrawWaves; ++w) { t0 += red[0][w]; t1 += red[1][w]; t2 += red[2][w]; }
        const int pb = q.pb0 + NG * tn + rg;
        g.part[pb] = t0; g.part[g.npart + pb] = t1; g.part[2 * (int64_t)g.npart + pb] = t2;
      }
    }
    return;
  }
#else
  constexpr int CT = BHG_GRAW_CT;
  constexpr int NCB = CT / 16;            // column blocks of a wave (2 or 4)
  constexpr int TPR = CT / 4;             // threads per row of a [rows][CT] tile (one float4 each)
  constexpr int RP = 256 / TPR;           // rows per pass of the workgroup
  constexpr int BPASS = 128 / RP, EPASS = 64 / RP;
  constexpr int BPAD = CT + 8;            // LDS row stride (floats) of a staged B tile
  constexpr int PPAD = CT + 1;            // ... of a partial tile
  using fvec = __attribute__((ext_vector_type(NCB))) float;
  // block -> product: the table is one 64-byte line of the kernel arguments; compares only, no further loads
  int i = 0;
#pragma unroll
  for (int j = 1; j < kHoistMax + 1; ++j) i += (j < g.n && blk >= g.blk0[j]) ? 1 : 0;
  const GrawProb q = g.p[i];
  const int t = blk - g.blk0[i];
  // Bp = 128: two 64-row groups per column tile.  Blocks t and t + 8 are the two groups of ONE column tile: they run on the same
  // XCD (workgroup ids go round-robin over the 8 XCDs; the block tables are multiples of 16), so the batch-sized tile they share is
  // fetched from the Infinity Cache once, not twice.
  const int rg = (t >> 3) & 1, tn = (t >> 4) * 8 + (t & 7);
  if (tn * CT >= q.N) return;                 // (padding block)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int rt = wave & 1, sub = wave >> 1;   // row tile of the 64 rows; operand pair (two pairs) or half of K (one pair)
  const int m0 = rg * 64 + rt * 32, n0 = tn * CT;
  const bool two = q.A2 != nullptr;
  const float* A = (two && sub) ? q.A2 : q.A1;
  // (rnew) the step length's partials are requested before the tile's operands: they are needed only in the epilogue
  AlphaPendingT<1, 2> ap;
  if (SMODE == FUSE_CG && g.rnew) alpha_begin(g.alpha, false, ap);
  const int c0 = two ? 0 : 2 * sub, nch = two ? 4 : 2;   // chunks of 32 k: the whole K of a pair, or one half of the single pair
  // ---- every global load of the workgroup, issued before the first wait ---------------------------------------------------------
  // A: lane (li, lk) of row block rb, k-block kb reads 16 B at ((kb * 128 + m0 + 16 rb + li) * 16 + 4 lk)
  f32x4 sa[4][2][2];   // [chunk][row block][k-block of the chunk]
  {
    const float* gA = A + (int64_t)(2 * c0) * (16 * 128) + (m0 + li) * 16 + 4 * lk;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int cc = c < nch ? c : nch - 1;   // (one pair: chunks 2, 3 re-read chunk 1 and are not used)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) sa[c][rb][h] = *reinterpret_cast<const f32x4*>(gA + (int64_t)(2 * cc + h) * (16 * 128) + rb * 256);
    }
  }
  // B: both pairs' [128 k][CT columns] tiles, thread (k = tid / TPR + RP j, 4 columns): full row segments
  const int tr = threadIdx.x / TPR, c4 = 4 * (threadIdx.x % TPR);
  f32x4 rb4[2][BPASS];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float* Bm = (p && two) ? q.B2 : q.B1;
#pragma unroll
    for (int j = 0; j < BPASS; ++j) rb4[p][j] = *reinterpret_cast<const f32x4*>(Bm + (int64_t)(tr + RP * j) * q.N + n0 + c4);
  }
  // the epilogue's operands: thread (row = tid / TPR + RP j of the 64, 4 columns)
  f32x4 e_x[EPASS], e_r[EPASS], e_p[EPASS];
  if (SMODE == FUSE_CG) {
#pragma unroll
    for (int j = 0; j < EPASS; ++j) {
      const int64_t idx = (int64_t)(rg * 64 + tr + RP * j) * q.N + n0 + c4;
      e_r[j] = *reinterpret_cast<const f32x4*>(q.Gr + idx);
      e_p[j] = *reinterpret_cast<const f32x4*>(q.Gp + idx);
    }
  } else if (g.rnew) {   // Neumann applying its own update: G(v) is both "residual" and "direction"
#pragma unroll
    for (int j = 0; j < EPASS; ++j) {
      const int64_t idx = (int64_t)(rg * 64 + tr + RP * j) * q.N + n0 + c4;
      e_r[j] = *reinterpret_cast<const f32x4*>(q.Gr + idx);
      e_p[j] = e_r[j];
    }
  }
  // (Rh_0(r') emission, product rh0_prod only — workgroup-uniform)
  const bool em = g.rnew && g.rh0p != nullptr && i == g.rh0_prod;
  BHG_STAMP(0, 1);
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int j = 0; j < BPASS; ++j) *reinterpret_cast<f32x4*>(sBf + ((p * 128) + tr + RP * j) * BPAD + c4) = rb4[p][j];
  __syncthreads();
  __shared__ float sCol[4 * BHG_GRAW_CT];
  if (em && threadIdx.x < 4 * CT) {   // column sums of the staged Rd_0 tile, bias_body's order: 4 row groups, even / odd trips
    const int col = threadIdx.x % CT, grp = threadIdx.x / CT;
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int j = 0; j < 32; j += 2) {
      s0 += sBf[(grp + 4 * j) * BPAD + col];
      s1 += sBf[(grp + 4 * (j + 1)) * BPAD + col];
    }
    sCol[grp * CT + col] = s0 + s1;   // (rows >= B of Rd_0 are zero: adding them changes nothing)
  }
  if (SMODE == FUSE_CG) {   // the inner products' partner X is one of the staged operands (Rd_l = B1 forward, Rh_{l-1} = B2 backward)
#pragma unroll
    for (int j = 0; j < EPASS; ++j)
      e_x[j] = *reinterpret_cast<const f32x4*>(sBf + (((q.dots == 2 ? 1 : 0) * 128) + rg * 64 + tr + RP * j) * BPAD + c4);
  }
  f32x4 acc[2][NCB];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < NCB; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[a][b][r] = 0.f;
  {
    // B fragment: row k = 32 c + 16 h + 4 lk + cc, columns NCB li .. NCB li + NCB - 1 — component t belongs to column block t
    const float* bt = sBf + (((two && sub) ? 128 : 0) + 32 * c0 + 4 * lk) * BPAD + NCB * li;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c < nch) {   // (wave-uniform)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
          for (int cc = 0; cc < 4; ++cc) {
            const fvec b = *reinterpret_cast<const fvec*>(bt + (32 * c + 16 * h + cc) * BPAD);
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
              acc[0][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(sa[c][0][h][cc], b[cb], acc[0][cb], 0, 0, 0);
              acc[1][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(sa[c][1][h][cc], b[cb], acc[1][cb], 0, 0, 0);
            }
          }
        }
      }
    }
  }
  BHG_STAMP(0, 2);
  __syncthreads();   // every wave is done with the B tiles: the partial tiles take their place
  float* sP = sBf;   // [wave][32][PPAD]
  // C/D layout of v_mfma_f32_16x16x4_f32: col = lane & 15, row = 4 * (lane >> 4) + reg; column block cb holds columns NCB li + cb
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) sP[(wave * 32 + 16 * rb + 4 * lk + r) * PPAD + NCB * li + cb] = acc[rb][cb][r];
  __syncthreads();
  // the emission's operands, requested HERE by the emitting tiles only (one operand pair: they end 2 us before the others; as
  // stand-in loads of every tile before the MFMAs they cost the launch 1.3 us — timeline of round 4)
  f32x4 e_m0[EPASS], rb0v, pb0v;
  if (em) {
#pragma unroll
    for (int j = 0; j < EPASS; ++j) e_m0[j] = *reinterpret_cast<const f32x4*>(g.mask0 + (int64_t)(rg * 64 + tr + RP * j) * q.N + n0 + c4);
    rb0v = *reinterpret_cast<const f32x4*>(g.rb0 + n0 + c4);
    pb0v = *reinterpret_cast<const f32x4*>(g.pb0s + n0 + c4);
  }
  float alpha_t = g.nalpha;
  if (SMODE == FUSE_CG && g.rnew) alpha_t = alpha_finish(g.alpha, false, ap);   // (workgroup-uniform; the same bits in every block)
  const float shift_t = SMODE == FUSE_CG ? g.alpha.shift : g.nshift;
  double d0 = 0.0, d1 = 0.0, d2 = 0.0;
#pragma unroll
  for (int j = 0; j < EPASS; ++j) {   // row rl of the 64: waves (rl >> 5) and 2 + (rl >> 5) hold the two shares
    const int rl = tr + RP * j;
    const int m = rg * 64 + rl;
    const float* p0 = sP + (((rl >> 5) * 32) + (rl & 31)) * PPAD + c4;
    const float* p1 = sP + (((2 + (rl >> 5)) * 32) + (rl & 31)) * PPAD + c4;
    f32x4 v;
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = p0[u] + p1[u];
    if (m >= g.B) v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (g.rnew) {
      if (m < g.B) {   // the rounding sequence of proj_update_one: Hp = raw + shift p; r' = r - alpha Hp
        f32x4 gr;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          float hv = v[u];
          if (shift_t != 0.f) hv = add_rn(hv, mul_rn(shift_t, e_p[j][u]));
          gr[u] = sub_rn(e_r[j][u], mul_rn(alpha_t, hv));
        }
        *reinterpret_cast<f32x4*>(const_cast<float*>(q.Gr) + (int64_t)m * q.N + n0 + c4) = gr;
        if (em) {
          f32x4 o;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int c = c4 + u;
            float hb = (sCol[c] + sCol[CT + c]) + (sCol[2 * CT + c] + sCol[3 * CT + c]);
            if (shift_t != 0.f) hb = add_rn(hb, mul_rn(shift_t, pb0v[u]));
            const float rbn = sub_rn(rb0v[u], mul_rn(alpha_t, hb));
            o[u] = (gr[u] + rbn) * e_m0[j][u];
          }
          *reinterpret_cast<f32x4*>(g.rh0p + ((int64_t)((n0 + c4) >> 4) * g.Bp + m) * 16 + ((n0 + c4) & 15)) = o;
          if (SMODE != FUSE_CG && g.rh0) *reinterpret_cast<f32x4*>(g.rh0 + (int64_t)m * q.N + n0 + c4) = o;
        }
      } else if (em) {   // padding rows of the packed operand: zero (they meet delta's zero rows in the Gram products)
        *reinterpret_cast<f32x4*>(g.rh0p + ((int64_t)((n0 + c4) >> 4) * g.Bp + m) * 16 + ((n0 + c4) & 15)) = f32x4{0.f, 0.f, 0.f, 0.f};
        if (SMODE != FUSE_CG && g.rh0) *reinterpret_cast<f32x4*>(g.rh0 + (int64_t)m * q.N + n0 + c4) = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    } else {
      *reinterpret_cast<f32x4*>(q.Graw + (int64_t)m * q.N + n0 + c4) = v;
    }
    if (SMODE == FUSE_CG && q.dots && m < g.B) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        d0 += (double)e_x[j][u] * (double)e_r[j][u];
        d1 += (double)e_x[j][u] * (double)e_p[j][u];
        d2 += (double)e_x[j][u] * (double)v[u];
      }
    }
  }
  BHG_STAMP(0, 3);
  if (SMODE == FUSE_CG && q.dots) {   // (workgroup-uniform)
    __shared__ double red[3][kGrawWaves];
    const double w0 = wave_sum(d0), w1 = wave_sum(d1), w2 = wave_sum(d2);
    if (lane == 0) { red[0][wave] = w0; red[1][wave] = w1; red[2][wave] = w2; }
    __syncthreads();
    if (threadIdx.x == 0) {
      double t0 = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll
      for (int w = 0; w < kGrawWaves; ++w) { t0 += red[0][w]; t1 += red[1][w]; t2 += red[2][w]; }
      const int pb = q.pb0 + 2 * tn + rg;
      g.part[pb] = t0; g.part[g.npart + pb] = t1; g.part[2 * (int64_t)g.npart + pb] = t2;
    }
  }
  BHG_STAMP(0, 4);
#endif   // BHG_GRAW_KLOOP
}
