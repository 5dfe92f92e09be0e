// Body of k_head_forward / k_headu — #included by head.inc and headu.inc INSIDE the kernel function (text, not a function: the kernel
// arguments must be named in the __global__ function itself).  Expects the parameter names of k_head_forward in scope, and
//   BHG_HEAD_B      this workgroup's sample row            BHG_HEAD_ROWS   rows of the launch (the padded batch)
//   BHG_HEAD_LAZY   1: `lazy_addend2` / `lazy_beta` in scope — the hoisted addend is Gf(r') + beta Gf(p) formed here (k_headu)
//   BHG_HEAD_J      defined (k_headj, bhg_mlp_headj.hip): the pre-head product reaches the classes through J_b — `hj_J`, `hj_Rh1`, `hj_K1`
//                   in scope; no slabs are combined, Rh_{L-2} is neither formed nor stored here (the launch's tiles do that)
  // rd_prev_p != NULL: a packed copy of rd_prev ([K / 16][rows][16], wskp.inc) for the first product of the backward chain
#if !BHG_HEAD_LAZY
  kernarg_warm<256>();   // (28 arguments: fetched in one round trip instead of group by group)
#endif
  extern __shared__ __attribute__((aligned(16))) float srow[];   // FUSED: the row of Rh_{L-2}, K floats
  // partT1 / partT2h != NULL (HEAD_JVP, fused CG solver): this sample row's share of p.Hp (see k_cg_alpha):
  //   partT1[b]  = sum_c Rz[b][c] * Rd_L[b][c]                          (the Gauss-Newton part)
  //   partT2h[b] = 2 * sum_k (delta_L V_L)[b][k] * Rh_{L-2}[b][k]       (the head layer's second-order part)
  __shared__ float t1s[kSmallC];
  __shared__ double red_t[kWaves];
  // HEAD_JVP with rd_prev != NULL also performs the R-backward step through the head for this sample row
  // (it only needs the row's own Rd_L):  rd_prev[b][k] = mask_prev[b][k] * sum_c (delta_top[b][c] V[c][k] + Rd_L[b][c] W[c][k])
  // mode HEAD_JVP:    rd[b][:] = sd[b] * (p*Rz - p (p.Rz))                     (one HVP's top of the network)
  // mode HEAD_COEFF:  aux[b]   = (p - onehot(y)).Rz / B                         (mixed-derivative coefficient)
  // mode HEAD_LOGITS: rd[b][:] = softmax(z), aux[b] = -log softmax(z)[y]        (forward pass; V = W, cb = bias)
  __shared__ float rz[kSmallC], rdl[kSmallC], dtl[kSmallC], pz[kSmallC];
  const int b = BHG_HEAD_B;
  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  if (b >= B) {
    if (mode != HEAD_COEFF && t < C) rd[(int64_t)b * C + t] = 0.f;
    if (mode != HEAD_JVP && t == 0) aux[b] = 0.f;
    if (mode == HEAD_JVP && rd_prev)
      for (int k = 4 * t; k < K; k += 1024) {
        *reinterpret_cast<float4*>(rd_prev + (int64_t)b * K + k) = make_float4(0.f, 0.f, 0.f, 0.f);
        if (rd_prev_p) *reinterpret_cast<float4*>(rd_prev_p + ((int64_t)(k >> 4) * BHG_HEAD_ROWS + b) * 16 + (k & 15)) = make_float4(0.f, 0.f, 0.f, 0.f);
      }
#ifndef BHG_HEAD_J
    if (FUSED)
      for (int k = 4 * t; k < K; k += 1024) *reinterpret_cast<float4*>(fz.rh_out + (int64_t)b * K + k) = make_float4(0.f, 0.f, 0.f, 0.f);
#endif
    return;
  }
  const float* hb = h + (int64_t)b * K;
  float acc[JMAX], cbv[JMAX];
  const float* vrow[JMAX];
  const float* wrow[JMAX];
#pragma unroll
  for (int j = 0; j < JMAX; ++j) {
    const int cc = min(wave + 4 * j, C - 1);
    acc[j] = 0.f;
    vrow[j] = V + (int64_t)cc * K;
    wrow[j] = W + (int64_t)cc * K;
    cbv[j] = cb[cc];
  }
  // PF: operands of the dot products (k = 4 lane and 4 lane + 256; clamped, not guarded) and the softmax inputs
  float4 pf_h[2], pf_v[2][JMAX], pf_w[2][JMAX];
  float pf_p = 0.f, pf_sd = 0.f, pf_dt = 0.f;
  if (PF) {
#pragma unroll
    for (int tr = 0; tr < 2; ++tr) {
      const int k = 4 * lane + 256 * tr;
      const int kc = k < K ? k : 0;
      pf_h[tr] = ld16(hb + kc);
#pragma unroll
      for (int j = 0; j < JMAX; ++j) {
        pf_v[tr][j] = ld16(vrow[j] + kc);
        pf_w[tr][j] = ld16(wrow[j] + kc);
      }
    }
    const int tc = t < C ? t : C - 1;
    pf_p = prob[(int64_t)b * C + tc];
    pf_sd = sd[b];
    pf_dt = delta_top[(int64_t)b * C + tc];
  }
#ifdef BHG_HEAD_J
  // J_b[c] . Rh_1[b] over K1 = d_{L-2}: lanes stride the rows like the dot products below, HJT trips of 256 k in flight; the first
  // batch is requested here, with the operands above
  constexpr int HJT = 3;
  const float* hj_rrow = hj_Rh1 + (int64_t)b * hj_K1;
  const float* hj_jrow[JMAX];
#pragma unroll
  for (int j = 0; j < JMAX; ++j) hj_jrow[j] = hj_J + ((int64_t)b * C + min(wave + 4 * j, C - 1)) * hj_K1;
  float4 hj_r[HJT], hj_j[HJT][JMAX];
#pragma unroll
  for (int tr = 0; tr < HJT; ++tr) {
    const int k = 4 * lane + 256 * tr;
    const int kc = k < hj_K1 ? k : 0;
    hj_r[tr] = ld16(hj_rrow + kc);
#pragma unroll
    for (int j = 0; j < JMAX; ++j) hj_j[tr][j] = ld16(hj_jrow[j] + kc);
  }
#endif
  if (FUSED) {
    for (int k = 4 * t; k < K; k += 1024) {
#ifndef BHG_HEAD_J
      const float* p0 = fz.part + (int64_t)b * K + k;
#endif
      const float4 bv = ld16(fz.bias + k);
      const float4 mv = ld16(fz.mask + (int64_t)b * K + k);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#ifndef BHG_HEAD_J
      constexpr int NB = PF ? 16 : 8;                 // slabs in flight together; the summation order is s = 0, 1, ... either way
      for (int s0 = 0; s0 < fz.splits; s0 += NB) {    // (as k_reduce_mask)
        float4 tt[NB];
#pragma unroll
        for (int u = 0; u < NB; ++u) tt[u] = ld16(p0 + (int64_t)(s0 + u < fz.splits ? s0 + u : fz.splits - 1) * fz.slab);
#pragma unroll
        for (int u = 0; u < NB; ++u)
          if (s0 + u < fz.splits) { v.x += tt[u].x; v.y += tt[u].y; v.z += tt[u].z; v.w += tt[u].w; }
      }
#endif
      if (fz.addend) {
        float4 ad = ld16(fz.addend + (int64_t)b * K + k);
#if BHG_HEAD_LAZY
        // the direction's share formed HERE: Gf(p') = Gf(r') + beta Gf(p) — the very rounding of the update blocks (proj_update_one),
        // which run as another block class of this launch and write Gf(p') into the OTHER slot (k_headu)
        if (lazy_addend2) {
          const float4 a2 = ld16(lazy_addend2 + (int64_t)b * K + k);
          ad.x = add_rn(ad.x, mul_rn(lazy_beta, a2.x)); ad.y = add_rn(ad.y, mul_rn(lazy_beta, a2.y));
          ad.z = add_rn(ad.z, mul_rn(lazy_beta, a2.z)); ad.w = add_rn(ad.w, mul_rn(lazy_beta, a2.w));
        }
#endif
        v.x += ad.x; v.y += ad.y; v.z += ad.z; v.w += ad.w;
      }
      v.x = (v.x + bv.x) * mv.x; v.y = (v.y + bv.y) * mv.y; v.z = (v.z + bv.z) * mv.z; v.w = (v.w + bv.w) * mv.w;
      *reinterpret_cast<float4*>(srow + k) = v;
#ifndef BHG_HEAD_J
      *reinterpret_cast<float4*>(fz.rh_out + (int64_t)b * K + k) = v;
#endif
    }
    __syncthreads();
  }
#ifdef BHG_HEAD_J
  // (srow holds mask (addend + c) — the part of Rh_{L-2} that does not come through W_{L-2}; the rest of it reaches rz through J)
  for (int k0 = 0; k0 < hj_K1; k0 += 256 * HJT) {
    if (k0 > 0) {
#pragma unroll
      for (int tr = 0; tr < HJT; ++tr) {
        const int k = k0 + 4 * lane + 256 * tr;
        const int kc = k < hj_K1 ? k : 0;
        hj_r[tr] = ld16(hj_rrow + kc);
#pragma unroll
        for (int j = 0; j < JMAX; ++j) hj_j[tr][j] = ld16(hj_jrow[j] + kc);
      }
    }
#pragma unroll
    for (int tr = 0; tr < HJT; ++tr) {
      if (k0 + 4 * lane + 256 * tr < hj_K1) {
        const float4 rv = hj_r[tr];
#pragma unroll
        for (int j = 0; j < JMAX; ++j) {
          float a = acc[j];
          const float4 jv = hj_j[tr][j];
          a = fmaf(rv.x, jv.x, a); a = fmaf(rv.y, jv.y, a); a = fmaf(rv.z, jv.z, a); a = fmaf(rv.w, jv.w, a);
          acc[j] = a;
        }
      }
    }
  }
#endif
  const float* rhb = HAS_RH ? (FUSED ? srow : Rh + (int64_t)b * K) : nullptr;
  // PF: operands of the fused R-backward (k = 4 t, all C <= 12 classes), requested while the dot products run
  float4 pf_mk, pf_W[12], pf_V[12];
  if (PF) {
    const int kd = 4 * t < K ? 4 * t : 0;
    pf_mk = ld16(mask_prev + (int64_t)b * K + kd);
#pragma unroll
    for (int c = 0; c < 12; ++c) {
      const int cc = min(c, C - 1);
      pf_W[c] = ld16(W + (int64_t)cc * K + kd);
      pf_V[c] = ld16(V + (int64_t)cc * K + kd);
    }
#pragma unroll
    for (int tr = 0; tr < 2; ++tr) {
      const int k = 4 * lane + 256 * tr;
      if (k < K) {
        const float4 hv = pf_h[tr];
        float4 rv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (HAS_RH) rv = *reinterpret_cast<const float4*>(rhb + k);
#pragma unroll
        for (int j = 0; j < JMAX; ++j) {
          float a = acc[j];
          const float4 vv = pf_v[tr][j], ww = pf_w[tr][j];
          a = fmaf(hv.x, vv.x, a); a = fmaf(hv.y, vv.y, a); a = fmaf(hv.z, vv.z, a); a = fmaf(hv.w, vv.w, a);
          if (HAS_RH) {
            a = fmaf(rv.x, ww.x, a); a = fmaf(rv.y, ww.y, a); a = fmaf(rv.z, ww.z, a); a = fmaf(rv.w, ww.w, a);
          }
          acc[j] = a;
        }
      }
    }
  }
  for (int k = 4 * lane; k < (PF ? 0 : K); k += 256) {
    const float4 hv = *reinterpret_cast<const float4*>(hb + k);
    float4 rv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (HAS_RH) rv = *reinterpret_cast<const float4*>(rhb + k);
    float4 vv[JMAX], ww[JMAX];
#pragma unroll
    for (int j = 0; j < JMAX; ++j) {
      vv[j] = *reinterpret_cast<const float4*>(vrow[j] + k);
      if (HAS_RH) ww[j] = *reinterpret_cast<const float4*>(wrow[j] + k);
    }
#pragma unroll
    for (int j = 0; j < JMAX; ++j) {
      float a = acc[j];
      a = fmaf(hv.x, vv[j].x, a); a = fmaf(hv.y, vv[j].y, a); a = fmaf(hv.z, vv[j].z, a); a = fmaf(hv.w, vv[j].w, a);
      if (HAS_RH) {
        a = fmaf(rv.x, ww[j].x, a); a = fmaf(rv.y, ww[j].y, a); a = fmaf(rv.z, ww[j].z, a); a = fmaf(rv.w, ww[j].w, a);
      }
      acc[j] = a;
    }
  }
#pragma unroll
  for (int j = 0; j < JMAX; ++j) {
    const int c = wave + 4 * j;
    const float a = wave_sum_f32(acc[j]);
    if (lane == 0 && c < C) rz[c] = a + cbv[j];
  }
  // Round 6: heads wider than 4 * JMAX classes (up to kSmallC = 256): the remaining classes in chunks of 4 * JMAX — the same dot
  // products in the same per-class order, the row re-read from LDS / L1 per chunk.  (Classes 0 .. 4 JMAX - 1 above: unchanged bits for
  // every head the earlier rounds took.)
  for (int cbase = 4 * JMAX; cbase < C; cbase += 4 * JMAX) {
    float acc2[JMAX], cb2[JMAX];
    const float* v2[JMAX];
    const float* w2[JMAX];
#pragma unroll
    for (int j = 0; j < JMAX; ++j) {
      const int cc = min(cbase + wave + 4 * j, C - 1);
      acc2[j] = 0.f;
      v2[j] = V + (int64_t)cc * K;
      w2[j] = W + (int64_t)cc * K;
      cb2[j] = cb[cc];
    }
    for (int k = 4 * lane; k < K; k += 256) {
      const float4 hv = *reinterpret_cast<const float4*>(hb + k);
      float4 rv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (HAS_RH) rv = *reinterpret_cast<const float4*>(rhb + k);
      float4 vv[JMAX], ww[JMAX];
#pragma unroll
      for (int j = 0; j < JMAX; ++j) {
        vv[j] = *reinterpret_cast<const float4*>(v2[j] + k);
        if (HAS_RH) ww[j] = *reinterpret_cast<const float4*>(w2[j] + k);
      }
#pragma unroll
      for (int j = 0; j < JMAX; ++j) {
        float a = acc2[j];
        a = fmaf(hv.x, vv[j].x, a); a = fmaf(hv.y, vv[j].y, a); a = fmaf(hv.z, vv[j].z, a); a = fmaf(hv.w, vv[j].w, a);
        if (HAS_RH) {
          a = fmaf(rv.x, ww[j].x, a); a = fmaf(rv.y, ww[j].y, a); a = fmaf(rv.z, ww[j].z, a); a = fmaf(rv.w, ww[j].w, a);
        }
        acc2[j] = a;
      }
    }
#pragma unroll
    for (int j = 0; j < JMAX; ++j) {
      const int c = cbase + wave + 4 * j;
      const float a = wave_sum_f32(acc2[j]);
      if (lane == 0 && c < C) rz[c] = a + cb2[j];
    }
  }
  __syncthreads();
  if (mode == HEAD_JVP) {
    float p = 0.f, sdv = 0.f, dt = 0.f;
    if (rz_out && t < C) rz_out[(int64_t)b * C + t] = rz[t];   // Rz_b(direction): accumulated into Rz(x) by k_cg_alpha
    // fused Neumann solver without an accumulator vector: sum_k Rz_b(v_k), one owner per sample row (deterministic)
    if (rzx_acc && t < C) rzx_acc[(int64_t)b * C + t] = (rzx_first ? 0.0 : rzx_acc[(int64_t)b * C + t]) + (double)rz[t];
    if (t < C) {
      if (PF) { p = pf_p; sdv = pf_sd; dt = pf_dt; }
      else {
        p = prob[(int64_t)b * C + t];
        sdv = sd[b];
        if (rd_prev) dt = delta_top[(int64_t)b * C + t];
      }
      pz[t] = p * rz[t];
    }
    __syncthreads();
    if (t < C) {
      float dot = 0.f;
      for (int c = 0; c < C; ++c) dot += pz[c];
      const float v = sdv * (p * rz[t] - p * dot);
      rd[(int64_t)b * C + t] = v;
      rdl[t] = v;
      dtl[t] = dt;
      t1s[t] = rz[t] * v;
    }
    if (rd_prev || partT1) __syncthreads();
    if (partT1 && t == 0) {
      double s1 = 0.0;
      for (int c = 0; c < C; ++c) s1 += (double)t1s[c];
      partT1[b] = s1;
    }
    double dacc = 0.0;
    if (PF) {       // (rd_prev != NULL by construction)
      const int k = 4 * t;
      if (k < K) {
        float4 acc2 = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 accd = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int c = 0; c < 12; ++c) {
          if (c < C) {
            const float r = rdl[c], d = dtl[c];
            const float4 v = pf_V[c], w = pf_W[c];
            acc2.x += d * v.x + r * w.x; acc2.y += d * v.y + r * w.y;
            acc2.z += d * v.z + r * w.z; acc2.w += d * v.w + r * w.w;
            accd.x += d * v.x; accd.y += d * v.y; accd.z += d * v.z; accd.w += d * v.w;
          }
        }
        acc2.x *= pf_mk.x; acc2.y *= pf_mk.y; acc2.z *= pf_mk.z; acc2.w *= pf_mk.w;
        *reinterpret_cast<float4*>(rd_prev + (int64_t)b * K + k) = acc2;
        if (rd_prev_p) *reinterpret_cast<float4*>(rd_prev_p + ((int64_t)(k >> 4) * BHG_HEAD_ROWS + b) * 16 + (k & 15)) = acc2;
        if (HAS_RH && partT2h) {
          const float4 rh4 = *reinterpret_cast<const float4*>(rhb + k);
          dacc += (double)accd.x * rh4.x + (double)accd.y * rh4.y + (double)accd.z * rh4.z + (double)accd.w * rh4.w;
        }
      }
    } else if (rd_prev) {  // fused R-backward through the head (K = feature width, K % 4 == 0)
      for (int k = 4 * t; k < K; k += 1024) {
        const float4 mk = *reinterpret_cast<const float4*>(mask_prev + (int64_t)b * K + k);
        float4 acc2 = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 accd = make_float4(0.f, 0.f, 0.f, 0.f);   // (delta_L V_L)[b][k..k+3] alone, for partT2h
        for (int c0 = 0; c0 < C; c0 += 4) {  // 8 independent 16-B loads per batch of 4 classes
          float4 w[4], v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int cc = min(c0 + u, C - 1);
            w[u] = *reinterpret_cast<const float4*>(W + (int64_t)cc * K + k);
            v[u] = *reinterpret_cast<const float4*>(V + (int64_t)cc * K + k);
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            if (c0 + u < C) {
              const float r = rdl[c0 + u], d = dtl[c0 + u];
              acc2.x += d * v[u].x + r * w[u].x; acc2.y += d * v[u].y + r * w[u].y;
              acc2.z += d * v[u].z + r * w[u].z; acc2.w += d * v[u].w + r * w[u].w;
              accd.x += d * v[u].x; accd.y += d * v[u].y; accd.z += d * v[u].z; accd.w += d * v[u].w;
            }
          }
        }
        acc2.x *= mk.x; acc2.y *= mk.y; acc2.z *= mk.z; acc2.w *= mk.w;
        *reinterpret_cast<float4*>(rd_prev + (int64_t)b * K + k) = acc2;
        if (rd_prev_p) *reinterpret_cast<float4*>(rd_prev_p + ((int64_t)(k >> 4) * BHG_HEAD_ROWS + b) * 16 + (k & 15)) = acc2;
        if (HAS_RH && partT2h) {
          const float4 rh4 = *reinterpret_cast<const float4*>(rhb + k);
          dacc += (double)accd.x * rh4.x + (double)accd.y * rh4.y + (double)accd.z * rh4.z + (double)accd.w * rh4.w;
        }
      }
    }
    if (partT2h) {
      const double s2 = block_sum(dacc, red_t);
      if (t == 0) partT2h[b] = 2.0 * s2;
    }
  } else if (mode == HEAD_COEFF) {
    if (t < C) pz[t] = (prob[(int64_t)b * C + t] - (t == (int)labels[b] ? 1.f : 0.f)) * rz[t];
    __syncthreads();
    if (t == 0) {
      float acc2 = 0.f;
      for (int c = 0; c < C; ++c) acc2 += pz[c];
      aux[b] = acc2 / (float)B;
    }
  } else if (C > 32) {  // HEAD_LOGITS for a wide head (round 6): thread = class, fixed-order sums by thread 0 over LDS
    if (t < C) pz[t] = rz[t];
    __syncthreads();
    if (t == 0) {
      float mx = pz[0];
      for (int c = 1; c < C; ++c) mx = fmaxf(mx, pz[c]);
      rdl[0] = mx;
    }
    __syncthreads();
    if (t < C) dtl[t] = expf(rz[t] - rdl[0]);
    __syncthreads();
    if (t == 0) {
      float sum = 0.f;
      for (int c = 0; c < C; ++c) sum += dtl[c];
      rdl[1] = rdl[0] + logf(sum);
    }
    __syncthreads();
    if (t < C) rd[(int64_t)b * C + t] = expf(rz[t] - rdl[1]);
    if (t == 0) aux[b] = rdl[1] - rz[(int)labels[b]];
  } else {  // HEAD_LOGITS: numerically stable log-softmax, one thread per row (C <= 32)
    if (t == 0) {
      float mx = rz[0];
      for (int c = 1; c < C; ++c) mx = fmaxf(mx, rz[c]);
      float sum = 0.f;
      for (int c = 0; c < C; ++c) sum += expf(rz[c] - mx);
      const float lse = mx + logf(sum);
      for (int c = 0; c < C; ++c) rd[(int64_t)b * C + c] = expf(rz[c] - lse);
      aux[b] = lse - rz[(int)labels[b]];
    }
  }
