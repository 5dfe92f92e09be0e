// bhg_fd.hip — the central finite difference (darts, SAMA) of a ReLU-MLP with per-sample-weighted cross-entropy, natively.
//
// betty/hypergradient/darts.py:29-67 (sama.py:25-59 alike) perturbs the live inner weights with three in-place axpys,
// w+ = w + eps v, w- = w+ - 2 eps v, w = w- + eps v (skipped under *_multitask), and differentiates the user's training_step
// at w+ and w- to the upper parameters.  For L_in = (1/B) sum_i s_lam(CE_i.detach()) CE_i(w) (+ a ridge without lam) that
// derivative is the VJP of the sample weights with cotangent CE(w+-)/B: all the inner network contributes is per-sample CE at
// the two weight sets.  Here:
//   bhg_mlp_fd_forward  per layer ONE split-K MFMA launch reads W and V once, forms w+ and w- in registers with the arithmetic
//                       of k_axpy_multi (so the network is evaluated at bit-for-bit the weights the three axpys produce), runs
//                       both products, and writes the final live weights in place (every element has exactly one owning
//                       workgroup: the grid tiles (N, K) only, the batch is looped inside).  N-sized traffic: 12 N bytes.
//                       Then a split reduce (+ bias, ReLU) per layer and one logsumexp row kernel for CE+ and CE-.
//   bhg_mwn_fd_vjp      the meta-weight-net VJP at both points (closed form of bhg_mwn.hip), combined as the reference does.
// A translation unit of its own: the K-loop kernels of bhg_mlp.hip keep their anchored code placement.
#include "bhg_common.hpp"

namespace bhg {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kFdTM = 128;      // batch rows per M tile (4 waves x 32)
constexpr int kFdTN = 32;       // output columns (weight rows) per workgroup
constexpr int kFdTK = 32;       // K step
constexpr int kFdPad = kFdTK + 4;
constexpr int kFdMaxMT = 4;     // batch <= 512 rows: the accumulators of every M tile stay in registers
constexpr int kFdWgTarget = 512;
constexpr int kFdMaxSplits = 32;

struct FdLayer {
  const float* hp;   // [M][K] activations at w+ (layer 0: the input)
  const float* hm;   // [M][K] activations at w- (layer 0: the same input)
  float* W;          // [N][K] live weights: read, and overwritten with the final weights when write_w
  const float* V;    // [N][K] direction
  float* b;          // [N] live bias (same)
  const float* vb;   // [N]
  float* bpm;        // [2][N] the perturbed biases, for the reduce
  float* part;       // [splits][2][M][N] partial products
  const float* eps;  // device scalar (fp32 eps of darts_eps)
  int M, K, N, splits, restore, write_w;
};

// The three axpys of darts.py:37-63 on one element, in k_axpy_multi's roundings (a = mul * eps).
__device__ __forceinline__ void fd_perturb(float w, float v, float a1, float a2, int restore, float& wp, float& wm, float& wf) {
  wp = add_rn(w, mul_rn(a1, v));
  wm = add_rn(wp, mul_rn(a2, v));
  wf = restore ? add_rn(wm, mul_rn(a1, v)) : wm;
}

// grid = (ceil(N / 32), splits), block = 256.  Wave w owns batch rows [32 w, 32 w + 32) of every 128-row M tile.
template <int MT>
__global__ __launch_bounds__(kThreads) void k_fd_gemm(FdLayer a) {
  __shared__ __attribute__((aligned(16))) float sBp[kFdTN * kFdPad];
  __shared__ __attribute__((aligned(16))) float sBm[kFdTN * kFdPad];
  __shared__ __attribute__((aligned(16))) float sAp[kFdTM * kFdPad];
  __shared__ __attribute__((aligned(16))) float sAm[kFdTM * kFdPad];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 31, lk = lane >> 5;
  const int n0 = blockIdx.x * kFdTN, split = blockIdx.y;
  const float eps = *a.eps;
  const float a1 = mul_rn(1.f, eps), a2 = mul_rn(-2.f, eps);
  const bool shared_a = a.hp == a.hm;

  // the biases of this column tile: the first split's workgroup owns them
  if (split == 0 && t < kFdTN && n0 + t < a.N) {
    float wp, wm, wf;
    fd_perturb(a.b[n0 + t], a.vb[n0 + t], a1, a2, a.restore, wp, wm, wf);
    a.bpm[n0 + t] = wp;
    a.bpm[a.N + n0 + t] = wm;
    if (a.write_w) a.b[n0 + t] = wf;
  }

  const int ksteps = (a.K + kFdTK - 1) / kFdTK;
  const int per = (ksteps + a.splits - 1) / a.splits;
  const int kbeg = split * per * kFdTK;
  const int kend = min(a.K, (split + 1) * per * kFdTK);

  f32x16 accp[MT], accm[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < 16; ++j) accp[i][j] = accm[i][j] = 0.f;

  for (int k0 = kbeg; k0 < kend; k0 += kFdTK) {
    // weight tile: thread t covers row n0 + (t >> 3), k = k0 + 4 (t & 7) .. +3
    {
      const int r = t >> 3, kk = 4 * (t & 7);
      const int n = n0 + r;
      float wp[4], wm[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = k0 + kk + u;
        const bool ok = n < a.N && k < kend;
        const int64_t idx = ok ? (int64_t)n * a.K + k : 0;
        const float w = ok ? a.W[idx] : 0.f;
        const float v = ok ? a.V[idx] : 0.f;
        float wf;
        fd_perturb(w, v, a1, a2, a.restore, wp[u], wm[u], wf);
        if (ok && a.write_w) a.W[idx] = wf;
        if (!ok) wp[u] = wm[u] = 0.f;
      }
      *reinterpret_cast<float4*>(sBp + r * kFdPad + kk) = make_float4(wp[0], wp[1], wp[2], wp[3]);
      *reinterpret_cast<float4*>(sBm + r * kFdPad + kk) = make_float4(wm[0], wm[1], wm[2], wm[3]);
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int m0 = mt * kFdTM;
      // activation tiles: 128 rows x 32 k, thread t covers rows (t >> 3) + 32 i
#pragma unroll
      for (int i = 0; i < kFdTM / 32; ++i) {
        const int r = (t >> 3) + 32 * i, kk = 4 * (t & 7);
        const int m = m0 + r;
        float vp[4], vm[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int k = k0 + kk + u;
          const bool ok = m < a.M && k < kend;
          const int64_t idx = ok ? (int64_t)m * a.K + k : 0;
          vp[u] = ok ? a.hp[idx] : 0.f;
          vm[u] = ok && !shared_a ? a.hm[idx] : 0.f;
        }
        *reinterpret_cast<float4*>(sAp + r * kFdPad + kk) = make_float4(vp[0], vp[1], vp[2], vp[3]);
        if (!shared_a) *reinterpret_cast<float4*>(sAm + r * kFdPad + kk) = make_float4(vm[0], vm[1], vm[2], vm[3]);
      }
      __syncthreads();
      const float* Am = shared_a ? sAp : sAm;
#pragma unroll
      for (int k8 = 0; k8 < kFdTK / 8; ++k8) {
        const int kb = 8 * k8 + 4 * lk;
        const float4 ap = *reinterpret_cast<const float4*>(sAp + (32 * wave + li) * kFdPad + kb);
        const float4 am = *reinterpret_cast<const float4*>(Am + (32 * wave + li) * kFdPad + kb);
        const float4 bp = *reinterpret_cast<const float4*>(sBp + li * kFdPad + kb);
        const float4 bm = *reinterpret_cast<const float4*>(sBm + li * kFdPad + kb);
        accp[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap.x, bp.x, accp[mt], 0, 0, 0);
        accm[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(am.x, bm.x, accm[mt], 0, 0, 0);
        accp[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap.y, bp.y, accp[mt], 0, 0, 0);
        accm[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(am.y, bm.y, accm[mt], 0, 0, 0);
        accp[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap.z, bp.z, accp[mt], 0, 0, 0);
        accm[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(am.z, bm.z, accm[mt], 0, 0, 0);
        accp[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap.w, bp.w, accp[mt], 0, 0, 0);
        accm[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(am.w, bm.w, accm[mt], 0, 0, 0);
      }
      __syncthreads();   // the activation tiles (and, after the last M tile, the weight tiles) are rewritten next
    }
  }

  // epilogue: C/D fragment of v_mfma_f32_32x32x2_f32: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const int col = n0 + li;
  if (col >= a.N) return;
  const int64_t slab = (int64_t)a.M * a.N;
  float* outp = a.part + (int64_t)split * 2 * slab;
  float* outm = outp + slab;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) {
      const int row = mt * kFdTM + 32 * wave + (rg & 3) + 8 * (rg >> 2) + 4 * lk;
      if (row < a.M) {
        outp[(int64_t)row * a.N + col] = accp[mt][rg];
        outm[(int64_t)row * a.N + col] = accm[mt][rg];
      }
    }
  }
}

// out_s[m][n] = sum over splits (in order) + bias_s[n], ReLU on hidden layers; s = 0 (w+), 1 (w-).
__global__ __launch_bounds__(kThreads) void k_fd_reduce(const float* __restrict__ part, int splits, const float* __restrict__ bpm,
                                                        float* __restrict__ outp, float* __restrict__ outm, int M, int N, int relu) {
  const int64_t slab = (int64_t)M * N;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= 2 * slab) return;
  const int s = i >= slab ? 1 : 0;
  const int64_t e = i - s * slab;
  const int n = (int)(e % N);
  float acc = 0.f;
  for (int sp = 0; sp < splits; ++sp) acc += part[(int64_t)sp * 2 * slab + s * slab + e];
  acc += bpm[s * N + n];
  if (relu) acc = acc > 0.f ? acc : 0.f;
  (s ? outm : outp)[e] = acc;
}

// One workgroup per (sample, sign): ce = logsumexp(z) - z[y].
__global__ __launch_bounds__(kThreads) void k_fd_ce(const float* __restrict__ zp, const float* __restrict__ zm,
                                                    const int64_t* __restrict__ labels, int C, int B, float* __restrict__ cep,
                                                    float* __restrict__ cem) {
  __shared__ double red[kWaves];
  __shared__ float redf[kWaves];
  const int b = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
  const float* row = (s ? zm : zp) + (int64_t)b * C;
  float mx = -INFINITY;
  for (int c = t; c < C; c += kThreads) mx = fmaxf(mx, row[c]);
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  if ((t & 63) == 0) redf[t >> 6] = mx;
  __syncthreads();
  mx = redf[0];
  for (int w = 1; w < kWaves; ++w) mx = fmaxf(mx, redf[w]);
  double sum = 0.0;
  for (int c = t; c < C; c += kThreads) sum += (double)expf(row[c] - mx);
  sum = block_sum(sum, red);
  if (t == 0) {
    int64_t y = labels[b];
    y = y < 0 ? 0 : (y >= C ? C - 1 : y);   // (an out-of-range label reads inside the row; the reference raises on it)
    (s ? cem : cep)[b] = (mx + logf((float)sum)) - row[y];
  }
}

// ---- the meta-weight-net VJP at both points (k_mwn_backward's closed form, once per point; the sums over samples in double)
constexpr int kMwnMaxH = 2048;
constexpr int kMwnChunk = 1024;

__device__ __forceinline__ float fd_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

// grads of sum_i (ce_i / B) s_i(ce_i) for ce = cep (point 0) and cem (point 1); out = (gm - gp) / two_eps, or (accumulate) out = (out +
// -(gp / two_eps)) + gm / two_eps — darts.py:44-53's two accumulations into .grad, in that order.
__global__ __launch_bounds__(kThreads) void k_mwn_fd(const float* __restrict__ cep, const float* __restrict__ cem, int B,
                                                     const float* __restrict__ w1, const float* __restrict__ b1,
                                                     const float* __restrict__ w2, const float* __restrict__ b2, int H,
                                                     const float* __restrict__ two_eps_dev, int accumulate, float* __restrict__ gw1,
                                                     float* __restrict__ gb1, float* __restrict__ gw2, float* __restrict__ gb2) {
  extern __shared__ float sp[];   // [3][H] parameters, then [2][kMwnChunk]
  __shared__ double red[kWaves];
  float* sdz = sp + 3 * H;
  float* sce = sdz + kMwnChunk;
  for (int j = threadIdx.x; j < H; j += kThreads) { sp[j] = w1[j]; sp[H + j] = b1[j]; sp[2 * H + j] = w2[j]; }
  const float bias2 = b2[0];
  const float inv_b = 1.f / (float)B;   // autograd's mean backward: grad / numel
  constexpr int kPer = kMwnMaxH / kThreads;
  constexpr int kSPer = kMwnChunk / kThreads;
  float g[2][3][kPer];
  float gb[2];
  __syncthreads();
  for (int pt = 0; pt < 2; ++pt) {
    const float* ce = pt ? cem : cep;
    // the sums over samples in double (the products of two floats are exact there), rounded to float once: g+ and g- differ by about
    // |CE+ - CE-| / |CE| of themselves, so an fp32 running sum's rounding (growing with sqrt(B)) would reach the difference itself
    double a_w1[kPer], a_b1[kPer], a_w2[kPer];
#pragma unroll
    for (int u = 0; u < kPer; ++u) a_w1[u] = a_b1[u] = a_w2[u] = 0.0;
    double a_b2 = 0.0;
    for (int i0 = 0; i0 < B; i0 += kMwnChunk) {
      const int n = B - i0 < kMwnChunk ? B - i0 : kMwnChunk;
#pragma unroll
      for (int u = 0; u < kSPer; ++u) {
        const int t = threadIdx.x + kThreads * u;
        if (t >= n) continue;
        const float c = ce[i0 + t];
        const float kc = c * inv_b;
        float z = bias2;
        for (int j = 0; j < H; ++j) {
          const float a = fmaf(sp[j], c, sp[H + j]);
          z = fmaf(sp[2 * H + j], a > 0.f ? a : 0.f, z);
        }
        const float v = fd_sigmoid(z);
        const float dz = kc * (v * (1.f - v));
        sdz[t] = dz;
        sce[t] = c;
        a_b2 += (double)dz;
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < kPer; ++u) {
        const int j = threadIdx.x + kThreads * u;
        if (j < H) {
          const float wj = sp[j], bj = sp[H + j];
          for (int t = 0; t < n; ++t) {
            const float c = sce[t], dz = sdz[t];
            const float a = fmaf(wj, c, bj);
            const double d = a > 0.f ? (double)dz : 0.0;   // the sums of dz and dz c over the active samples; times w2_j below
            a_w2[u] = fma(d, (double)a, a_w2[u]);
            a_b1[u] += d;
            a_w1[u] = fma(d, (double)c, a_w1[u]);
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int j = threadIdx.x + kThreads * u;
      const double vj = j < H ? (double)sp[2 * H + j] : 0.0;
      g[pt][0][u] = (float)(vj * a_w1[u]);
      g[pt][1][u] = (float)(vj * a_b1[u]);
      g[pt][2][u] = (float)a_w2[u];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a_b2 += __shfl_down(a_b2, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a_b2;
    __syncthreads();
    gb[pt] = (float)((red[0] + red[1]) + (red[2] + red[3]));
    __syncthreads();
  }
  const float te = *two_eps_dev;
  auto combine = [&](float* dst, float gp, float gm) {
    if (accumulate) *dst = __fadd_rn(__fadd_rn(*dst, -__fdiv_rn(gp, te)), __fdiv_rn(gm, te));
    else *dst = __fdiv_rn(__fsub_rn(gm, gp), te);
  };
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int j = threadIdx.x + kThreads * u;
    if (j < H) {
      combine(gw1 + j, g[0][0][u], g[1][0][u]);
      combine(gb1 + j, g[0][1][u], g[1][1][u]);
      combine(gw2 + j, g[0][2][u], g[1][2][u]);
    }
  }
  if (threadIdx.x == 0) combine(gb2, gb[0], gb[1]);
}

int fd_splits(int N, int K) {
  const int tiles = (N + kFdTN - 1) / kFdTN;
  const int ksteps = (K + kFdTK - 1) / kFdTK;
  int s = kFdWgTarget / tiles;
  s = s < 1 ? 1 : s;
  s = s > kFdMaxSplits ? kFdMaxSplits : s;
  s = s > ksteps ? ksteps : s;
  // every split gets at least one K step: shrink until the last one is non-empty
  while (s > 1 && (int64_t)(s - 1) * ((ksteps + s - 1) / s) >= ksteps) --s;
  return s;
}

// workspace: per hidden layer l < L-1 two activation buffers [B][N_l]; logits [2][B][C]; partials (largest layer); bpm [2][max N].
struct FdWs {
  size_t act_off[BHG_MLP_MAX_LAYERS][2];
  size_t logits_off, part_off, bpm_off, total;
};
size_t fd_align(size_t b) { return (b + 255) & ~(size_t)255; }
FdWs fd_layout(const int* dims, int L, int B) {
  FdWs w{};
  size_t off = 0, part = 0;
  int maxn = 1;
  for (int l = 0; l < L; ++l) {
    const int K = dims[l], N = dims[l + 1];
    maxn = N > maxn ? N : maxn;
    const size_t p = (size_t)fd_splits(N, K) * 2 * (size_t)B * N * sizeof(float);
    part = p > part ? p : part;
    if (l + 1 < L) {
      for (int s = 0; s < 2; ++s) { w.act_off[l][s] = off; off = fd_align(off + (size_t)B * N * sizeof(float)); }
    }
  }
  w.logits_off = off; off = fd_align(off + 2 * (size_t)B * dims[L] * sizeof(float));
  w.part_off = off; off = fd_align(off + part);
  w.bpm_off = off; off = fd_align(off + 2 * (size_t)maxn * sizeof(float));
  w.total = off;
  return w;
}

int check_fd_dims(const int* dims, int L, int B) {
  BHG_REQUIRE(dims, "NULL dims");
  BHG_REQUIRE(L >= 1 && L <= BHG_MLP_MAX_LAYERS, "unsupported layer count");
  BHG_REQUIRE(B >= 1 && B <= kFdMaxMT * kFdTM, "bhg_mlp_fd_forward takes 1 <= batch <= 512");
  for (int l = 0; l <= L; ++l) BHG_REQUIRE(dims[l] >= 1, "every width must be >= 1");
  return BHG_OK;
}

}  // namespace
}  // namespace bhg

using namespace bhg;

extern "C" {

size_t bhg_mlp_fd_ws_bytes(const int* dims, int L, int B) {
  if (check_fd_dims(dims, L, B) != BHG_OK) return 0;
  return fd_layout(dims, L, B).total;
}

int bhg_mlp_fd_forward(const float* x, const int64_t* labels, int B, const int* dims, int L, void* const* params,
                       const void* const* dir, const float* eps_dev, int restore, float* ce_plus, float* ce_minus, void* ws,
                       size_t ws_bytes, void* stream) {
  if (int rc = check_fd_dims(dims, L, B)) return rc;
  BHG_REQUIRE(x && labels && params && dir && eps_dev && ce_plus && ce_minus && ws, "NULL argument");
  const FdWs lay = fd_layout(dims, L, B);
  BHG_REQUIRE(ws_bytes >= lay.total, "workspace too small (bhg_mlp_fd_ws_bytes)");
  for (int i = 0; i < 2 * L; ++i) BHG_REQUIRE(params[i] && dir[i], "NULL parameter or direction tensor");
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  const int MT = (B + kFdTM - 1) / kFdTM;
  for (int l = 0; l < L; ++l) {
    FdLayer a{};
    a.hp = l == 0 ? x : reinterpret_cast<const float*>(base + lay.act_off[l - 1][0]);
    a.hm = l == 0 ? x : reinterpret_cast<const float*>(base + lay.act_off[l - 1][1]);
    a.W = static_cast<float*>(params[2 * l]);
    a.V = static_cast<const float*>(dir[2 * l]);
    a.b = static_cast<float*>(params[2 * l + 1]);
    a.vb = static_cast<const float*>(dir[2 * l + 1]);
    a.bpm = reinterpret_cast<float*>(base + lay.bpm_off);
    a.part = reinterpret_cast<float*>(base + lay.part_off);
    a.eps = eps_dev;
    a.M = B; a.K = dims[l]; a.N = dims[l + 1];
    a.splits = fd_splits(a.N, a.K);
    a.restore = restore != 0;
    a.write_w = 1;
    const dim3 grid((a.N + kFdTN - 1) / kFdTN, a.splits);
    switch (MT) {
      case 1: hipLaunchKernelGGL(k_fd_gemm<1>, grid, dim3(kThreads), 0, st, a); break;
      case 2: hipLaunchKernelGGL(k_fd_gemm<2>, grid, dim3(kThreads), 0, st, a); break;
      case 3: hipLaunchKernelGGL(k_fd_gemm<3>, grid, dim3(kThreads), 0, st, a); break;
      default: hipLaunchKernelGGL(k_fd_gemm<4>, grid, dim3(kThreads), 0, st, a); break;
    }
    const bool last = l == L - 1;
    float* op = reinterpret_cast<float*>(base + (last ? lay.logits_off : lay.act_off[l][0]));
    float* om = last ? op + (size_t)B * a.N : reinterpret_cast<float*>(base + lay.act_off[l][1]);
    const int64_t n = 2 * (int64_t)B * a.N;
    hipLaunchKernelGGL(k_fd_reduce, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, a.part, a.splits, a.bpm, op,
                       om, B, a.N, last ? 0 : 1);
  }
  const float* zp = reinterpret_cast<const float*>(base + lay.logits_off);
  const int C = dims[L];
  hipLaunchKernelGGL(k_fd_ce, dim3(B, 2), dim3(kThreads), 0, st, zp, zp + (size_t)B * C, labels, C, B, ce_plus, ce_minus);
  BHG_HIP_CHECK(hipGetLastError());
  return BHG_OK;
}

int bhg_mwn_fd_vjp(const float* ce_plus, const float* ce_minus, int B, const float* w1, const float* b1, const float* w2, const float* b2,
                   int H, const float* two_eps_dev, int accumulate, float* gw1, float* gb1, float* gw2, float* gb2, void* stream) {
  BHG_REQUIRE(ce_plus && ce_minus && w1 && b1 && w2 && b2 && two_eps_dev && gw1 && gb1 && gw2 && gb2, "NULL argument");
  BHG_REQUIRE(B >= 1 && H >= 1 && H <= kMwnMaxH, "the closed-form meta-weight-net takes 1 <= hidden width <= 2048");
  hipLaunchKernelGGL(k_mwn_fd, dim3(1), dim3(kThreads), sizeof(float) * (3 * (size_t)H + 2 * kMwnChunk), static_cast<hipStream_t>(stream),
                     ce_plus, ce_minus, B, w1, b1, w2, b2, H, two_eps_dev, accumulate, gw1, gb1, gw2, gb2);
  BHG_HIP_CHECK(hipGetLastError());
  return BHG_OK;
}

}  // extern "C"
