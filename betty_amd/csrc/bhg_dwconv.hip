// bhg_dwconv.hip — the Hessian-vector product's share of a depthwise convolution, in at most four launches.
//
// Where it sits on the path: betty/hypergradient/cg.py:39-41 / neumann.py:62 take H p as the DOUBLE BACKWARD
// `torch.autograd.grad(in_grad, params, grad_outputs=p)`.  ATen's _convolution_double_backward handles a grouped convolution with a loop
// over its groups: for the depthwise layers of a DARTS / MobileNet-style block (groups == C) that is C tiny convolutions per layer and
// term, enqueue-bound.  The layer is (groups == C_in == C_out, no bias, square k x k filter w[c, u, v], stride s,
// padding p, dilation d; taps outside the image read 0)
//     y[n, c, i, j] = sum_{u, v} w[c, u, v] * x[n, c, i s - p + u d, j s - p + v d]
// its first backward the map F : (x, w, gy) -> (gx, gw), and one Hessian-vector product needs F's vector-Jacobian product: for
// cotangents a (of gx, shaped like x) and b (of gw, shaped like w), either of which may be absent (= zero),
//     dgy = conv(a, w) + conv(x, b)                      two depthwise forwards into one output             k_dw_dgy
//     dx  = conv_backward_input(gy ; filter b)           dx[n, c, h, x] = sum_{u, v} b[c, u, v] gy[n, c, i, j],  i s - p + u d = h   k_dw_dx
//     dw  = conv_backward_weight(input a, gy)            dw[c, u, v] = sum_{n, i, j} gy[n, c, i, j] a[n, c, i s - p + u d, j s - p + v d]
//                                                        k_dw_dw_part (per-slice sums, fp64) + k_dw_dw_combine (slice order, fp64)
// (tests/dwconv_ref.py restates the three in float64; tests/test_dwconv_ref.py holds that restatement to autograd's double backward.)
//
// Every pass works on TILES of one (sample, channel) plane: a th x tw tile (powers of two, th * tw <= 256, tw <= 32) of the output
// (k_dw_dgy, k_dw_dw_part) or of the input (k_dw_dx), whose source rectangle — the tile's footprint with its halo — is staged in LDS
// with zeros where it leaves the image.  A workgroup of 256 threads takes `pb` <= 8 such UNITS side by side (small maps: four 8 x 8
// planes per workgroup), one thread per tile element.  When the source's width is a multiple of 4 the staging moves aligned groups of 4
// floats (16 bytes; a group lies wholly inside or wholly outside the image), otherwise single floats.  These passes are HBM / cache
// bound (at most 2 k^2 flop per 8 bytes): there is no MFMA.  No atomics, no grid barrier, no spin; every loop is bounded by the
// arguments; the workspace is written (k_dw_dw_part) before it is read (k_dw_dw_combine) in every call: bitwise deterministic.
//
// Layout: NCHW contiguous fp32.  K and the stride are template parameters (6 instances per kernel); dilation and padding are run-time.
#include "bhg_common.hpp"

#include <limits.h>

namespace bhg {
namespace {

constexpr int kDwMaxSlices = 64;   // slices of one channel's N * H_out * W_out terms of dw: what bhg_dwconv_ws_bytes reserves
constexpr int kDwMaxUnits = 8;     // units (plane tiles) side by side in one workgroup
constexpr int kDwMaxLds = 60 << 10;   // dynamic LDS of one workgroup: dw_tiling halves pb until the staged tiles fit

struct DwTile {
  int th, tw, lth, ltw;   // tile extent (powers of two) and their logarithms
  int pb;                 // units per workgroup: min(kDwMaxUnits, 256 / (th * tw))
  int ty, tx;             // tiles per plane
  int rows, ls;           // staged rows per unit, and the LDS row stride in floats (a multiple of 4)
  int vec;                // 4: the source is staged in aligned groups of 4 floats; 1: float by float
};

struct DwArgs {
  const float* x; const float* w; const float* gy; const float* a; const float* b;   // a, b may be NULL (zero)
  float* dx; float* dw; float* dgy;
  double* part;                    // [C][k * k][slices]
  int N, C, H, W, Ho, Wo, pad, dil;
  DwTile out;                      // tiles of the output plane: k_dw_dgy, k_dw_dw_part (source: x / a, H x W)
  DwTile in;                       // tiles of the input plane:  k_dw_dx                 (source: gy, Ho x Wo)
  long long units_out, units_in;   // N * C * ty * tx
  int upc;                         // units per channel of the dw pass: N * out.ty * out.tx
  int groups, gps, slices;         // groups of pb units per channel; groups per slice; slices per channel (<= kDwMaxSlices)
};

struct DwUnits {                   // what the first pb threads of a workgroup leave for the others
  long long plane[kDwMaxUnits];    // n * C + c, or -1 past the last unit
  int y0[kDwMaxUnits], x0[kDwMaxUnits];     // tile origin in the tiled plane
  int sy0[kDwMaxUnits], sx0[kDwMaxUnits];   // source row / column of the staged rectangle's first row / column (sx0 % 4 == 0 when vec)
};

// ceil(t / S) for S in {1, 2} and any sign of t
template <int S>
__device__ __forceinline__ int dw_cdiv(const int t) { return S == 1 ? t : (t + 1) >> 1; }

// One unit's descriptor.  `u` indexes the units of the grid (dgy, dx) or of one channel (dw); `forward` says which way the tile maps to
// its source: output tile -> input rectangle (origin * S - pad), or input tile -> the output positions that reach it.
template <int K, int S, bool FORWARD>
__device__ __forceinline__ void dw_describe(DwUnits& d, const int slot, const long long plane, const int r, const DwTile& t, const int pad,
                                            const int dil) {
  const int tyi = r / t.tx, txi = r - tyi * t.tx;
  const int y0 = tyi << t.lth, x0 = txi << t.ltw;
  d.plane[slot] = plane;
  d.y0[slot] = y0;
  d.x0[slot] = x0;
  const int sy = FORWARD ? y0 * S - pad : dw_cdiv<S>(y0 + pad - (K - 1) * dil);
  const int sx = FORWARD ? x0 * S - pad : dw_cdiv<S>(x0 + pad - (K - 1) * dil);
  d.sy0[slot] = sy;
  d.sx0[slot] = t.vec == 4 ? (sx & ~3) : sx;
}

// pb units' source rectangles -> LDS, zeros outside the image and for units past the last one.  tile: [pb][rows][ls] floats.
__device__ __forceinline__ void dw_stage(float* __restrict__ tile, const float* __restrict__ src, const DwUnits& d, const DwTile& t,
                                         const int Hs, const int Ws) {
  if (t.vec == 4) {
    const int gpr = t.ls >> 2, per = t.rows * gpr, total = t.pb * per;
    for (int idx = threadIdx.x; idx < total; idx += kThreads) {
      const int ul = idx / per, r = idx - ul * per, iy = r / gpr, g = r - iy * gpr;
      const int sy = d.sy0[ul] + iy, sx = d.sx0[ul] + 4 * g;
      const long long plane = d.plane[ul];
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (plane >= 0 && sy >= 0 && sy < Hs && sx >= 0 && sx < Ws)   // Ws % 4 == 0 and sx % 4 == 0: the group is inside as a whole
        v = *reinterpret_cast<const float4*>(src + (plane * Hs + sy) * (long long)Ws + sx);
      *reinterpret_cast<float4*>(tile + (ul * t.rows + iy) * t.ls + 4 * g) = v;
    }
  } else {
    const int per = t.rows * t.ls, total = t.pb * per;
    for (int idx = threadIdx.x; idx < total; idx += kThreads) {
      const int ul = idx / per, r = idx - ul * per, iy = r / t.ls, ix = r - iy * t.ls;
      const int sy = d.sy0[ul] + iy, sx = d.sx0[ul] + ix;
      const long long plane = d.plane[ul];
      float v = 0.f;
      if (plane >= 0 && sy >= 0 && sy < Hs && sx >= 0 && sx < Ws) v = src[(plane * Hs + sy) * (long long)Ws + sx];
      tile[(ul * t.rows + iy) * t.ls + ix] = v;
    }
  }
}

// dgy = conv(a, w) + conv(x, b).  grid = ceil(units_out / pb).
template <int K, int S>
__global__ __launch_bounds__(kThreads) void k_dw_dgy(DwArgs q) {
  extern __shared__ float4 dw_lds4[];
  __shared__ DwUnits d;
  float* lds = reinterpret_cast<float*>(dw_lds4);
  const DwTile& t = q.out;
  const int tid = threadIdx.x;
  if (tid < t.pb) {
    const long long u = (long long)blockIdx.x * t.pb + tid;
    const int tiles = t.ty * t.tx;
    const long long plane = u < q.units_out ? u / tiles : -1;
    dw_describe<K, S, true>(d, tid, plane, plane >= 0 ? (int)(u - plane * tiles) : 0, t, q.pad, q.dil);
  }
  __syncthreads();
  const int per = t.rows * t.ls;
  float* ta = lds;
  float* tx = lds + (q.a ? t.pb * per : 0);
  if (q.a) dw_stage(ta, q.a, d, t, q.H, q.W);
  if (q.b) dw_stage(tx, q.x, d, t, q.H, q.W);
  __syncthreads();
  const int ul = tid >> (t.lth + t.ltw), r = tid & ((1 << (t.lth + t.ltw)) - 1), oy = r >> t.ltw, ox = r & (t.tw - 1);
  if (ul >= t.pb) return;
  const long long plane = d.plane[ul];
  const int i = d.y0[ul] + oy, j = d.x0[ul] + ox;
  if (plane < 0 || i >= q.Ho || j >= q.Wo) return;
  const int c = (int)(plane % q.C);
  const int off = (ul * t.rows + oy * S) * t.ls + (d.x0[ul] * S - q.pad - d.sx0[ul]) + ox * S;
  float acc = 0.f;
  if (q.a) {
    const float* __restrict__ f = q.w + (long long)c * (K * K);
#pragma unroll
    for (int u = 0; u < K; ++u)
#pragma unroll
      for (int v = 0; v < K; ++v) acc = fmaf(f[u * K + v], ta[off + u * q.dil * t.ls + v * q.dil], acc);
  }
  if (q.b) {
    const float* __restrict__ f = q.b + (long long)c * (K * K);
#pragma unroll
    for (int u = 0; u < K; ++u)
#pragma unroll
      for (int v = 0; v < K; ++v) acc = fmaf(f[u * K + v], tx[off + u * q.dil * t.ls + v * q.dil], acc);
  }
  q.dgy[(plane * q.Ho + i) * (long long)q.Wo + j] = acc;
}

// dx[n, c, h, x] = sum_{u, v} b[c, u, v] gy[n, c, i, j] over the taps with i s - p + u d = h and j s - p + v d = x: a gather, so every
// element of dx is written — the rows and columns no output position reaches (stride 2) get their 0.  grid = ceil(units_in / pb).
template <int K, int S>
__global__ __launch_bounds__(kThreads) void k_dw_dx(DwArgs q) {
  extern __shared__ float4 dw_lds4[];
  __shared__ DwUnits d;
  float* tg = reinterpret_cast<float*>(dw_lds4);
  const DwTile& t = q.in;
  const int tid = threadIdx.x;
  if (tid < t.pb) {
    const long long u = (long long)blockIdx.x * t.pb + tid;
    const int tiles = t.ty * t.tx;
    const long long plane = u < q.units_in ? u / tiles : -1;
    dw_describe<K, S, false>(d, tid, plane, plane >= 0 ? (int)(u - plane * tiles) : 0, t, q.pad, q.dil);
  }
  __syncthreads();
  dw_stage(tg, q.gy, d, t, q.Ho, q.Wo);
  __syncthreads();
  const int ul = tid >> (t.lth + t.ltw), r = tid & ((1 << (t.lth + t.ltw)) - 1), oy = r >> t.ltw, ox = r & (t.tw - 1);
  if (ul >= t.pb) return;
  const long long plane = d.plane[ul];
  const int h = d.y0[ul] + oy, xx = d.x0[ul] + ox;
  if (plane < 0 || h >= q.H || xx >= q.W) return;
  const int c = (int)(plane % q.C);
  const float* __restrict__ f = q.b + (long long)c * (K * K);
  const float* __restrict__ base = tg + ul * t.rows * t.ls;
  const int sy0 = d.sy0[ul], sx0 = d.sx0[ul];
  float acc = 0.f;
#pragma unroll
  for (int u = 0; u < K; ++u) {
    const int ti = h + q.pad - u * q.dil;          // = i * S where the tap reaches an output row; >= S * sy0 by the choice of sy0
    if (S == 2 && (ti & 1)) continue;
    const int li = (S == 2 ? ti >> 1 : ti) - sy0;
#pragma unroll
    for (int v = 0; v < K; ++v) {
      const int tj = xx + q.pad - v * q.dil;
      if (S == 2 && (tj & 1)) continue;
      const int lj = (S == 2 ? tj >> 1 : tj) - sx0;
      acc = fmaf(f[u * K + v], base[li * t.ls + lj], acc);
    }
  }
  q.dx[(plane * q.H + h) * (long long)q.W + xx] = acc;
}

// dw, first stage.  grid = (slices, C): slice s of channel c takes the channel's unit groups [s * gps, (s + 1) * gps), each of pb
// (sample, tile) units; a thread keeps its k * k sums in fp64 registers, the workgroup adds them in a fixed tree: part[c][tap][s].
template <int K, int S>
__global__ __launch_bounds__(kThreads) void k_dw_dw_part(DwArgs q) {
  extern __shared__ float4 dw_lds4[];
  __shared__ DwUnits d;
  __shared__ double red[kWaves];
  float* ta = reinterpret_cast<float*>(dw_lds4);
  const DwTile& t = q.out;
  const int tid = threadIdx.x, c = blockIdx.y, s = blockIdx.x;
  const int tiles = t.ty * t.tx;
  const int ul = tid >> (t.lth + t.ltw), r = tid & ((1 << (t.lth + t.ltw)) - 1), oy = r >> t.ltw, ox = r & (t.tw - 1);
  const int g0 = s * q.gps, g1 = g0 + q.gps < q.groups ? g0 + q.gps : q.groups;
  double acc[K * K];
#pragma unroll
  for (int e = 0; e < K * K; ++e) acc[e] = 0.0;
  for (int gi = g0; gi < g1; ++gi) {
    __syncthreads();   // the previous group's readers are done with `d` and the tile
    if (tid < t.pb) {
      const int u = gi * t.pb + tid;
      const int n = u < q.upc ? u / tiles : -1;
      dw_describe<K, S, true>(d, tid, n >= 0 ? (long long)n * q.C + c : -1, n >= 0 ? u - n * tiles : 0, t, q.pad, q.dil);
    }
    __syncthreads();
    dw_stage(ta, q.a, d, t, q.H, q.W);
    __syncthreads();
    if (ul < t.pb) {
      const long long plane = d.plane[ul];
      const int i = d.y0[ul] + oy, j = d.x0[ul] + ox;
      if (plane >= 0 && i < q.Ho && j < q.Wo) {
        const double g = (double)q.gy[(plane * q.Ho + i) * (long long)q.Wo + j];
        const int off = (ul * t.rows + oy * S) * t.ls + (d.x0[ul] * S - q.pad - d.sx0[ul]) + ox * S;
#pragma unroll
        for (int u = 0; u < K; ++u)
#pragma unroll
          for (int v = 0; v < K; ++v) acc[u * K + v] += g * (double)ta[off + u * q.dil * t.ls + v * q.dil];
      }
    }
  }
  double* out = q.part + (long long)c * (K * K) * q.slices + s;
#pragma unroll
  for (int e = 0; e < K * K; ++e) {
    const double v = block_sum(acc[e], red);
    if (tid == 0) out[(long long)e * q.slices] = v;
  }
}

// dw, second stage.  grid = C: wave w adds the slices of taps w, w + 4, ... in a fixed order.  slices == 0 (a absent): dw = 0.
__global__ __launch_bounds__(kThreads) void k_dw_dw_combine(const double* __restrict__ part, float* __restrict__ dw, const int kk,
                                                            const int slices) {
  const int c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int e = wave; e < kk; e += kWaves) {
    const double v = wave_sum(sum_strided<1>(part + ((long long)c * kk + e) * slices, slices, lane, 64));
    if (lane == 0) dw[(long long)c * kk + e] = (float)v;
  }
}

inline int dw_pow2(int v, int cap) {   // the smallest power of two >= v, at most cap (a power of two)
  int p = 1;
  while (p < v && p < cap) p <<= 1;
  return p;
}
inline int dw_log2(int p) {
  int l = 0;
  while ((1 << l) < p) ++l;
  return l;
}

// The tiling of a plane of eh x ew elements.  span(n): source rows / columns that n tile rows / columns need.
inline void dw_tiling(DwTile* t, int eh, int ew, int src_w, int k, int stride, int dil, bool forward, int arrays) {
  int tw = dw_pow2(ew, 32);
  if (tw < 4) tw = 4;
  const int th = dw_pow2(eh, kThreads / tw);
  t->th = th; t->tw = tw; t->lth = dw_log2(th); t->ltw = dw_log2(tw);
  t->pb = kThreads / (th * tw) < kDwMaxUnits ? kThreads / (th * tw) : kDwMaxUnits;
  t->ty = (eh + th - 1) / th;
  t->tx = (ew + tw - 1) / tw;
  const int halo = (k - 1) * dil;
  const int rows = forward ? (th - 1) * stride + halo + 1 : (th - 1 + halo) / stride + 1;
  const int cols = forward ? (tw - 1) * stride + halo + 1 : (tw - 1 + halo) / stride + 1;
  t->rows = rows;
  t->ls = (cols + 3 + 3) & ~3;   // up to 3 columns in front of the first one when the staging starts at a multiple of 4
  // `arrays` staged tiles of pb units must fit the LDS budget: flat tiles with a wide halo (1 x 32 outputs at k = 7, d = 2, s = 2: 13 x 80
  // floats per unit) do not at pb = 8.  pb is a power of two <= 8, so this halves at most three times; one unit always fits (<= 27 KiB).
  while (t->pb > 1 && sizeof(float) * (size_t)arrays * t->pb * rows * t->ls > (size_t)kDwMaxLds) t->pb >>= 1;
  t->vec = src_w % 4 == 0 ? 4 : 1;
}

inline int dw_out_extent(int in, int k, int stride, int pad, int dil) {
  const long long span = (long long)in + 2LL * pad - (long long)dil * (k - 1) - 1;
  return span < 0 ? 0 : (int)(span / stride) + 1;
}

// Why the launch does not take a shape, or NULL where it does: bhg_dwconv_backward_vjp and bhg_dwconv_plan refuse the same shapes.
inline const char* dw_shape_error(int N, int C, int H, int W, int k, int stride, int pad, int dil) {
  if (!(N > 0 && C > 0 && H > 0 && W > 0)) return "empty tensor";
  if (C > 65535) return "more than 65535 channels";   // the channel is the grid's y dimension
  if (!(k == 3 || k == 5 || k == 7)) return "unsupported kernel size (supported: 3, 5, 7)";
  if (!(stride == 1 || stride == 2)) return "unsupported stride (supported: 1, 2)";
  if (!(dil == 1 || dil == 2)) return "unsupported dilation (supported: 1, 2)";
  if (!(pad >= 0 && pad <= dil * (k - 1))) return "padding outside 0 .. dilation * (k - 1)";
  if (dw_out_extent(H, k, stride, pad, dil) < 1 || dw_out_extent(W, k, stride, pad, dil) < 1) return "empty output";
  return nullptr;
}

inline size_t dw_lds_out(const DwArgs& q, int arrays) { return sizeof(float) * (size_t)arrays * q.out.pb * q.out.rows * q.out.ls; }
inline size_t dw_lds_in(const DwArgs& q) { return sizeof(float) * (size_t)q.in.pb * q.in.rows * q.in.ls; }

// Everything the launches take from the shape; returns NULL or why not.
inline const char* dw_plan(DwArgs* q, int N, int C, int H, int W, int k, int stride, int pad, int dil) {
  const char* bad = dw_shape_error(N, C, H, W, k, stride, pad, dil);
  if (bad) return bad;
  q->N = N; q->C = C; q->H = H; q->W = W; q->pad = pad; q->dil = dil;
  q->Ho = dw_out_extent(H, k, stride, pad, dil);
  q->Wo = dw_out_extent(W, k, stride, pad, dil);
  dw_tiling(&q->out, q->Ho, q->Wo, W, k, stride, dil, true, 2);
  dw_tiling(&q->in, H, W, q->Wo, k, stride, dil, false, 1);
  q->units_out = (long long)N * C * q->out.ty * q->out.tx;
  q->units_in = (long long)N * C * q->in.ty * q->in.tx;
  const long long upc = (long long)N * q->out.ty * q->out.tx;
  if (q->units_out > INT_MAX || q->units_in > INT_MAX || upc > INT_MAX) return "more than 2^31 - 1 tiles";
  q->upc = (int)upc;
  // slices of one channel: about 2048 workgroups per launch, never more than the workspace reserves, none empty (gps is derived from the
  // bounded count and the count recomputed from gps: no search)
  q->groups = (q->upc + q->out.pb - 1) / q->out.pb;
  int slices = (2048 + C - 1) / C;
  if (slices > kDwMaxSlices) slices = kDwMaxSlices;
  if (slices > q->groups) slices = q->groups;
  q->gps = (q->groups + slices - 1) / slices;
  q->slices = (q->groups + q->gps - 1) / q->gps;
  if (dw_lds_out(*q, 2) > (size_t)kDwMaxLds || dw_lds_in(*q) > (size_t)kDwMaxLds) return "tile larger than the LDS budget";
  return nullptr;
}

template <int K, int S>
int dw_launch(const DwArgs& q, hipStream_t st) {
  const int both = (q.a ? 1 : 0) + (q.b ? 1 : 0);
  const unsigned g_out = (unsigned)((q.units_out + q.out.pb - 1) / q.out.pb), g_in = (unsigned)((q.units_in + q.in.pb - 1) / q.in.pb);
  hipLaunchKernelGGL((k_dw_dgy<K, S>), dim3(g_out), dim3(kThreads), dw_lds_out(q, both), st, q);
  if (q.dx) {
    if (q.b)
      hipLaunchKernelGGL((k_dw_dx<K, S>), dim3(g_in), dim3(kThreads), dw_lds_in(q), st, q);
    else
      BHG_HIP_CHECK(hipMemsetAsync(q.dx, 0, sizeof(float) * (size_t)q.N * q.C * q.H * q.W, st));
  }
  if (q.dw) {
    if (q.a) hipLaunchKernelGGL((k_dw_dw_part<K, S>), dim3(q.slices, q.C), dim3(kThreads), dw_lds_out(q, 1), st, q);
    hipLaunchKernelGGL(k_dw_dw_combine, dim3(q.C), dim3(kThreads), 0, st, q.part, q.dw, K * K, q.a ? q.slices : 0);
  }
  BHG_HIP_CHECK(hipGetLastError());
  return BHG_OK;
}

}  // namespace
}  // namespace bhg

using namespace bhg;

extern "C" {

size_t bhg_dwconv_ws_bytes(int C, int k) { return C > 0 && k > 0 ? sizeof(double) * kDwMaxSlices * (size_t)k * k * (size_t)C : 0; }

int bhg_dwconv_plan(int N, int C, int H, int W, int k, int stride, int pad, int dil, char* buf, size_t buf_bytes) {
  BHG_REQUIRE(buf && buf_bytes > 0, "NULL buffer");
  DwArgs q{};
  const char* bad = dw_plan(&q, N, C, H, W, k, stride, pad, dil);
  BHG_REQUIRE(!bad, bad);
  const int len = snprintf(buf, buf_bytes,
                           "Ho=%d Wo=%d th=%d tw=%d pb=%d ty=%d tx=%d rows=%d ls=%d vec=%d ith=%d itw=%d ipb=%d ity=%d itx=%d irows=%d ils=%d "
                           "ivec=%d units=%d groups=%d gps=%d slices=%d max_slices=%d lds_dgy=%d lds_dx=%d",
                           q.Ho, q.Wo, q.out.th, q.out.tw, q.out.pb, q.out.ty, q.out.tx, q.out.rows, q.out.ls, q.out.vec, q.in.th, q.in.tw,
                           q.in.pb, q.in.ty, q.in.tx, q.in.rows, q.in.ls, q.in.vec, q.upc, q.groups, q.gps, q.slices, kDwMaxSlices,
                           (int)dw_lds_out(q, 2), (int)dw_lds_in(q));
  BHG_REQUIRE(len > 0 && (size_t)len < buf_bytes, "buffer too small for the plan line");
  return BHG_OK;
}

int bhg_dwconv_backward_vjp(const float* x, const float* w, const float* gy, const float* a, const float* b, int N, int C, int H, int W,
                            int k, int stride, int pad, int dil, float* dx, float* dw, float* dgy, void* ws, size_t ws_bytes,
                            void* stream) {
  BHG_REQUIRE(x && w && gy && dgy && ws, "null pointer");
  DwArgs q{};
  const char* bad = dw_plan(&q, N, C, H, W, k, stride, pad, dil);
  BHG_REQUIRE(!bad, bad);
  BHG_REQUIRE(ws_bytes >= bhg_dwconv_ws_bytes(C, k), "workspace smaller than bhg_dwconv_ws_bytes(C, k)");
  BHG_REQUIRE(((uintptr_t)ws & 7) == 0, "the workspace must be 8-byte aligned");
  if (q.out.vec == 4)
    for (const void* p : {b ? (const void*)x : nullptr, (const void*)a})   // x is staged only for the conv(x, b) term
      BHG_REQUIRE(((uintptr_t)p & 15) == 0, "x and a must be 16-byte aligned when W is a multiple of 4");
  if (q.in.vec == 4) BHG_REQUIRE(((uintptr_t)gy & 15) == 0, "gy must be 16-byte aligned when the output width is a multiple of 4");
  q.x = x; q.w = w; q.gy = gy; q.a = a; q.b = b; q.dx = dx; q.dw = dw; q.dgy = dgy; q.part = static_cast<double*>(ws);
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (k * 10 + stride) {
    case 31: return dw_launch<3, 1>(q, st);
    case 32: return dw_launch<3, 2>(q, st);
    case 51: return dw_launch<5, 1>(q, st);
    case 52: return dw_launch<5, 2>(q, st);
    case 71: return dw_launch<7, 1>(q, st);
    default: return dw_launch<7, 2>(q, st);
  }
}

}  // extern "C"
