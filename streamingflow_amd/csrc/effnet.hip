// EfficientNet trunk of the camera Encoder for gfx950 (efficientnet_pytorch 0.7.x model.py as streamingflow/models/encoder.py:64-105
// walks it: stem, MBConv blocks up to the version's break index, two endpoints) + its C ABI.  Eval mode, fp32, NHWC.
//
// An MBConv block is at most five launches, all on the caller's stream (no forked stream, no synchronisation, no allocation — capturable):
//
//   pointwise_kernel<SWISH>   expand 1x1 + BN + swish (absent at expand ratio 1)                 x [P][cin]      -> e [P][cexp]
//   zero fill                 the block's channel sums
//   dw_kernel<K>              depthwise KxK (K = 3, 5; stride 1, 2; four explicit pads) + BN + swish               e -> d [P'][cexp]
//                             AND the per-image channel sums of what it wrote (the SE's global pool)
//   se_gate_kernel            sums -> mean -> reduce 1x1 + bias -> swish -> expand 1x1 + bias -> sigmoid            -> gate [n][cexp]
//   pointwise_kernel<GATE>    project 1x1 + BN (+ the block's input when it has the skip); gate[image][channel] is multiplied into the
//                             input as it is staged: d is written once (dw_kernel) and read once (here), no scaling pass
//
// Channel sums.  dw_kernel adds every output as a 2^-24 fixed-point integer (llrint(y * 2^24), 64 bits): first into the workgroup's LDS
// copy, then one 64-bit integer atomic per channel and workgroup into sums[image][channel].  Integer addition is associative, so the
// sums — and everything behind them — are bitwise the same whatever order the workgroups arrive in: run to run, eager or replayed.
// |y| < 2^24 and up to 2^15 pixels per image stay far inside 63 bits; the quantisation is 2^-25 absolute on a mean of O(1) values,
// below fp32 rounding of the same mean.
//
// dw_kernel and stem_kernel are bandwidth-bound: channels run along lanes, four per lane (one 16-byte load / store), a workgroup takes
// ~2048 (pixel, channel-quad) items of one image in NHWC order, so a wave's accesses are contiguous runs of the tensor.
//
// pointwise_kernel is a plain fp32 GEMM on 64 pixel x 64 cout tiles, K in chunks of 16 through LDS, 4 x 4 outputs per lane, summed in
// ascending k: a fixed order.  Weights are sf_conv_w packs (w[cout_pad][cin_pad], cin_pad = round_up(cin, 32), cout_pad = round_up(cout, 16), zero
// filled).  Trunk channel counts are multiples of 8 but not of 16 or 32 (24, 56, 144, 336): input quads at k >= cin and weight rows at
// cout_pad and beyond are staged as zeros, never read, so the padding contributes exact zeros.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "dispatch.h"
#include "../../include/sfnative_effnet.h"

namespace sf {

constexpr float EFF_FX = 16777216.f;                   // 2^24: fixed-point scale of the channel sums
constexpr double EFF_FX_INV = 1.0 / 16777216.0;
constexpr int EFF_THREADS = 256;
constexpr int EFF_ITEMS = 2048;                        // (pixel, channel-quad) items per depthwise workgroup
constexpr int PW_TM = 64, PW_TN = 64, PW_TK = 16, PW_PITCH = PW_TM + 4;

__device__ __forceinline__ float swishf(float x) { return x / (1.f + expf(-x)); }
__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 fma4(float a, float4 w, float4 c) {
  return make_float4(fmaf(a, w.x, c.x), fmaf(a, w.y, c.y), fmaf(a, w.z, c.z), fmaf(a, w.w, c.w));
}
__device__ __forceinline__ float4 fma44(float4 a, float4 w, float4 c) {
  return make_float4(fmaf(a.x, w.x, c.x), fmaf(a.y, w.y, c.y), fmaf(a.z, w.z, c.z), fmaf(a.w, w.w, c.w));
}

// ---- stem: 3 -> C, 3x3, stride 2, pads (pt, pl), BN + swish.  img planar [n][3][H][W] or NHWC [n][H][W][3]; w [27][C], k = (ky*3 + kx)*3 + c
template <bool PLANAR>
__global__ __launch_bounds__(EFF_THREADS) void stem_kernel(const float* __restrict__ img, const float* __restrict__ w,
                                                           const float* __restrict__ scale, const float* __restrict__ bias,
                                                           float* __restrict__ out, size_t total, int H, int W, int Ho, int Wo, int C4,
                                                           int pt, int pl) {
  const size_t idx = (size_t)blockIdx.x * EFF_THREADS + threadIdx.x;
  if (idx >= total) return;
  const int c4 = (int)(idx % C4);
  const size_t p = idx / C4;
  const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho);
  const size_t im = p / ((size_t)Wo * Ho);
  const int C = 4 * C4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = 2 * oy - pt + ky;
    if (iy < 0 || iy >= H) continue;
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = 2 * ox - pl + kx;
      if (ix < 0 || ix >= W) continue;
      for (int c = 0; c < 3; ++c) {
        const float v = PLANAR ? img[((im * 3 + c) * H + iy) * W + ix] : img[((im * H + iy) * W + ix) * 3 + c];
        acc = fma4(v, ld4(w + ((ky * 3 + kx) * 3 + c) * C + 4 * c4), acc);
      }
    }
  }
  const float4 s = ld4(scale + 4 * c4), b = ld4(bias + 4 * c4);
  float4 y = fma44(acc, s, b);
  y = make_float4(swishf(y.x), swishf(y.y), swishf(y.z), swishf(y.w));
  *reinterpret_cast<float4*>(out + p * C + 4 * c4) = y;
}

// ---- depthwise K x K + BN + swish + channel sums.  grid (pixel tiles of one image, images); w [K*K][C]; dynamic LDS: C x 8 bytes
template <int K>
__global__ __launch_bounds__(EFF_THREADS) void dw_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ scale, const float* __restrict__ bias,
                                                         float* __restrict__ out, unsigned long long* __restrict__ sums, int H, int W, int Ho,
                                                         int Wo, int C4, int stride, int pt, int pl, int tile_px) {
  extern __shared__ unsigned long long lsum[];
  const int C = 4 * C4;
  const int im = blockIdx.y;
  for (int c = threadIdx.x; c < C; c += EFF_THREADS) lsum[c] = 0ull;
  __syncthreads();
  const int p0 = blockIdx.x * tile_px;
  const int npx = min(tile_px, Ho * Wo - p0);
  const float* xi = x + (size_t)im * H * W * C;
  float* oi = out + (size_t)im * Ho * Wo * C;
  for (int i = threadIdx.x; i < npx * C4; i += EFF_THREADS) {
    const int p = i / C4, c4 = i - p * C4;
    const int pix = p0 + p, oy = pix / Wo, ox = pix - oy * Wo;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
      const int iy = oy * stride - pt + ky;
      if (iy < 0 || iy >= H) continue;
#pragma unroll
      for (int kx = 0; kx < K; ++kx) {
        const int ix = ox * stride - pl + kx;
        if (ix < 0 || ix >= W) continue;
        acc = fma44(ld4(xi + ((size_t)iy * W + ix) * C + 4 * c4), ld4(w + (ky * K + kx) * C + 4 * c4), acc);
      }
    }
    float4 y = fma44(acc, ld4(scale + 4 * c4), ld4(bias + 4 * c4));
    y = make_float4(swishf(y.x), swishf(y.y), swishf(y.z), swishf(y.w));
    *reinterpret_cast<float4*>(oi + (size_t)pix * C + 4 * c4) = y;
    // two's complement: adding the unsigned image of a negative fixed-point value is the signed add
    atomicAdd(&lsum[4 * c4 + 0], (unsigned long long)__float2ll_rn(y.x * EFF_FX));
    atomicAdd(&lsum[4 * c4 + 1], (unsigned long long)__float2ll_rn(y.y * EFF_FX));
    atomicAdd(&lsum[4 * c4 + 2], (unsigned long long)__float2ll_rn(y.z * EFF_FX));
    atomicAdd(&lsum[4 * c4 + 3], (unsigned long long)__float2ll_rn(y.w * EFF_FX));
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += EFF_THREADS) atomicAdd(&sums[(size_t)im * C + c], lsum[c]);
}

// ---- SE gate: one workgroup per image.  wr [cse][C], we [C][cse]; dynamic LDS: (C + cse) floats
__global__ __launch_bounds__(EFF_THREADS) void se_gate_kernel(const unsigned long long* __restrict__ sums, const float* __restrict__ wr,
                                                              const float* __restrict__ br, const float* __restrict__ we,
                                                              const float* __restrict__ be, float* __restrict__ gate, int C, int cse,
                                                              double inv) {
  extern __shared__ float sm[];
  float* mean = sm;
  float* sq = sm + C;
  const int im = blockIdx.x;
  for (int c = threadIdx.x; c < C; c += EFF_THREADS) mean[c] = (float)((double)(long long)sums[(size_t)im * C + c] * inv);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = wave; j < cse; j += EFF_THREADS / 64) {
    float a = 0.f;
    for (int c = lane; c < C; c += 64) a = fmaf(wr[(size_t)j * C + c], mean[c], a);
    for (int o = 32; o; o >>= 1) a += __shfl_xor(a, o);      // a fixed tree: every lane ends with the same sum
    if (lane == 0) sq[j] = swishf(a + br[j]);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += EFF_THREADS) {
    float a = be[c];
    for (int j = 0; j < cse; ++j) a = fmaf(we[(size_t)c * cse + j], sq[j], a);
    gate[(size_t)im * C + c] = sigmoidf(a);
  }
}

// ---- 1x1 convolution: out[p][co] = act((sum_k x[p][k] * gate[image(p)][k] * w[co][k]) * scale[co] + bias[co]) + res[p][co]
template <bool GATE, bool SWISH>
__global__ __launch_bounds__(EFF_THREADS) void pointwise_kernel(const float* __restrict__ x, const float* __restrict__ gate,
                                                                const float* __restrict__ w, const float* __restrict__ scale,
                                                                const float* __restrict__ bias, const float* __restrict__ res,
                                                                float* __restrict__ out, size_t P, int HW, int cin, int cin_pad, int cout,
                                                                int cout_pad) {
  __shared__ __attribute__((aligned(16))) float Xs[PW_TK][PW_PITCH];
  __shared__ __attribute__((aligned(16))) float Ws[PW_TK][PW_PITCH];
  const size_t p0 = (size_t)blockIdx.x * PW_TM;
  const int co0 = blockIdx.y * PW_TN;
  const int lr = threadIdx.x >> 2, lq = (threadIdx.x & 3) * 4;      // staging: row of the tile, first k of this lane's quad
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;           // compute: pixels 4 ty .. + 3, couts 4 tx .. + 3
  const size_t lp = p0 + lr;
  const bool lp_ok = lp < P;
  const float* xrow = x + lp * cin;
  const float* grow = GATE && lp_ok ? gate + (lp / HW) * cin : nullptr;
  const bool lw_ok = co0 + lr < cout_pad;
  const float* wrow = w + (size_t)(co0 + lr) * cin_pad;
  float acc[4][4] = {};
  for (int k0 = 0; k0 < cin; k0 += PW_TK) {
    const int k = k0 + lq;
    float4 xv = make_float4(0.f, 0.f, 0.f, 0.f), wv = xv;
    if (lp_ok && k < cin) {      // cin is a multiple of 4: a quad is inside or outside as a whole
      xv = ld4(xrow + k);
      if (GATE) {
        const float4 g = ld4(grow + k);
        xv = make_float4(xv.x * g.x, xv.y * g.y, xv.z * g.z, xv.w * g.w);
      }
    }
    if (lw_ok && k < cin_pad) wv = ld4(wrow + k);
    __syncthreads();      // the previous chunk has been read
    Xs[lq + 0][lr] = xv.x; Xs[lq + 1][lr] = xv.y; Xs[lq + 2][lr] = xv.z; Xs[lq + 3][lr] = xv.w;
    Ws[lq + 0][lr] = wv.x; Ws[lq + 1][lr] = wv.y; Ws[lq + 2][lr] = wv.z; Ws[lq + 3][lr] = wv.w;
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < PW_TK; ++kk) {
      const float4 a = ld4(&Xs[kk][4 * ty]), b = ld4(&Ws[kk][4 * tx]);
      const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
    }
  }
  const int co = co0 + 4 * tx;
  if (co >= cout) return;      // cout is a multiple of 4
  const float4 s = scale ? ld4(scale + co) : make_float4(1.f, 1.f, 1.f, 1.f);
  const float4 b = bias ? ld4(bias + co) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const size_t p = p0 + 4 * ty + i;
    if (p >= P) break;
    float4 y = fma44(make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]), s, b);
    if (SWISH) y = make_float4(swishf(y.x), swishf(y.y), swishf(y.z), swishf(y.w));
    if (res) {
      const float4 r = ld4(res + p * cout + co);
      y = make_float4(y.x + r.x, y.y + r.y, y.z + r.z, y.w + r.w);
    }
    *reinterpret_cast<float4*>(out + p * cout + co) = y;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
static inline bool aligned16(const void* p) { return !((uintptr_t)p & 15); }
static inline int launched() { return hipGetLastError() == hipSuccess ? SF_OK : SF_ERR_LAUNCH; }
static inline int out_size(int in, int k, int stride, int p0, int p1) { return (in + p0 + p1 - k) / stride + 1; }

static int check_stem(const sf_effnet_w& w) {
  if (!w.stem_w || !w.stem_scale || !w.stem_bias || w.c_stem < 1 || w.pad_t < 0 || w.pad_l < 0 || w.pad_b < 0 || w.pad_r < 0 ||
      w.pad_t > 2 || w.pad_l > 2 || w.pad_b > 2 || w.pad_r > 2 || !aligned16(w.stem_w) || !aligned16(w.stem_scale) || !aligned16(w.stem_bias))
    return SF_ERR_INVALID;
  return w.c_stem % 8 ? SF_ERR_UNSUPPORTED : SF_OK;
}

static int stem(const sf_effnet_w& w, const float* img, int planar, float* out, int n, int H, int W, hipStream_t st) {
  const int Ho = out_size(H, 3, 2, w.pad_t, w.pad_b), Wo = out_size(W, 3, 2, w.pad_l, w.pad_r), C4 = w.c_stem / 4;
  const size_t total = (size_t)n * Ho * Wo * C4, blocks = (total + EFF_THREADS - 1) / EFF_THREADS;
  if (blocks >= (size_t(1) << 31)) return SF_ERR_UNSUPPORTED;
  if (planar)
    hipLaunchKernelGGL(stem_kernel<true>, dim3((unsigned)blocks), dim3(EFF_THREADS), 0, st, img, w.stem_w, w.stem_scale, w.stem_bias, out, total,
                       H, W, Ho, Wo, C4, w.pad_t, w.pad_l);
  else
    hipLaunchKernelGGL(stem_kernel<false>, dim3((unsigned)blocks), dim3(EFF_THREADS), 0, st, img, w.stem_w, w.stem_scale, w.stem_bias, out, total,
                       H, W, Ho, Wo, C4, w.pad_t, w.pad_l);
  return launched();
}

// a 1x1 pack the pointwise kernel takes
static int check_pointwise(const sf_conv_w& c) {
  if (!c.w || c.kh != 1 || c.kw != 1 || c.stride != 1 || c.dil != 1 || c.pad != 0 || c.c1 != 0 || c.c0 < 1 || c.cout < 1 || c.cin_pad < c.c0 ||
      (c.cin_pad % 16) || c.cout_pad < c.cout || !aligned16(c.w) || !aligned16(c.scale) || !aligned16(c.bias))
    return SF_ERR_INVALID;
  return (c.c0 % 8) || (c.cout % 8) ? SF_ERR_UNSUPPORTED : SF_OK;
}

static int pointwise(const sf_conv_w& c, const float* x, const float* gate, const float* res, float* out, bool swish, size_t P, int HW,
                     hipStream_t st) {
  const size_t gx = (P + PW_TM - 1) / PW_TM;
  if (gx >= (size_t(1) << 31)) return SF_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)gx, (unsigned)((c.cout + PW_TN - 1) / PW_TN)), block(EFF_THREADS);
#define SF_PW(G, S) \
  hipLaunchKernelGGL((pointwise_kernel<G, S>), grid, block, 0, st, x, gate, c.w, c.scale, c.bias, res, out, P, HW, c.c0, c.cin_pad, c.cout, c.cout_pad)
  if (gate && swish) SF_PW(true, true);
  else if (gate) SF_PW(true, false);
  else if (swish) SF_PW(false, true);
  else SF_PW(false, false);
#undef SF_PW
  return launched();
}

struct MbGeom {
  int Ho, Wo;
};
// SF_ERR_INVALID: not an MBConv block; SF_ERR_UNSUPPORTED: a block this file has no kernel for.  Reads no device memory
static int check_block(const sf_mbconv_w& b, int H, int W, MbGeom* g) {
  if (b.cin < 1 || b.cexp < 1 || b.cout < 1 || b.cse < 1 || H < 1 || W < 1) return SF_ERR_INVALID;
  if ((b.k != 3 && b.k != 5) || (b.stride != 1 && b.stride != 2) || (b.cin % 8) || (b.cexp % 8) || (b.cout % 8)) return SF_ERR_UNSUPPORTED;
  if (!b.dw_w || !b.dw_scale || !b.dw_bias || !b.se_reduce_w || !b.se_reduce_b || !b.se_expand_w || !b.se_expand_b) return SF_ERR_INVALID;
  if (!aligned16(b.dw_w) || !aligned16(b.dw_scale) || !aligned16(b.dw_bias)) return SF_ERR_INVALID;
  if (b.pad_t < 0 || b.pad_l < 0 || b.pad_b < 0 || b.pad_r < 0 || b.pad_t >= b.k || b.pad_l >= b.k || b.pad_b >= b.k || b.pad_r >= b.k)
    return SF_ERR_INVALID;
  if (b.expand.w) {
    SF_TRY(check_pointwise(b.expand));
    if (b.expand.c0 != b.cin || b.expand.cout != b.cexp) return SF_ERR_INVALID;
  } else if (b.cexp != b.cin) {
    return SF_ERR_INVALID;
  }
  SF_TRY(check_pointwise(b.project));
  if (b.project.c0 != b.cexp || b.project.cout != b.cout) return SF_ERR_INVALID;
  if (b.skip && (b.stride != 1 || b.cin != b.cout)) return SF_ERR_INVALID;
  if (H + b.pad_t + b.pad_b < b.k || W + b.pad_l + b.pad_r < b.k) return SF_ERR_INVALID;
  g->Ho = out_size(H, b.k, b.stride, b.pad_t, b.pad_b);
  g->Wo = out_size(W, b.k, b.stride, b.pad_l, b.pad_r);
  if ((size_t)b.cexp * (sizeof(float) + sizeof(unsigned long long)) + b.cse * sizeof(float) > 48 * 1024) return SF_ERR_UNSUPPORTED;      // LDS of the two small kernels
  return SF_OK;
}

static int dwconv(const sf_mbconv_w& b, const float* x, float* out, unsigned long long* sums, int n, int H, int W, const MbGeom& g, hipStream_t st) {
  const int C4 = b.cexp / 4;
  const int tile_px = std::max(1, EFF_ITEMS / C4);
  const long tiles = ((long)g.Ho * g.Wo + tile_px - 1) / tile_px;
  if (tiles >= (1L << 31) || n > 65535 || (long)g.Ho * g.Wo * C4 >= (1L << 31) || (long)H * W >= (1L << 31)) return SF_ERR_UNSUPPORTED;
  SF_HIP(zero_fill(sums, (size_t)n * b.cexp * sizeof(unsigned long long), st));
  const dim3 grid((unsigned)tiles, (unsigned)n), block(EFF_THREADS);
  const size_t lds = (size_t)b.cexp * sizeof(unsigned long long);
  if (b.k == 3)
    hipLaunchKernelGGL(dw_kernel<3>, grid, block, lds, st, x, b.dw_w, b.dw_scale, b.dw_bias, out, sums, H, W, g.Ho, g.Wo, C4, b.stride, b.pad_t,
                       b.pad_l, tile_px);
  else
    hipLaunchKernelGGL(dw_kernel<5>, grid, block, lds, st, x, b.dw_w, b.dw_scale, b.dw_bias, out, sums, H, W, g.Ho, g.Wo, C4, b.stride, b.pad_t,
                       b.pad_l, tile_px);
  return launched();
}

static int se_gate(const sf_mbconv_w& b, const unsigned long long* sums, float* gate, int n, int HW, hipStream_t st) {
  const size_t lds = (size_t)(b.cexp + b.cse) * sizeof(float);
  hipLaunchKernelGGL(se_gate_kernel, dim3((unsigned)n), dim3(EFF_THREADS), lds, st, sums, b.se_reduce_w, b.se_reduce_b, b.se_expand_w,
                     b.se_expand_b, gate, b.cexp, b.cse, EFF_FX_INV / (double)HW);
  return launched();
}

// the block's workspace (dispatch.h: Arena): the expanded tensor (nothing at ratio 1), the depthwise output, the channel sums and the gate
struct MbBufs {
  float *e, *d, *gate;
  unsigned long long* sums;
  void take(Arena& A, size_t e_floats, size_t d_floats, size_t nc) {
    e = A.take(e_floats); d = A.take(d_floats);
    sums = reinterpret_cast<unsigned long long*>(A.take(2 * nc)); gate = A.take(nc);
  }
};
struct MbLayout {
  MbBufs b;
  void take(Arena& A, const sf_mbconv_w* w, int n, int H, int W) {
    const size_t ho = out_size(H, w->k, w->stride ? w->stride : 1, w->pad_t, w->pad_b), wo = out_size(W, w->k, w->stride ? w->stride : 1, w->pad_l, w->pad_r);
    b.take(A, w->expand.w ? (size_t)n * H * W * w->cexp : 0, (size_t)n * ho * wo * w->cexp, (size_t)n * w->cexp);
  }
};

static int mbconv(const sf_mbconv_w& b, const float* x, float* out, int n, int H, int W, const MbGeom& g, const MbBufs& B, hipStream_t st) {
  const size_t P = (size_t)n * H * W, Po = (size_t)n * g.Ho * g.Wo;
  const float* e = x;
  if (b.expand.w) {
    SF_TRY(pointwise(b.expand, x, nullptr, nullptr, B.e, true, P, H * W, st));
    e = B.e;
  }
  SF_TRY(dwconv(b, e, B.d, B.sums, n, H, W, g, st));
  SF_TRY(se_gate(b, B.sums, B.gate, n, g.Ho * g.Wo, st));
  return pointwise(b.project, B.d, B.gate, b.skip ? x : nullptr, out, false, Po, g.Ho * g.Wo, st);
}

// the trunk's walk on shapes only: sizes after the stem and after every block, the blocks whose outputs are the two endpoints
struct TrunkPlan {
  std::vector<int> Hs, Ws;      // [0]: after the stem, [i + 1]: after block i
  std::vector<MbGeom> geo;
  size_t x_max = 0, e_max = 0, d_max = 0, nc_max = 0;
  int hi = -1, lo = -1;         // producers of reduction_{index + 1} / reduction_{index}: block numbers, -1 = the stem
  int status = SF_OK;
};
// encoder.py:64-105: an endpoint is recorded whenever the resolution drops (the tensor BEFORE the drop), the last output is the final one
static TrunkPlan plan_trunk(const sf_effnet_w& w, int n, int H, int W, bool check) {
  TrunkPlan t;
  if (w.n_blocks < 1 || !w.blocks || n < 1 || H < 1 || W < 1 || w.index < 1) { t.status = SF_ERR_INVALID; return t; }
  if (check && (t.status = check_stem(w)) != SF_OK) return t;
  if (H + w.pad_t + w.pad_b < 3 || W + w.pad_l + w.pad_r < 3) { t.status = SF_ERR_INVALID; return t; }
  int h = out_size(H, 3, 2, w.pad_t, w.pad_b), wd = out_size(W, 3, 2, w.pad_l, w.pad_r), c = w.c_stem;
  t.Hs.push_back(h); t.Ws.push_back(wd);
  t.x_max = (size_t)n * h * wd * c;
  std::vector<int> ends;
  for (int i = 0; i < w.n_blocks; ++i) {
    const sf_mbconv_w& b = w.blocks[i];
    MbGeom g{};
    if ((t.status = check ? check_block(b, h, wd, &g) : SF_OK) != SF_OK) return t;
    if (!check) {
      if (b.k < 1 || b.stride < 1 || b.cexp < 1 || b.cout < 1 || h + b.pad_t + b.pad_b < b.k || wd + b.pad_l + b.pad_r < b.k) { t.status = SF_ERR_INVALID; return t; }
      g.Ho = out_size(h, b.k, b.stride, b.pad_t, b.pad_b); g.Wo = out_size(wd, b.k, b.stride, b.pad_l, b.pad_r);
    }
    if (check && b.cin != c) { t.status = SF_ERR_INVALID; return t; }
    if (b.expand.w) t.e_max = std::max(t.e_max, (size_t)n * h * wd * b.cexp);
    t.d_max = std::max(t.d_max, (size_t)n * g.Ho * g.Wo * b.cexp);
    t.nc_max = std::max(t.nc_max, (size_t)n * b.cexp);
    t.x_max = std::max(t.x_max, (size_t)n * g.Ho * g.Wo * b.cout);
    if (h > g.Ho) ends.push_back(i - 1);
    h = g.Ho; wd = g.Wo; c = b.cout;
    t.Hs.push_back(h); t.Ws.push_back(wd); t.geo.push_back(g);
  }
  ends.push_back(w.n_blocks - 1);
  if ((int)ends.size() < w.index + 1) { t.status = SF_ERR_INVALID; return t; }      // the image is too small to reach the endpoint
  t.hi = ends[w.index]; t.lo = ends[w.index - 1];
  return t;
}

// the trunk's workspace: two activation buffers the blocks alternate between (the endpoints are written where the caller wants them) and
// one MbBufs large enough for every block
struct TrunkBufs {
  float* x[2];
  MbBufs mb;
  void take(Arena& A, const TrunkPlan* t) {
    x[0] = A.take(t->x_max); x[1] = A.take(t->x_max);
    mb.take(A, t->e_max, t->d_max, t->nc_max);
  }
};

}  // namespace sf

extern "C" {

using namespace sf;

int sf_effnet_abi_version(void) { return SF_EFFNET_ABI_VERSION; }
size_t sf_effnet_abi_sizeof(int which) {
  return which == SF_EFFNET_STRUCT_MBCONV_W ? sizeof(sf_mbconv_w) : which == SF_EFFNET_STRUCT_EFFNET_W ? sizeof(sf_effnet_w) : 0;
}

int sf_effnet_stem_fwd(const void* w_, const float* image, int planar, float* out, int n, int H, int W, void* stream) {
  const sf_effnet_w* w = static_cast<const sf_effnet_w*>(w_);
  if (!w || !image || !out || n < 1 || H < 1 || W < 1 || !aligned16(out)) return SF_ERR_INVALID;
  SF_TRY(check_stem(*w));
  if (H + w->pad_t + w->pad_b < 3 || W + w->pad_l + w->pad_r < 3) return SF_ERR_INVALID;
  return stem(*w, image, planar, out, n, H, W, static_cast<hipStream_t>(stream));
}

int sf_effnet_dwconv_fwd(const void* b_, const float* x, float* out, uint64_t* sums, int n, int H, int W, void* stream) {
  const sf_mbconv_w* b = static_cast<const sf_mbconv_w*>(b_);
  MbGeom g;
  if (!b || !x || !out || !sums || n < 1 || !aligned16(x) || !aligned16(out) || !aligned16(sums)) return SF_ERR_INVALID;
  SF_TRY(check_block(*b, H, W, &g));
  return dwconv(*b, x, out, reinterpret_cast<unsigned long long*>(sums), n, H, W, g, static_cast<hipStream_t>(stream));
}

int sf_effnet_se_gate_fwd(const void* b_, const uint64_t* sums, float* gate, int n, int HW, void* stream) {
  const sf_mbconv_w* b = static_cast<const sf_mbconv_w*>(b_);
  MbGeom g;
  if (!b || !sums || !gate || n < 1 || HW < 1) return SF_ERR_INVALID;
  SF_TRY(check_block(*b, b->k, b->k, &g));
  return se_gate(*b, reinterpret_cast<const unsigned long long*>(sums), gate, n, HW, static_cast<hipStream_t>(stream));
}

int sf_effnet_pointwise_fwd(const sf_conv_w* w, const float* x, const float* gate, const float* residual, float* out, int swish, int n, int HW,
                            void* stream) {
  if (!w || !x || !out || n < 1 || HW < 1 || !aligned16(x) || !aligned16(gate) || !aligned16(residual) || !aligned16(out)) return SF_ERR_INVALID;
  SF_TRY(check_pointwise(*w));
  return pointwise(*w, x, gate, residual, out, swish != 0, (size_t)n * HW, HW, static_cast<hipStream_t>(stream));
}

size_t sf_mbconv_ws_bytes(const void* b_, int n, int H, int W) {
  const sf_mbconv_w* b = static_cast<const sf_mbconv_w*>(b_);
  if (!b || n < 1 || H < 1 || W < 1 || b->k < 1 || b->stride < 1 || b->cexp < 1 || H + b->pad_t + b->pad_b < b->k || W + b->pad_l + b->pad_r < b->k) return 0;
  return layout_bytes<MbLayout>(b, n, H, W);
}

int sf_mbconv_fwd(const void* b_, const float* x, float* out, int n, int H, int W, float* ws, size_t ws_bytes, void* stream) {
  const sf_mbconv_w* b = static_cast<const sf_mbconv_w*>(b_);
  MbGeom g;
  if (!b || !x || !out || n < 1 || !aligned16(x) || !aligned16(out) || !aligned16(ws)) return SF_ERR_INVALID;
  SF_TRY(check_block(*b, H, W, &g));
  MbLayout L;
  if (!carve(L, ws, ws_bytes, b, n, H, W)) return SF_ERR_WORKSPACE;
  return mbconv(*b, x, out, n, H, W, g, L.b, static_cast<hipStream_t>(stream));
}

size_t sf_effnet_trunk_ws_bytes(const void* w_, int n, int H, int W) {
  const sf_effnet_w* w = static_cast<const sf_effnet_w*>(w_);
  if (!w) return 0;
  const TrunkPlan t = plan_trunk(*w, n, H, W, false);
  return t.status == SF_OK ? layout_bytes<TrunkBufs>(&t) : 0;
}

int sf_effnet_trunk_fwd(const void* w_, const float* image, int planar, float* out_hi, float* out_lo, int n, int H, int W, float* ws,
                        size_t ws_bytes, void* stream) {
  const sf_effnet_w* w = static_cast<const sf_effnet_w*>(w_);
  if (!w || !image || !out_hi || !out_lo || !aligned16(out_hi) || !aligned16(out_lo) || !aligned16(ws)) return SF_ERR_INVALID;
  const TrunkPlan t = plan_trunk(*w, n, H, W, true);      // every refusal comes before the first launch
  if (t.status != SF_OK) return t.status;
  TrunkBufs B;
  if (!carve(B, ws, ws_bytes, &t)) return SF_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  auto dst = [&](int producer, int flip) { return producer == t.hi ? out_hi : producer == t.lo ? out_lo : B.x[flip]; };
  float* cur = dst(-1, 0);
  SF_TRY(stem(*w, image, planar, cur, n, H, W, st));
  for (int i = 0; i < w->n_blocks; ++i) {
    float* nxt = dst(i, (i + 1) & 1);
    SF_TRY(mbconv(w->blocks[i], cur, nxt, n, t.Hs[i], t.Ws[i], t.geo[i], B.mb, st));
    cur = nxt;
  }
  return SF_OK;
}

}  // extern "C"
