// Per-pixel-flow bilinear warp for gfx950 + C ABI (sf_flow_warp_fwd): warp_with_flow of BEVerse's motion head
// (mmdet3d/models/beverse/models/motion_modules.py:434-449) on NHWC maps, with the 2-channel 1x1 offset head
// (offset_pred / flow_pred[1], :173-174, :257-258, :353-354) optionally computed in the same launch.
//   flow      f = flow_in[p] (x, y), or W_off[2][Cf] . feat[p][0:Cf] + b_off[2]
//   source    ix = j + fx, iy = i + fy: what warp_with_flow's normalisation followed by grid_sample(align_corners=True)'s
//             un-normalisation ((j + fx)/(W-1)*2 - 1 + 1)/2*(W-1) comes to, a few ulp of W apart and exact for integer flows
//   sample    4 taps at floor / floor + 1 with grid_sample's weights and summation order (nw, ne, sw, se); a tap outside
//             [0, W) x [0, H) contributes zero and is not read, so nothing of a neighbouring image ever is
//   output    out[p*out_cs + out_co + c], c < C: a channel slice of a wider [P][out_cs] tensor (the GRU cell's input)
// Bandwidth-bound: Cf + C floats read per pixel from HBM (the taps of neighbouring pixels hit L2), C written.  A pixel's channels are
// contiguous, so a pixel takes lp = min(64, pow2 >= C/4) lanes of one float4 each (several pixels per wave below C = 256); the two dot
// products of the head are reduced across those lanes with xor shuffles, which leave the same sum in every lane.  No LDS, no atomics.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/sfnative.h"

namespace sf {

__global__ __launch_bounds__(256) void flow_warp_kernel(const float* __restrict__ state, const float* __restrict__ feat,
                                                        const float* __restrict__ w_off, const float* __restrict__ b_off,
                                                        const float* __restrict__ flow_in, float* __restrict__ out,
                                                        float* __restrict__ flow_out, int P, int H, int W, int C4, int Cf4, int lp_log2,
                                                        int out_cs, int out_co) {
  const int lp = 1 << lp_log2, sub = threadIdx.x & (lp - 1);
  const long pix = (long)blockIdx.x * (256 >> lp_log2) + (threadIdx.x >> lp_log2);
  const bool live = pix < P;
  const int p = live ? (int)pix : P - 1;      // lanes past the end redo the last pixel and store nothing: every lane reaches the shuffles
  float fx, fy;
  if (feat) {
    const float4* f = reinterpret_cast<const float4*>(feat) + (size_t)p * Cf4;
    const float4* w0 = reinterpret_cast<const float4*>(w_off);
    const float4* w1 = w0 + Cf4;
    float ax = 0.f, ay = 0.f;
    for (int k = sub; k < Cf4; k += lp) {
      const float4 v = f[k], a = w0[k], b = w1[k];
      ax += v.x * a.x + v.y * a.y + v.z * a.z + v.w * a.w;
      ay += v.x * b.x + v.y * b.y + v.z * b.z + v.w * b.w;
    }
    for (int off = lp >> 1; off; off >>= 1) {      // partners stay inside the pixel's aligned group of lp lanes
      ax += __shfl_xor(ax, off);
      ay += __shfl_xor(ay, off);
    }
    fx = ax + b_off[0];
    fy = ay + b_off[1];
  } else {
    const float2 fl = reinterpret_cast<const float2*>(flow_in)[p];
    fx = fl.x;
    fy = fl.y;
  }
  if (flow_out && live && sub == 0) reinterpret_cast<float2*>(flow_out)[p] = make_float2(fx, fy);

  const int hw = H * W, b = p / hw, r = p - b * hw, i = r / W, j = r - i * W;
  const float ix = (float)j + fx, iy = (float)i + fy;
  // floor in float, clamped to [-2, W] before the conversion (both taps of either end stay invalid): a non-finite or huge flow gives
  // invalid taps, never a wild index
  const float x0f = floorf(ix), y0f = floorf(iy);
  const int x0 = (int)fminf(fmaxf(x0f, -2.f), (float)W), y0 = (int)fminf(fmaxf(y0f, -2.f), (float)H);
  const int x1 = x0 + 1, y1 = y0 + 1;
  const bool fin = fabsf(ix) < 1e9f && fabsf(iy) < 1e9f;      // false for NaN / inf
  const bool vx0 = fin && x0 >= 0 && x0 < W, vx1 = fin && x1 >= 0 && x1 < W;
  const bool vy0 = fin && y0 >= 0 && y0 < H, vy1 = fin && y1 >= 0 && y1 < H;
  const float tx = ix - x0f, ty = iy - y0f;
  const float nw = (1.f - tx) * (1.f - ty), ne = tx * (1.f - ty), sw = (1.f - tx) * ty, se = tx * ty;
  const float4* img = reinterpret_cast<const float4*>(state) + (size_t)b * hw * C4;
  const float4* p00 = img + ((long)y0 * W + x0) * C4;      // formed, not read, unless the tap is valid
  const float4* p01 = img + ((long)y0 * W + x1) * C4;
  const float4* p10 = img + ((long)y1 * W + x0) * C4;
  const float4* p11 = img + ((long)y1 * W + x1) * C4;
  float* o = out + (size_t)p * out_cs + out_co;
  for (int c = sub; c < C4; c += lp) {
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 a = z, bq = z, cq = z, d = z;
    if (vy0 && vx0) a = p00[c];
    if (vy0 && vx1) bq = p01[c];
    if (vy1 && vx0) cq = p10[c];
    if (vy1 && vx1) d = p11[c];
    float4 v;
    v.x = a.x * nw + bq.x * ne + cq.x * sw + d.x * se;
    v.y = a.y * nw + bq.y * ne + cq.y * sw + d.y * se;
    v.z = a.z * nw + bq.z * ne + cq.z * sw + d.z * se;
    v.w = a.w * nw + bq.w * ne + cq.w * sw + d.w * se;
    if (live) reinterpret_cast<float4*>(o)[c] = v;
  }
}

static bool overlaps(const void* a, size_t an, const void* b, size_t bn) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + bn && b0 < a0 + an;
}
static bool misaligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; }

}  // namespace sf

extern "C" {

int sf_flow_warp_fwd(const float* state, const float* feat, const float* w_off, const float* b_off, const float* flow_in, float* out,
                     float* flow_out, int B, int H, int W, int C, int Cf, int out_cs, int out_co, void* stream) {
  using namespace sf;
  if (!state || !out || (feat != nullptr) == (flow_in != nullptr)) return SF_ERR_INVALID;
  if (B < 1 || H < 2 || W < 2 || C < 4 || (C % 4) || (out_cs % 4) || (out_co % 4) || out_co < 0 || out_cs < out_co + C) return SF_ERR_INVALID;
  if (feat && (!w_off || !b_off || Cf < 4 || (Cf % 4))) return SF_ERR_INVALID;
  const long P = (long)B * H * W;
  if (P >= (1L << 31)) return SF_ERR_INVALID;
  if (misaligned(state, 16) || misaligned(out, 16) || (feat && (misaligned(feat, 16) || misaligned(w_off, 16))) ||
      (flow_in && misaligned(flow_in, 8)) || (flow_out && misaligned(flow_out, 8)))
    return SF_ERR_INVALID;
  // neighbouring pixels are read while others are written: the written slice may overlap no input
  const float* o0 = out + out_co;
  const size_t on = ((size_t)(P - 1) * out_cs + C) * sizeof(float);
  if (overlaps(o0, on, state, (size_t)P * C * sizeof(float))) return SF_ERR_INVALID;
  if (feat && overlaps(o0, on, feat, (size_t)P * Cf * sizeof(float))) return SF_ERR_INVALID;
  if (flow_in && overlaps(o0, on, flow_in, (size_t)P * 2 * sizeof(float))) return SF_ERR_INVALID;
  if (flow_out && (overlaps(flow_out, (size_t)P * 2 * sizeof(float), o0, on) ||
                   overlaps(flow_out, (size_t)P * 2 * sizeof(float), state, (size_t)P * C * sizeof(float)) ||
                   (feat && overlaps(flow_out, (size_t)P * 2 * sizeof(float), feat, (size_t)P * Cf * sizeof(float)))))
    return SF_ERR_INVALID;
  int lp_log2 = 0;
  while ((1 << lp_log2) < C / 4 && lp_log2 < 6) ++lp_log2;
  const long per_block = 256 >> lp_log2;
  const long blocks = (P + per_block - 1) / per_block;      // < 2^31 / 4
  hipLaunchKernelGGL(flow_warp_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), state, feat, w_off, b_off,
                     flow_in, out, flow_out, (int)P, H, W, C / 4, feat ? Cf / 4 : 0, lp_log2, out_cs, out_co);
  return hipGetLastError() == hipSuccess ? SF_OK : SF_ERR_LAUNCH;
}

}  // extern "C"
