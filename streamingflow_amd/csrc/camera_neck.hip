// Camera encoder neck for gfx950 (streamingflow/models/encoder.py:107-112 after the endpoint selection) + its C ABI.
//
// Reference: per branch (features, depth) DeepLabHead(c_hi, c_hi, 64) on the /16 endpoint, then UpsamplingConcat
// (layers/convolutions.py:183-201): bilinear x2, cat[/8 endpoint, upsampled], two 3x3 conv + BN + ReLU.  Here both heads are ONE
// sf_deeplab_w (hid = 2 * 64: branch and pooling weights stacked on cout, projection / 3x3 / classifier block-diagonal; packed by
// streamingflow_amd/models/encoder.py), so the chain is
//
//   sf_deeplab_head_fwd          the twin head: [n][H][W][c_hi] -> [n][H][W][2 c_hi] = [feature | depth]
//   sf_upsample_bilinear2_add    one launch for both halves -> [n][2H][2W][2 c_hi]
//   sf_conv2d_ex_fwd x 4         conv1 of each branch reads in0 = the /8 endpoint, in1 = its channel slice of the upsampled tensor
//                                (in1_cs = 2 c_hi; nothing concatenated is written), conv2 follows; the feature branch ends as the rays
//                                [n * 4HW][C] the lift gathers from
//   depth_softmax_planar_kernel  the depth branch's NHWC logits [P][D] -> planar logits AND planar probabilities [n][D][4HW], the
//                                layouts the model returns (depth_prediction) and the lift reads — one pass, no transpose launch
//
// all on the caller's stream: no forked stream, no synchronisation, no allocation — capturable.
//
// depth_softmax_planar_kernel is bandwidth-bound layout work.  A workgroup (4 waves) takes 64 consecutive pixels of one image: the
// 64 x D logits arrive as 16-byte loads along D (a pixel's D floats are contiguous) into LDS rows of pitch D + 1 — odd, so the column
// reads of the later phases (lane = pixel, fixed d: ds_read_b32, banks mod 32 per 32-lane half) hit 32 different banks.  Each wave
// then owns a quarter of the depth bins: partial max, max of the four, partial sums of expf(x - max), sum of the four in a fixed
// order, and for each of its d rows one 256-byte store of the logits and one of expf(x - max) / sum.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "dispatch.h"

namespace sf {

constexpr int DSP_TILE = 64;      // pixels per workgroup = lanes of a wave
constexpr int DSP_WAVES = 4;
constexpr int DSP_MAX_D = 128;

__global__ __launch_bounds__(DSP_TILE* DSP_WAVES) void depth_softmax_planar_kernel(const float* __restrict__ logits, int cs, int co,
                                                                                   float* __restrict__ out_logits,
                                                                                   float* __restrict__ out_prob, int D, int fHW,
                                                                                   int tiles_per_img) {
  extern __shared__ float sm[];      // [64][D + 1] | pmax [4][64] | psum [4][64]
  const int pitch = D + 1;
  float* pmax = sm + DSP_TILE * pitch;
  float* psum = pmax + DSP_WAVES * DSP_TILE;
  const int img = blockIdx.x / tiles_per_img, tile = blockIdx.x - img * tiles_per_img;
  const int p0 = tile * DSP_TILE;
  const int npx = min(DSP_TILE, fHW - p0);      // the tail tile of an image is short; tiles never straddle images
  const int D4 = D >> 2;
  const float* src = logits + ((size_t)img * fHW + p0) * cs + co;
  for (int i = threadIdx.x; i < npx * D4; i += DSP_TILE * DSP_WAVES) {
    const int p = i / D4, q = i - p * D4;
    const float4 v = *reinterpret_cast<const float4*>(src + (size_t)p * cs + 4 * q);
    float* row = sm + p * pitch + 4 * q;
    row[0] = v.x; row[1] = v.y; row[2] = v.z; row[3] = v.w;
  }
  __syncthreads();
  const int lane = threadIdx.x & (DSP_TILE - 1), wave = threadIdx.x / DSP_TILE;
  const bool live = lane < npx;
  const float* mine = sm + lane * pitch;
  const int d0 = wave * D4, d1 = d0 + D4;      // this wave's quarter of the bins
  float m = -INFINITY;
  if (live)
    for (int d = d0; d < d1; ++d) m = fmaxf(m, mine[d]);
  pmax[wave * DSP_TILE + lane] = m;
  __syncthreads();
  m = fmaxf(fmaxf(pmax[lane], pmax[DSP_TILE + lane]), fmaxf(pmax[2 * DSP_TILE + lane], pmax[3 * DSP_TILE + lane]));
  float s = 0.f;
  if (live)
    for (int d = d0; d < d1; ++d) s += expf(mine[d] - m);
  psum[wave * DSP_TILE + lane] = s;
  __syncthreads();
  if (!live) return;
  const float sum = ((psum[lane] + psum[DSP_TILE + lane]) + psum[2 * DSP_TILE + lane]) + psum[3 * DSP_TILE + lane];
  const size_t plane = ((size_t)img * D + d0) * fHW + p0 + lane;
  for (int d = d0; d < d1; ++d) {      // one d row per store: the wave writes 64 consecutive floats
    const float x = mine[d];
    const size_t o = plane + (size_t)(d - d0) * fHW;
    out_logits[o] = x;
    out_prob[o] = expf(x - m) / sum;
  }
}

static int depth_softmax_planar(const float* logits, int cs, int co, float* out_logits, float* out_prob, int rows, int D, int fHW,
                                hipStream_t st) {
  if (!logits || !out_logits || !out_prob || rows < 1 || D < 1 || fHW < 1 || co < 0) return SF_ERR_INVALID;
  if ((D % 4) || D > DSP_MAX_D) return SF_ERR_UNSUPPORTED;
  if ((cs % 4) || (co % 4) || co + D > cs || ((uintptr_t)logits & 15)) return SF_ERR_INVALID;
  const long tiles = (fHW + DSP_TILE - 1) / DSP_TILE;
  if (rows * tiles >= (1L << 31)) return SF_ERR_UNSUPPORTED;
  const size_t lds = ((size_t)DSP_TILE * (D + 1) + 2 * DSP_WAVES * DSP_TILE) * sizeof(float);      // <= 35 KB
  hipLaunchKernelGGL(depth_softmax_planar_kernel, dim3((unsigned)(rows * tiles)), dim3(DSP_TILE * DSP_WAVES), lds, st, logits, cs, co,
                     out_logits, out_prob, D, fHW, (int)tiles);
  return hipGetLastError() == hipSuccess ? SF_OK : SF_ERR_LAUNCH;
}

struct NeckShape {
  int c_hi, c_lo, C, D, hid;
};
// the neck's workspace (dispatch.h: Arena): the twin head's output, its upsampling, conv1's output of either branch, the depth logits as
// NHWC, and the workspaces of the head and of the convolutions' split-K, as their own queries size them
struct NeckBufs {
  float *head_out, *up, *t_feat, *t_depth, *d_nhwc, *head_ws, *conv_ws;
  size_t head_ws_bytes, conv_ws_bytes;
  void take(Arena& A, const NeckShape& s, int n, int H, int W) {
    const size_t P = (size_t)n * H * W;
    head_out = A.take(P * 2 * s.c_hi); up = A.take(4 * P * 2 * s.c_hi);
    t_feat = A.take(4 * P * s.C); t_depth = A.take(4 * P * s.D); d_nhwc = A.take(4 * P * s.D);
    head_ws_bytes = sf_deeplab_head_ws_bytes(s.c_hi, s.hid, n, H, W); conv_ws_bytes = sf_conv2d_ex_ws_bytes();
    head_ws = A.take(head_ws_bytes / sizeof(float)); conv_ws = A.take(conv_ws_bytes / sizeof(float));
  }
};

// the four convolutions must be the two UpsamplingConcat chains of one twin head: [feature conv1, feature conv2, depth conv1, depth conv2]
static bool neck_shape(const sf_deeplab_w* head, const sf_conv_w* convs, NeckShape* s) {
  if (!head || !convs) return false;
  s->c_hi = head->C; s->hid = head->hid; s->c_lo = convs[0].c0; s->C = convs[1].cout; s->D = convs[3].cout;
  if (s->c_hi < 4 || s->hid < 4 || head->cls.cout != 2 * s->c_hi) return false;
  for (int b = 0; b < 2; ++b) {
    const sf_conv_w &c1 = convs[2 * b], &c2 = convs[2 * b + 1];
    if (!c1.w || !c2.w || c1.c0 != s->c_lo || c1.c1 != s->c_hi || c2.c0 != c1.cout || c2.c1 != 0 || c2.cout != c1.cout) return false;
    if (c1.kh != 3 || c1.kw != 3 || c2.kh != 3 || c2.kw != 3 || c1.stride != 1 || c2.stride != 1 || c1.pad != 1 || c2.pad != 1 || c1.dil != 1 ||
        c2.dil != 1)
      return false;
  }
  return s->c_lo >= 4 && s->C >= 4 && s->D >= 4;
}

}  // namespace sf

extern "C" {

using namespace sf;

int sf_depth_softmax_planar_fwd(const float* logits_nhwc, int cs, int co, float* out_logits, float* out_prob, int rows, int D, int fHW,
                                void* stream) {
  return depth_softmax_planar(logits_nhwc, cs, co, out_logits, out_prob, rows, D, fHW, static_cast<hipStream_t>(stream));
}

size_t sf_camera_neck_ws_bytes(int c_hi, int c_lo, int C, int D, int hid, int n, int H, int W) {
  if (c_hi < 1 || c_lo < 1 || C < 1 || D < 1 || hid < 1 || n < 1 || H < 1 || W < 1) return 0;
  return layout_bytes<NeckBufs>(NeckShape{c_hi, c_lo, C, D, hid}, n, H, W);
}

int sf_camera_neck_fwd(const sf_deeplab_w* head, const sf_conv_w* convs, const float* hi, const float* lo, float* rays, float* depth_logits,
                       float* depth_prob, int n, int H, int W, float* ws, size_t ws_bytes, void* stream) {
  NeckShape s;
  if (!hi || !lo || !rays || !depth_logits || !depth_prob || n < 1 || H < 1 || W < 1 || ((uintptr_t)ws & 15) || !neck_shape(head, convs, &s))
    return SF_ERR_INVALID;
  if ((s.D % 4) || s.D > DSP_MAX_D) return SF_ERR_UNSUPPORTED;      // the last launch's refusal, before anything is written
  NeckBufs b;
  if (!carve(b, ws, ws_bytes, s, n, H, W)) return SF_ERR_WORKSPACE;
  const int twin = 2 * s.c_hi;
  const auto [head_out, up, t_feat, t_depth, d_nhwc, head_ws, conv_ws, head_ws_bytes, conv_ws_bytes] = b;
  int rc = sf_deeplab_head_fwd(head, hi, head_out, n, H, W, head_ws, head_ws_bytes, stream);
  if (rc != SF_OK) return rc;
  rc = sf_upsample_bilinear2_add_fwd(head_out, nullptr, up, n, H, W, twin, stream);
  if (rc != SF_OK) return rc;
  const int H2 = 2 * H, W2 = 2 * W;
  // cat[x, upsampled] (convolutions.py:200): in0 = the /8 endpoint, in1 = this branch's half of the upsampled twin tensor
  rc = sf_conv2d_ex_fwd(&convs[0], lo, s.c_lo, up, twin, nullptr, 0, 0, t_feat, s.C, 0, n, H2, W2, 0, conv_ws, conv_ws_bytes, stream);
  if (rc != SF_OK) return rc;
  rc = sf_conv2d_ex_fwd(&convs[2], lo, s.c_lo, up + s.c_hi, twin, nullptr, 0, 0, t_depth, s.D, 0, n, H2, W2, 0, conv_ws, conv_ws_bytes, stream);
  if (rc != SF_OK) return rc;
  rc = sf_conv2d_ex_fwd(&convs[1], t_feat, s.C, nullptr, 0, nullptr, 0, 0, rays, s.C, 0, n, H2, W2, 0, conv_ws, conv_ws_bytes, stream);
  if (rc != SF_OK) return rc;
  rc = sf_conv2d_ex_fwd(&convs[3], t_depth, s.D, nullptr, 0, nullptr, 0, 0, d_nhwc, s.D, 0, n, H2, W2, 0, conv_ws, conv_ws_bytes, stream);
  if (rc != SF_OK) return rc;
  return depth_softmax_planar(d_nhwc, s.D, 0, depth_logits, depth_prob, n, s.D, H2 * W2, static_cast<hipStream_t>(stream));
}

}  // extern "C"
