// Evaluation-side kernels for gfx950 + C ABI: the per-pixel parts of
// streamingflow/metrics.py and streamingflow/utils/instance.py.  Integer / index work: results are exact.
//   sf_confusion_fwd          joint histogram of two label maps (IntersectionOverUnion's stat scores,
//                             PanopticMetric's bincount of prediction + K * target, metrics.py:37, :171-176)
//   sf_instance_centers_fwd   find_instance_centers (instance.py:80-92): threshold, 3x3 max-pool NMS, and the
//                             row-major list torch.nonzero returns (flags + exclusive scan + compaction)
//   sf_group_pixels_fwd       group_pixels + foreground mask (instance.py:95-116, :136-137): nearest centre of
//                             (pixel + offset), first minimum on ties
//   sf_instance_moments_fwd   per (frame, instance) pixel counts and position sums, plain and flow-warped — the masked means
//                             of make_instance_id_temporally_consistent (instance.py:213-236), all frames in one launch,
//                             integer atomics only (order-independent)
//   sf_confusion_frames_fwd   the joint histogram per frame of a whole label sequence in one launch
//   sf_instance_seq_fwd       centres, grouping and consecutive ids (get_instance_segmentation_and_centers, instance.py:119-144)
//                             of a whole sequence of frames: a fixed number of launches, nothing read back by the host
//   sf_instance_labels_fwd    convert_instance_mask_to_center_and_offset_label (instance.py:12-77): centerness, centre offsets and
//                             future displacements of B sequences of T instance maps: one moments launch (plain + ego-warped), one
//                             label launch, nothing read back by the host
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <cstring>

#include <rocprim/device/device_scan.hpp>

#include "../../include/sfnative.h"

namespace sf {

__global__ void confusion_kernel(const long long* __restrict__ a, const long long* __restrict__ b, long n, int K,
                                 unsigned long long* __restrict__ out, int* __restrict__ bad) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long long x = a[i], y = b[i];
    if (x < 0 || x >= K || y < 0 || y >= K) { *bad = 1; continue; }
    atomicAdd(out + (size_t)y * K + x, 1ULL);
  }
}

// keep[i][j] = thresholded value is a strict-positive local maximum of its 3x3 neighbourhood
__global__ void center_flag_kernel(const float* __restrict__ c, int H, int W, float thr, int* __restrict__ flag) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= H * W) return;
  const int i = idx / W, j = idx - i * W;
  auto val = [&](int y, int x) -> float {
    if (y < 0 || y >= H || x < 0 || x >= W) return -INFINITY;       // max_pool2d pads with -inf
    const float v = c[y * W + x];
    return v > thr ? v : -1.f;                                       // F.threshold(x, thr, -1)
  };
  const float v = val(i, j);
  float m = v;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) m = fmaxf(m, val(i + dy, j + dx));
  flag[idx] = (v == m && v > 0.f) ? 1 : 0;
}

__global__ void center_compact_kernel(const int* __restrict__ flag, const int* __restrict__ scan, int H, int W, int cap,
                                      int* __restrict__ centers, int* __restrict__ n_out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = H * W;
  if (idx == 0) n_out[0] = scan[n - 1] + flag[n - 1];
  if (idx >= n || !flag[idx]) return;
  const int r = scan[idx];
  if (r >= cap) return;
  centers[2 * r] = idx / W;
  centers[2 * r + 1] = idx % W;
}

__global__ void group_pixels_kernel(const int* __restrict__ centers, int nc, const float* __restrict__ off, const unsigned char* __restrict__ fg,
                                    int H, int W, long long* __restrict__ inst) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= H * W) return;
  const int i = idx / W, j = idx - i * W;
  const float lx = __fadd_rn((float)i, off[idx]), ly = __fadd_rn((float)j, off[H * W + idx]);
  float best = INFINITY;
  int arg = 0;
  for (int k = 0; k < nc; ++k) {
    const float dx = __fsub_rn((float)centers[2 * k], lx), dy = __fsub_rn((float)centers[2 * k + 1], ly);
    const float d = __fsqrt_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
    if (d < best) { best = d; arg = k; }
  }
  inst[idx] = fg[idx] ? (long long)(arg + 1) : 0LL;
}

// Per (frame, instance id) pixel count, exact integer sums of (row, col) and sums of the flow-warped position
// (row + flow0, col + flow1) in 2^-20 fixed point.  Integer atomics only: the result does not depend on the order the
// pixels arrive in (bitwise reproducible), unlike a floating-point atomicAdd.
constexpr double MOMENT_FX = 1048576.0;
__global__ void instance_moments_kernel(const long long* __restrict__ inst, const float* __restrict__ flow, int F, int H, int W, int max_id,
                                        unsigned long long* __restrict__ pos, unsigned long long* __restrict__ warped, int* __restrict__ cnt) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long plane = (long)H * W;
  if (idx >= F * plane) return;
  const int f = (int)(idx / plane);
  const int pix = (int)(idx - f * plane);
  const long long id = inst[idx];
  if (id <= 0 || id > max_id) return;
  const int i = pix / W, j = pix - i * W;
  const size_t slot = (size_t)f * (max_id + 1) + (size_t)id;
  atomicAdd(pos + 2 * slot, (unsigned long long)i);
  atomicAdd(pos + 2 * slot + 1, (unsigned long long)j);
  atomicAdd(cnt + slot, 1);
  if (warped) {
    const float* fl = flow + (size_t)f * 2 * plane;
    const float x = __fadd_rn((float)i, fl[pix]), y = __fadd_rn((float)j, fl[plane + pix]);
    // two's complement: adding the unsigned image of a negative fixed-point value is the signed add
    atomicAdd(warped + 2 * slot, (unsigned long long)llrint((double)x * MOMENT_FX));
    atomicAdd(warped + 2 * slot + 1, (unsigned long long)llrint((double)y * MOMENT_FX));
  }
}

// joint histograms of F label-map pairs of n elements each: out[f][b][a] (labels outside [0, K) set *bad)
__global__ void confusion_frames_kernel(const long long* __restrict__ a, const long long* __restrict__ b, long n, int F, int K,
                                        unsigned long long* __restrict__ out, int* __restrict__ bad) {
  const long total = n * F;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long long x = a[i], y = b[i];
    if (x < 0 || x >= K || y < 0 || y >= K) { *bad = 1; continue; }
    const long f = i / n;
    // in BEV instance maps > 95 % of the pixels are (background, background): the lanes of a wave that hold that pair for
    // the same frame as the first of them add ONE ballot count instead of up to 64 atomics on one address (integer adds:
    // the result does not depend on who adds)
    const bool bg = (x == 0) & (y == 0);
    const unsigned long long m = __ballot(bg);
    bool done = false;
    if (m) {
      const int leader = __ffsll((long long)m) - 1;
      const long fl = __shfl(f, leader);
      const unsigned long long same = __ballot(bg && f == fl);
      if (bg && f == fl) {
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(out + (size_t)f * K * K, (unsigned long long)__popcll(same));
        done = true;
      }
    }
    if (!done) atomicAdd(out + ((size_t)f * K + (size_t)y) * K + x, 1ULL);
  }
}

// ---- the same post-processing for F frames [F][H][W] at once (sf_instance_seq_fwd) -------------------------------------------
// One flag / scan / compaction over all F*H*W pixels: a centre's rank within its frame is its scan value minus the scan value of
// the frame's first pixel, so each frame fills its own [cap][2] table and an overflowing frame never reaches the next one.
__global__ void seq_center_flag_kernel(const float* __restrict__ c, int F, int H, int W, float thr, int* __restrict__ flag) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int plane = H * W;
  if (idx >= (long)F * plane) return;
  const int f = (int)(idx / plane), pix = (int)(idx - (long)f * plane);
  const int i = pix / W, j = pix - i * W;
  const float* cf = c + (size_t)f * plane;
  auto val = [&](int y, int x) -> float {
    if (y < 0 || y >= H || x < 0 || x >= W) return -INFINITY;       // max_pool2d pads with -inf
    const float v = cf[y * W + x];
    return v > thr ? v : -1.f;                                       // F.threshold(x, thr, -1)
  };
  const float v = val(i, j);
  float m = v;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) m = fmaxf(m, val(i + dy, j + dx));
  flag[idx] = (v == m && v > 0.f) ? 1 : 0;
}

__global__ void seq_center_compact_kernel(const int* __restrict__ flag, const int* __restrict__ scan, int F, int H, int W, int cap,
                                          int* __restrict__ centers, int* __restrict__ n_out) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int plane = H * W;
  if (idx >= (long)F * plane) return;
  const int f = (int)(idx / plane), pix = (int)(idx - (long)f * plane);
  const int base = scan[(size_t)f * plane];
  if (pix == plane - 1) n_out[f] = scan[idx] + flag[idx] - base;   // uncapped
  if (!flag[idx]) return;
  const int r = scan[idx] - base;
  if (r >= cap) return;
  int* row = centers + ((size_t)f * cap + r) * 2;
  row[0] = pix / W;
  row[1] = pix % W;
}

// group_pixels_kernel per frame: a workgroup serves 256 pixels of ONE frame and walks that frame's min(n, cap) centres through LDS
// in pieces of SEQ_CHUNK (ascending, so the first minimum still wins ties).  Also marks which raw ids 0..cap the frame holds.
constexpr int SEQ_CHUNK = 128;
__global__ void seq_group_pixels_kernel(const int* __restrict__ centers, const int* __restrict__ n_centers, int cap, const float* __restrict__ off,
                                        const unsigned char* __restrict__ fg, int H, int W, int blocks_per_frame,
                                        long long* __restrict__ inst, int* __restrict__ present) {
  __shared__ int tab[2 * SEQ_CHUNK];
  const int f = blockIdx.x / blocks_per_frame;
  const int plane = H * W;
  const int pix = (blockIdx.x - f * blocks_per_frame) * blockDim.x + threadIdx.x;
  const bool live = pix < plane;
  const int nc = min(n_centers[f], cap);
  const int* table = centers + (size_t)f * cap * 2;
  const float* of = off + (size_t)f * 2 * plane;
  const int i = pix / W, j = pix - i * W;
  float lx = 0.f, ly = 0.f;
  if (live) { lx = __fadd_rn((float)i, of[pix]); ly = __fadd_rn((float)j, of[plane + pix]); }
  float best = INFINITY;
  int arg = 0;
  for (int k0 = 0; k0 < nc; k0 += SEQ_CHUNK) {       // nc is uniform over the workgroup: every thread reaches the barriers
    const int m = min(SEQ_CHUNK, nc - k0);
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * m; e += blockDim.x) tab[e] = table[2 * k0 + e];
    __syncthreads();
    for (int k = 0; k < m; ++k) {
      const float dx = __fsub_rn((float)tab[2 * k], lx), dy = __fsub_rn((float)tab[2 * k + 1], ly);
      const float d = __fsqrt_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
      if (d < best) { best = d; arg = k0 + k; }
    }
  }
  if (!live) return;
  const int id = (nc > 0 && fg[(size_t)f * plane + pix]) ? arg + 1 : 0;     // a frame without centres is all background
  inst[(size_t)f * plane + pix] = (long long)id;
  present[(size_t)f * (cap + 1) + id] = 1;                                  // every writer stores the same value
}

// lut[f][v] = number of present values of frame f smaller than v (make_instance_seg_consecutive: the inverse index of a sorted
// unique; a frame without background pixels has present[0] == 0, so its first instance becomes 0, as in the reference).
// One workgroup of 256 per frame, 256 values per round: ballot prefix inside a wave, wave totals through LDS.
__global__ void seq_lut_kernel(const int* __restrict__ present, int cap, int* __restrict__ lut) {
  __shared__ int wave_sum[4];
  const int f = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int* p = present + (size_t)f * (cap + 1);
  int* l = lut + (size_t)f * (cap + 1);
  int carry = 0;
  for (int v0 = 0; v0 <= cap; v0 += 256) {
    const int v = v0 + threadIdx.x;
    const bool on = v <= cap && p[v] != 0;
    const unsigned long long b = __ballot(on);
    const int before = __popcll(b & ((1ULL << lane) - 1ULL));
    __syncthreads();
    if (lane == 0) wave_sum[wave] = __popcll(b);
    __syncthreads();
    int prior = carry, total = 0;
    for (int w = 0; w < 4; ++w) {
      if (w < wave) prior += wave_sum[w];
      total += wave_sum[w];
    }
    if (v <= cap) l[v] = prior + before;
    carry += total;
  }
}

__global__ void seq_relabel_kernel(const int* __restrict__ lut, int cap, long plane, long total, long long* __restrict__ inst) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const long f = idx / plane;
  inst[idx] = (long long)lut[f * (cap + 1) + inst[idx]];
}

// warp_features (utils/geometry.py:196-236): affine_grid(theta, align_corners=False) + grid_sample(mode, zeros
// padding, align_corners=False) on NCHW maps.  theta [b][6] row major (2 x 3).
//   base grid   x_j = (2j + 1)/W - 1,  y_i = (2i + 1)/H - 1
//   source      gx = t0*x + t1*y + t2, gy = t3*x + t4*y + t5;  ix = ((gx + 1)*W - 1)/2, iy likewise
//   nearest     index = nearbyint(ix) (ties to even), zero when outside; bilinear: 4 taps, zeros outside
// The source position (in pixels) of destination pixel (i, j) under the 2x3 matrix t: the ONE statement of this arithmetic, shared by
// warp_affine_kernel and the warped half of instance_label_moments_kernel, which must pick the same source pixel bit for bit.
// Which multiply-adds are fused is therefore written out and the compiler's own contraction is off in here (left to it, the same
// expression came out fused in one kernel and unfused in the other); the fused ones are those warp_affine_kernel has always run.
__device__ __forceinline__ void warp_source(const float* __restrict__ t, int i, int j, int H, int W, float& ix, float& iy) {
#pragma clang fp contract(off)
  const float xs = (2.f * j + 1.f) / (float)W - 1.f, ys = (2.f * i + 1.f) / (float)H - 1.f;      // 2j + 1 is exact either way
  const float gx = fmaf(t[0], xs, t[1] * ys) + t[2];
  const float gy = fmaf(t[3], xs, t[4] * ys) + t[5];
  ix = fmaf(gx + 1.f, (float)W, -1.f) * 0.5f;
  iy = fmaf(gy + 1.f, (float)H, -1.f) * 0.5f;
}

__global__ void warp_affine_kernel(const float* __restrict__ x, const float* __restrict__ theta, int B, int C, int H, int W, int bilinear,
                                   float* __restrict__ out) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * H * W) return;
  const int j = (int)(idx % W);
  const long r = idx / W;
  const int i = (int)(r % H), b = (int)(r / H);
  float ix, iy;
  warp_source(theta + 6 * b, i, j, H, W, ix, iy);
  const size_t plane = (size_t)H * W;
  const float* xb = x + (size_t)b * C * plane;
  float* ob = out + (size_t)b * C * plane + (size_t)i * W + j;
  if (!bilinear) {
    const float fx = nearbyintf(ix), fy = nearbyintf(iy);
    const bool ok = fx >= 0.f && fx < (float)W && fy >= 0.f && fy < (float)H;
    const size_t src = ok ? (size_t)((int)fy) * W + (int)fx : 0;
    for (int c = 0; c < C; ++c) ob[c * plane] = ok ? xb[c * plane + src] : 0.f;
    return;
  }
  const float x0f = floorf(ix), y0f = floorf(iy);
  const int x0 = (int)x0f, y0 = (int)y0f, x1 = x0 + 1, y1 = y0 + 1;
  const float wx1 = ix - x0f, wy1 = iy - y0f, wx0 = 1.f - wx1, wy0 = 1.f - wy1;
  auto in = [&](int yy, int xx) { return yy >= 0 && yy < H && xx >= 0 && xx < W; };
  for (int c = 0; c < C; ++c) {
    const float* pc = xb + c * plane;
    float v = 0.f;
    if (in(y0, x0)) v += pc[(size_t)y0 * W + x0] * (wx0 * wy0);
    if (in(y0, x1)) v += pc[(size_t)y0 * W + x1] * (wx1 * wy0);
    if (in(y1, x0)) v += pc[(size_t)y1 * W + x0] * (wx0 * wy1);
    if (in(y1, x1)) v += pc[(size_t)y1 * W + x1] * (wx1 * wy1);
    ob[c * plane] = v;
  }
}

// ---- ground-truth labels from instance maps (sf_instance_labels_fwd): convert_instance_mask_to_center_and_offset_label ---------
// Pass 1.  Per (frame, id in 1..K): pixel count and integer sums of (row, col), of the frame as it is ("plain") and of the frame
// resampled by theta[f] with nearest-neighbour sampling ("warped").  The warped half never writes a warped map: a thread owns
// DESTINATION pixel (i, j), looks its source pixel up exactly as warp_affine_kernel's nearest branch does (warp_source, then
// nearbyint and the range test) and adds (i, j) to the moments of the id it finds there.  Integer atomics only (the sums do not
// depend on the arrival order); ids outside 1..K are background and issue none.
__global__ void instance_label_moments_kernel(const long long* __restrict__ inst, const float* __restrict__ theta, int F, int H, int W, int K,
                                              int* __restrict__ cnt, unsigned long long* __restrict__ pos, int* __restrict__ wcnt,
                                              unsigned long long* __restrict__ wpos) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long plane = (long)H * W;
  if (idx >= F * plane) return;
  const int f = (int)(idx / plane);
  const int pix = (int)(idx - f * plane);
  const int i = pix / W, j = pix - i * W;
  const long long* frame = inst + (size_t)f * plane;
  const size_t row = (size_t)f * ((size_t)K + 1);
  const long long id = frame[pix];
  if (id >= 1 && id <= K) {
    atomicAdd(pos + 2 * (row + id), (unsigned long long)i);
    atomicAdd(pos + 2 * (row + id) + 1, (unsigned long long)j);
    atomicAdd(cnt + row + id, 1);
  }
  float ix, iy;
  warp_source(theta + 6 * (size_t)f, i, j, H, W, ix, iy);
  const float fx = nearbyintf(ix), fy = nearbyintf(iy);
  const bool ok = fx >= 0.f && fx < (float)W && fy >= 0.f && fy < (float)H;
  if (!ok) return;                                                    // zeros padding: background
  const long long wid = frame[(size_t)((int)fy) * W + (int)fx];
  if (wid >= 1 && wid <= K) {
    atomicAdd(wpos + 2 * (row + wid), (unsigned long long)i);
    atomicAdd(wpos + 2 * (row + wid) + 1, (unsigned long long)j);
    atomicAdd(wcnt + row + wid, 1);
  }
}

// x[mask].mean().round() of the reference: the fp32 sum of integer coordinates is exact while it stays below 2^24 (every grid
// up to 256 x 256), one fp32 division, round half to even.
__device__ __forceinline__ float moment_centre(unsigned long long sum, int count) { return rintf(__fdiv_rn((float)sum, (float)count)); }

// Pass 2.  A workgroup serves 256 pixels of ONE frame.  It builds the frame's instance table in LDS from the moments, LABEL_CHUNK
// ids at a time (K is not bounded by LDS): presence, centre, and — when the instance is also in the next frame of its sequence and
// its warped mask there is not empty — the displacement warped centre(t + 1) - centre(t).  Every thread then walks the chunk with
// the same index (LDS broadcasts) for the smallest squared distance to a centre, exact in integers; a pixel whose own id falls
// into the chunk picks its offset and flow from its entry.  max_k exp(-d_k^2 / sigma^2) = exp(-min_k d_k^2 / sigma^2): one fp32
// division and one exp per pixel, unfused, on the operands the reference has.
constexpr int LABEL_CHUNK = 128;
struct LabelEntry {
  int present, xc, yc, moves;
  float dx, dy;
};
__global__ void instance_label_kernel(const long long* __restrict__ inst, const int* __restrict__ cnt, const unsigned long long* __restrict__ pos,
                                      const int* __restrict__ wcnt, const unsigned long long* __restrict__ wpos, int T, int H, int W, int K,
                                      int blocks_per_frame, float sigma_sq, float ignore, float* __restrict__ center, float* __restrict__ offset,
                                      float* __restrict__ flow) {
  __shared__ LabelEntry tab[LABEL_CHUNK];
  const int f = blockIdx.x / blocks_per_frame;
  const int plane = H * W;
  const int pix = (blockIdx.x - f * blocks_per_frame) * blockDim.x + threadIdx.x;
  const bool live = pix < plane;
  const int i = pix / W, j = pix - i * W;
  const bool has_next = (f % T) < T - 1;                              // frame f + 1 belongs to the same sequence
  const size_t row = (size_t)f * ((size_t)K + 1), next = row + (size_t)K + 1;
  const long long own = live ? inst[(size_t)f * plane + pix] : 0LL;
  int best = INT_MAX;
  bool any = false;
  float ox = ignore, oy = ignore, fx = ignore, fy = ignore;
  for (int k0 = 0; k0 < K; k0 += LABEL_CHUNK) {                       // K is uniform over the workgroup: every thread reaches the barriers
    const int m = min(LABEL_CHUNK, K - k0);
    __syncthreads();
    if ((int)threadIdx.x < m) {
      const size_t id = (size_t)k0 + 1 + threadIdx.x;
      LabelEntry e = {0, 0, 0, 0, 0.f, 0.f};
      const int n = cnt[row + id];
      if (n > 0) {
        e.present = 1;
        e.xc = (int)moment_centre(pos[2 * (row + id)], n);
        e.yc = (int)moment_centre(pos[2 * (row + id) + 1], n);
        if (has_next && cnt[next + id] > 0) {
          const int wn = wcnt[next + id];
          if (wn > 0) {
            e.moves = 1;
            e.dx = __fsub_rn(moment_centre(wpos[2 * (next + id)], wn), (float)e.xc);
            e.dy = __fsub_rn(moment_centre(wpos[2 * (next + id) + 1], wn), (float)e.yc);
          }
        }
      }
      tab[threadIdx.x] = e;
    }
    __syncthreads();
    for (int k = 0; k < m; ++k) {
      if (!tab[k].present) continue;                                  // uniform: no lane diverges here
      const int dx = tab[k].xc - i, dy = tab[k].yc - j;
      best = min(best, dx * dx + dy * dy);
      any = true;
    }
    const long long mine = own - 1 - k0;
    if (mine >= 0 && mine < m) {                                      // the pixel itself makes its instance present
      const LabelEntry e = tab[(int)mine];
      ox = (float)(e.xc - i);
      oy = (float)(e.yc - j);
      if (e.moves) { fx = e.dx; fy = e.dy; }
    }
  }
  if (!live) return;
  const size_t o1 = (size_t)f * plane + pix, o2 = (size_t)f * 2 * plane + pix;
  center[o1] = any ? expf(-__fdiv_rn((float)best, sigma_sq)) : 0.f;
  offset[o2] = ox;
  offset[o2 + plane] = oy;
  flow[o2] = fx;
  flow[o2 + plane] = fy;
}

inline size_t a256e(size_t n) { return (n + 255) & ~size_t(255); }

}  // namespace sf

using namespace sf;

extern "C" {

int sf_confusion_fwd(const int64_t* a, const int64_t* b, long n, int K, int64_t* out, int32_t* bad, void* stream) {
  if (!out || !bad || K < 1 || n < 0) return SF_ERR_INVALID;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(out, 0, (size_t)K * K * sizeof(int64_t), st) != hipSuccess) return SF_ERR_LAUNCH;
  if (hipMemsetAsync(bad, 0, sizeof(int32_t), st) != hipSuccess) return SF_ERR_LAUNCH;
  if (n == 0) return SF_OK;
  if (!a || !b) return SF_ERR_INVALID;
  long blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(confusion_kernel, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<const long long*>(a),
                     reinterpret_cast<const long long*>(b), n, K, reinterpret_cast<unsigned long long*>(out), bad);
  return hipGetLastError() == hipSuccess ? SF_OK : SF_ERR_LAUNCH;
}

size_t sf_instance_centers_ws_bytes(int H, int W) {
  if (H < 1 || W < 1) return 0;
  size_t tb = 0;
  (void)rocprim::exclusive_scan(nullptr, tb, (const int*)nullptr, (int*)nullptr, 0, (size_t)H * W, rocprim::plus<int>(), nullptr);
  return 2 * a256e((size_t)H * W * 4) + a256e(tb) + 256;
}

int sf_instance_centers_fwd(const float* center, int H, int W, float conf_threshold, int32_t* centers, int cap, int32_t* n_centers,
                            void* ws, size_t ws_bytes, void* stream) {
  if (!center || !centers || !n_centers || H < 1 || W < 1 || cap < 1 || !ws) return SF_ERR_INVALID;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t n = (size_t)H * W, a = a256e(n * 4);
  size_t tb = 0;
  (void)rocprim::exclusive_scan(nullptr, tb, (const int*)nullptr, (int*)nullptr, 0, n, rocprim::plus<int>(), st);
  if (ws_bytes < 2 * a + a256e(tb)) return SF_ERR_WORKSPACE;
  char* p = static_cast<char*>(ws);
  int* flag = reinterpret_cast<int*>(p);
  int* scan = reinterpret_cast<int*>(p + a);
  void* tmp = p + 2 * a;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipLaunchKernelGGL(center_flag_kernel, grid, block, 0, st, center, H, W, conf_threshold, flag);
  if (rocprim::exclusive_scan(tmp, tb, (const int*)flag, scan, 0, n, rocprim::plus<int>(), st) != hipSuccess) return SF_ERR_LAUNCH;
  hipLaunchKernelGGL(center_compact_kernel, grid, block, 0, st, flag, scan, H, W, cap, centers, n_centers);
  return hipGetLastError() == hipSuccess ? SF_OK : SF_ERR_LAUNCH;
}

int sf_group_pixels_fwd(const int32_t* centers, int n_centers, const float* offsets, const uint8_t* foreground, int H, int W,
                        int64_t* instance, void* stream) {
  if (!centers || !offsets || !foreground || !instance || n_centers < 1 || H < 1 || W < 1) return SF_ERR_INVALID;
  hipLaunchKernelGGL(group_pixels_kernel, dim3((H * W + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), centers, n_centers,
                     offsets, foreground, H, W, reinterpret_cast<long long*>(instance));
  return hipGetLastError() == hipSuccess ? SF_OK : SF_ERR_LAUNCH;
}

// workspace of sf_instance_seq_fwd: flags, scan (F*H*W ints each), rocPRIM's scan storage, present and lut ((cap + 1) ints per frame each).
// The one place the sizes are checked and the layout is laid out: both entry points below go through it.
struct SeqLayout {
  size_t n, tab, a, at, tb, total;
  int bpf;      // workgroups of 256 pixels per frame
};
static bool seq_layout(int F, int H, int W, int cap, hipStream_t st, SeqLayout* L) {
  if (F < 1 || H < 1 || W < 1 || cap < 1) return false;
  L->n = (size_t)F * H * W;
  L->tab = (size_t)F * ((size_t)cap + 1);
  if (L->n >= (size_t(1) << 31) || L->tab >= (size_t(1) << 31)) return false;
  L->bpf = (int)(((size_t)H * W + 255) / 256);
  // the grouping launch pads every frame to whole workgroups: its thread count has to stay a 32-bit number too
  if ((size_t)F * L->bpf * 256 >= (size_t(1) << 32)) return false;
  L->a = a256e(L->n * 4);
  L->at = a256e(L->tab * 4);
  size_t tb = 0;
  (void)rocprim::exclusive_scan(nullptr, tb, (const int*)nullptr, (int*)nullptr, 0, L->n, rocprim::plus<int>(), st);
  L->tb = a256e(tb);
  L->total = 2 * L->a + L->tb + 2 * L->at;
  return true;
}

size_t sf_instance_seq_ws_bytes(int F, int H, int W, int cap) {
  SeqLayout L;
  return seq_layout(F, H, W, cap, nullptr, &L) ? L.total : 0;
}

int sf_instance_seq_fwd(const float* center, const float* offsets, const uint8_t* foreground, int F, int H, int W, float conf_threshold,
                        int cap, int32_t* centers, int32_t* n_centers, int64_t* instance, void* ws, size_t ws_bytes, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  SeqLayout L;
  if (!center || !offsets || !foreground || !centers || !n_centers || !instance || !ws || !seq_layout(F, H, W, cap, st, &L))
    return SF_ERR_INVALID;
  if (ws_bytes < L.total) return SF_ERR_WORKSPACE;
  const size_t n = L.n, tab = L.tab, a = L.a, at = L.at, tb = L.tb;
  char* p = static_cast<char*>(ws);
  int* flag = reinterpret_cast<int*>(p);
  int* scan = reinterpret_cast<int*>(p + a);
  void* tmp = p + 2 * a;
  int* present = reinterpret_cast<int*>(p + 2 * a + tb);
  int* lut = reinterpret_cast<int*>(p + 2 * a + tb + at);
  // rows of the centre tables past a frame's count stay zero: the outputs are a function of the inputs alone
  if (hipMemsetAsync(centers, 0, (size_t)F * cap * 2 * sizeof(int32_t), st) != hipSuccess) return SF_ERR_LAUNCH;
  if (hipMemsetAsync(present, 0, tab * sizeof(int), st) != hipSuccess) return SF_ERR_LAUNCH;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipLaunchKernelGGL(seq_center_flag_kernel, grid, block, 0, st, center, F, H, W, conf_threshold, flag);
  size_t scan_bytes = tb;
  if (rocprim::exclusive_scan(tmp, scan_bytes, (const int*)flag, scan, 0, n, rocprim::plus<int>(), st) != hipSuccess) return SF_ERR_LAUNCH;
  hipLaunchKernelGGL(seq_center_compact_kernel, grid, block, 0, st, flag, scan, F, H, W, cap, centers, n_centers);
  const int bpf = L.bpf;
  hipLaunchKernelGGL(seq_group_pixels_kernel, dim3((unsigned)((size_t)F * bpf)), block, 0, st, centers, n_centers, cap, offsets, foreground,
                     H, W, bpf, reinterpret_cast<long long*>(instance), present);
  hipLaunchKernelGGL(seq_lut_kernel, dim3((unsigned)F), block, 0, st, present, cap, lut);
  hipLaunchKernelGGL(seq_relabel_kernel, grid, block, 0, st, lut, cap, (long)H * W, (long)n, reinterpret_cast<long long*>(instance));
  return hipGetLastError() == hipSuccess ? SF_OK : SF_ERR_LAUNCH;
}

// workspace of sf_instance_labels_fwd, F = B*T frames, n = F * (K + 1) slots (slot = frame * (K + 1) + id; the slots of id 0 stay zero),
// every part starting on a multiple of 256 bytes:
//   plain counts  int32 [n] | plain (row, col) sums  int64 [n][2] | warped counts  int32 [n] | warped (row, col) sums  int64 [n][2]
struct LabelLayout {
  size_t n, ac, as, total;      // slots, bytes of a count part, bytes of a sum part
  int F, bpf;                   // frames, workgroups of 256 pixels per frame
};
static bool label_layout(int B, int T, int H, int W, int K, LabelLayout* L) {
  if (B < 1 || T < 1 || H < 1 || W < 1 || K < 0 || K >= (1 << 24) || H > 32768 || W > 32768) return false;
  const size_t frames = (size_t)B * T;
  L->n = frames * ((size_t)K + 1);
  if (frames * H * W >= (size_t(1) << 31) || L->n >= (size_t(1) << 31)) return false;
  L->F = (int)frames;
  L->bpf = (int)(((size_t)H * W + 255) / 256);
  if (frames * L->bpf * 256 >= (size_t(1) << 32)) return false;      // the label launch pads every frame to whole workgroups
  L->ac = a256e(L->n * sizeof(int32_t));
  L->as = a256e(L->n * 2 * sizeof(int64_t));
  L->total = 2 * (L->ac + L->as);
  return true;
}

size_t sf_instance_labels_ws_bytes(int B, int T, int H, int W, int num_instances) {
  LabelLayout L;
  return label_layout(B, T, H, W, num_instances, &L) ? L.total : 0;
}

int sf_instance_labels_fwd(const int64_t* instance, const float* theta, int B, int T, int H, int W, int num_instances, double sigma,
                           float ignore_index, float* center, float* offset, float* flow, void* ws, size_t ws_bytes, void* stream) {
  LabelLayout L;
  if (!instance || !theta || !center || !offset || !flow || !ws || !(sigma > 0.0) || !label_layout(B, T, H, W, num_instances, &L))
    return SF_ERR_INVALID;
  if (ws_bytes < L.total) return SF_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* p = static_cast<char*>(ws);
  int* cnt = reinterpret_cast<int*>(p);
  unsigned long long* pos = reinterpret_cast<unsigned long long*>(p + L.ac);
  int* wcnt = reinterpret_cast<int*>(p + L.ac + L.as);
  unsigned long long* wpos = reinterpret_cast<unsigned long long*>(p + 2 * L.ac + L.as);
  if (hipMemsetAsync(ws, 0, L.total, st) != hipSuccess) return SF_ERR_LAUNCH;
  const long long* ids = reinterpret_cast<const long long*>(instance);
  const size_t pixels = (size_t)L.F * H * W;
  hipLaunchKernelGGL(instance_label_moments_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, st, ids, theta, L.F, H, W,
                     num_instances, cnt, pos, wcnt, wpos);
  // sigma ** 2 of the reference is a Python number (double) that torch divides by in fp32
  hipLaunchKernelGGL(instance_label_kernel, dim3((unsigned)((size_t)L.F * L.bpf)), dim3(256), 0, st, ids, cnt, pos, wcnt, wpos, T, H, W,
                     num_instances, L.bpf, (float)(sigma * sigma), ignore_index, center, offset, flow);
  return hipGetLastError() == hipSuccess ? SF_OK : SF_ERR_LAUNCH;
}

int sf_instance_moments_fwd(const int64_t* instance, const float* flow, int F, int H, int W, int max_id, int64_t* pos_sums,
                            int64_t* warped_fx, int32_t* counts, void* stream) {
  if (!instance || !pos_sums || !counts || F < 1 || H < 1 || W < 1 || max_id < 0 || (warped_fx && !flow)) return SF_ERR_INVALID;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t slots = (size_t)F * (max_id + 1);
  if (hipMemsetAsync(pos_sums, 0, slots * 2 * sizeof(int64_t), st) != hipSuccess) return SF_ERR_LAUNCH;
  if (warped_fx && hipMemsetAsync(warped_fx, 0, slots * 2 * sizeof(int64_t), st) != hipSuccess) return SF_ERR_LAUNCH;
  if (hipMemsetAsync(counts, 0, slots * sizeof(int32_t), st) != hipSuccess) return SF_ERR_LAUNCH;
  const long total = (long)F * H * W;
  hipLaunchKernelGGL(instance_moments_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                     reinterpret_cast<const long long*>(instance), flow, F, H, W, max_id, reinterpret_cast<unsigned long long*>(pos_sums),
                     reinterpret_cast<unsigned long long*>(warped_fx), counts);
  return hipGetLastError() == hipSuccess ? SF_OK : SF_ERR_LAUNCH;
}

int sf_confusion_frames_fwd(const int64_t* a, const int64_t* b, long n_per_frame, int F, int K, int64_t* out, int32_t* bad, void* stream) {
  if (!out || !bad || K < 1 || F < 1 || n_per_frame < 0) return SF_ERR_INVALID;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(out, 0, (size_t)F * K * K * sizeof(int64_t), st) != hipSuccess) return SF_ERR_LAUNCH;
  if (hipMemsetAsync(bad, 0, sizeof(int32_t), st) != hipSuccess) return SF_ERR_LAUNCH;
  if (n_per_frame == 0) return SF_OK;
  if (!a || !b) return SF_ERR_INVALID;
  long blocks = (n_per_frame * F + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(confusion_frames_kernel, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<const long long*>(a),
                     reinterpret_cast<const long long*>(b), n_per_frame, F, K, reinterpret_cast<unsigned long long*>(out), bad);
  return hipGetLastError() == hipSuccess ? SF_OK : SF_ERR_LAUNCH;
}

int sf_warp_affine_fwd(const float* x, const float* theta, int B, int C, int H, int W, int bilinear, float* out, void* stream) {
  if (!x || !theta || !out || B < 1 || C < 1 || H < 1 || W < 1) return SF_ERR_INVALID;
  const long total = (long)B * H * W;
  hipLaunchKernelGGL(warp_affine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x, theta, B,
                     C, H, W, bilinear, out);
  return hipGetLastError() == hipSuccess ? SF_OK : SF_ERR_LAUNCH;
}

}  // extern "C"
