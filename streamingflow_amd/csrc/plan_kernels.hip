// The planner for gfx950: the stage after the decoder's heads.
//   sf_plan_cost_fwd            Cost_Function.forward (streamingflow/cost.py:25-46): the seven cost terms of all B x N sampled trajectories
//   sf_plan_select_refine_fwd   Planning.select + the GRU refinement loop (streamingflow/models/planning_model.py:47-64, :129-145)
//   sf_plan_metric_fwd          PlanningMetric.update (streamingflow/metrics.py:292-389)
// The arithmetic that decides a grid cell is the reference's, operation for operation: IEEE divisions (no reciprocals), truncation
// towards zero, the additions in the reference's order, and no fused multiply-adds (the compiler's contraction is switched off in
// plan_cost_kernel and plan_metric_kernel; torch on the host contracts nothing.  plan_select_refine_kernel decides no cell: its dot
// products may contract and are held to the refinement tolerance).  The build passes no fast-math flag, so `/` and sqrtf are the correctly
// rounded ones (hipcc's -fhip-fp32-correctly-rounded-divide-sqrt default).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/sfnative.h"

namespace sf {
namespace {

constexpr int WAVE = 64;
constexpr int COST_WAVES = 4;         // trajectories per workgroup of plan_cost_kernel
constexpr int REFINE_THREADS = 1024;  // one workgroup per sample: 16 waves share the rows of the GRU's matrices
constexpr int MAX_STATE = 256;

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = WAVE / 2; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = WAVE / 2; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = WAVE / 2; o; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  return v;
}

// .long() then clamp(0, G - 1): truncation towards zero sends (-1, 0) to cell 0 like every negative value, so clamping the float first
// selects the same cell and cannot overflow the conversion (NaN -> 0)
__device__ __forceinline__ int cell(float v, int G) { return !(v > 0.f) ? 0 : (v >= (float)(G - 1) ? G - 1 : (int)v); }
__device__ __forceinline__ int cell(double v, int G) { return !(v > 0.0) ? 0 : (v >= (double)(G - 1) ? G - 1 : (int)v); }
__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

struct PlanCostArgs {
  const float* trajs;
  long stride;
  const float* cost_volume;
  const uint8_t* occ;
  const float* lane;
  const float* drv;
  const float* target;
  const int32_t* rc0;
  const int32_t* rcl;
  const float* dx;
  const float* bx;
  const float* w;
  const int* drop_target;
  int n0, nl, B, N, T, G;
  float f_safety, f_headway, f_divider, f_comfort, f_progress, f_rule, f_volume, headway_L, divider_L;
  float* cost_fo;
  float* cost_fc;
  float* cs;
};

// Progress drops its target term when target_points.sum() < 0.5 — a sum over the whole batch, formed once per call
__global__ void plan_target_flag_kernel(const float* __restrict__ target, int n, int* __restrict__ flag) {
  if (blockIdx.x || threadIdx.x) return;
  float s = 0.f;
  for (int i = 0; i < n; ++i) s += target[i];
  *flag = s < 0.5f ? 1 : 0;
}

// One wavefront per trajectory.  Per waypoint the lanes stride over the footprint cells (n0 of the ego rectangle, nl of the rectangle
// grown by lambda) and over the divider window; butterfly sums form the areas.  The per-trajectory chains (speed, acceleration, jerk,
// progress) are carried in registers by every lane alike.  Every gather is clamped into the grid as the reference clamps it.
__global__ __launch_bounds__(COST_WAVES* WAVE) void plan_cost_kernel(PlanCostArgs a) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & (WAVE - 1);
  const long traj = (long)blockIdx.x * COST_WAVES + (threadIdx.x >> 6);
  if (traj >= (long)a.B * a.N) return;      // a whole wavefront at a time
  const int b = (int)(traj / a.N), G = a.G, T = a.T;
  const float dx0 = a.dx[0], dx1 = a.dx[1], bx0 = a.bx[0], bx1 = a.bx[1], w0 = a.w[0], w1 = a.w[1];
  const size_t plane = (size_t)G * G;
  const float* __restrict__ p = a.trajs + (size_t)traj * T * a.stride;
  const float* __restrict__ lane_map = a.lane + (size_t)b * plane;
  const float* __restrict__ drv = a.drv + (size_t)b * plane;
  // lane pixels further than divider_L cannot lower a distance that counts: ceil(L / min(dx)) cells each way
  float reach = ceilf(a.divider_L / fminf(dx0, dx1));
  const int R = !(reach > 0.f) ? 0 : (reach > (float)G ? G : (int)reach);
  const int side = 2 * R + 1;
  const long cells = (long)side * side;      // R <= G <= 32768: past int for a reach of thousands of cells

  float px = 0.f, py = 0.f, vlat_prev = 0.f, vlon_prev = 0.f, ev_prev = 0.f, eacc_prev = 0.f;
  float max_lat = 0.f, max_lon = 0.f, max_jerk = 0.f, ymax = 0.f, fo_sum = 0.f, x = 0.f, y = 0.f;
#pragma unroll 1
  for (int t = 0; t < T; ++t) {
    x = p[t * a.stride] * -1.f;          // trajs * [-1, 1]
    y = p[t * a.stride + 1];
    // get_points: / dx, then x and y swap: the row comes from y / dx[1], the column from x / dx[0]
    const float qc = x / dx0, qr = y / dx1, qrh = (y + a.headway_L) / dx1;
    const uint8_t* __restrict__ occ = a.occ + ((size_t)b * T + t) * plane;
    int s1 = 0, s2 = 0, off_road = 0;
    float ahead = 0.f;
#pragma unroll 1
    for (int i = lane; i < a.n0; i += WAVE) {
      const float fr = (float)a.rc0[2 * i], fc = (float)a.rc0[2 * i + 1];
      const int r = cell(qr + fr, G), c = cell(qc + fc, G), rh = cell(qrh + fr, G);
      s1 += occ[(size_t)r * G + c];
      off_road += drv[(size_t)r * G + c] == 0.f ? 1 : 0;
      ahead += (float)occ[(size_t)rh * G + c] * drv[(size_t)rh * G + c];
    }
#pragma unroll 1
    for (int i = lane; i < a.nl; i += WAVE) {
      const int r = cell(qr + (float)a.rcl[2 * i], G), c = cell(qc + (float)a.rcl[2 * i + 1], G);
      s2 += occ[(size_t)r * G + c];
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    off_road = wave_sum(off_road);
    ahead = wave_sum(ahead);

    const float ddx = x - px, ddy = y - py;      // p_{-1} = 0
    const float speed = sqrtf(ddx * ddx + ddy * ddy) / 0.5f;
    const float safety = clampf(((float)s1 * w0 + ((float)s2 * speed) * w1) * a.f_safety, 0.f, 100.f);
    const float headway = clampf(ahead * a.f_headway, 0.f, 100.f);
    const float rule = clampf((float)off_road * a.f_rule, 0.f, 100.f);

    // discretize: the point's own cell
    const int yi = cell((y - bx0) / dx0, G), xi = cell((x - bx1) / dx1, G);
    const float cvol = clampf(clampf(a.cost_volume[((size_t)b * T + t) * plane + (size_t)yi * G + xi], 0.f, 1000.f) * a.f_volume, 0.f, 100.f);

    float dmin = __builtin_inff();
#pragma unroll 1
    for (long k = lane; k < cells; k += WAVE) {
      const int dr = (int)(k / side) - R, dc = (int)(k % side) - R;
      const int r = yi + dr, c = xi + dc;
      if (r >= 0 && r < G && c >= 0 && c < G && lane_map[(size_t)r * G + c] != 0.f) {
        const float ey = (float)dr * dx1, ex = (float)dc * dx0;      // (yx - index) * reversed(dx)
        dmin = fminf(dmin, sqrtf(ey * ey + ex * ex));
      }
    }
    dmin = wave_min(dmin);
    const float gap = a.divider_L - dmin;
    const float divider = clampf((dmin > a.divider_L ? 0.f : gap * gap) * a.f_divider, 0.f, 100.f);

    const float fo = safety + headway + divider + cvol + rule;
    if (lane == 0) a.cost_fo[(size_t)traj * T + t] = fo;
    fo_sum += fo;

    // Comfort: acceleration chains start at i = 1, the jerk chain at i = 2
    const float vlat = ddx / 0.5f, vlon = ddy / 0.5f;
    float eacc = 0.f;
    if (t >= 1) {
      max_lat = fmaxf(max_lat, fabsf((vlat - vlat_prev) / 0.5f));
      max_lon = fmaxf(max_lon, fabsf((vlon - vlon_prev) / 0.5f));
      eacc = (speed - ev_prev) / 0.5f;
    }
    if (t >= 2) max_jerk = fmaxf(max_jerk, fabsf((eacc - eacc_prev) / 0.5f));
    ymax = t == 0 ? y : fmaxf(ymax, y);
    vlat_prev = vlat, vlon_prev = vlon, ev_prev = speed, eacc_prev = eacc, px = x, py = y;
  }
  if (lane) return;
  const float lat = clampf(max_lat - 3.f, 0.f, 30.f), lon = clampf(max_lon - 3.f, 0.f, 30.f), jerk = clampf(max_jerk - 1.f, 0.f, 20.f);
  float sub = 0.f + lat * lat;
  sub += lon * lon;
  sub += jerk * jerk;
  const float comfort = clampf(sub * a.f_comfort, 0.f, 100.f);
  float to_target = 0.f;
  if (!*a.drop_target) {
    const float ex = x - a.target[2 * b], ey = y - a.target[2 * b + 1];      // the last waypoint
    to_target = ex * ex + ey * ey;
  }
  const float progress = clampf((to_target - ymax) * a.f_progress, -100.f, 100.f);
  const float fc = comfort + progress;
  a.cost_fc[traj] = fc;
  a.cs[traj] = fc + fo_sum;
}

struct PlanRefineArgs {
  const float* cs;
  const float* trajs;
  long stride;
  const float* target;
  const float* h0;
  const float *w_ih, *w_hh, *b_ih, *b_hh, *w1, *b1, *w2, *b2;
  int N, T, S;
  float* selected;
  float* refined;
};

__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v < bv || (v == bv && i < bi); }

// dot(row of an [rows, S] matrix, vec in LDS) by one wavefront: lanes stride over the columns (coalesced), butterfly sum
__device__ __forceinline__ float wave_dot(const float* __restrict__ row, const float* vec, int S, int lane) {
  float acc = 0.f;
  for (int k = lane; k < S; k += WAVE) acc += row[k] * vec[k];
  return wave_sum(acc);
}

// One workgroup per sample: arg-min of cs over N (lowest index on a tie), the selected [T, 3] trajectory, then — S > 0 — the
// refinement loop with h and x in LDS: GRUCell([x, traj_t[:2], target]) -> Linear -> ReLU -> Linear -> x, gate order r, z, n.
__global__ __launch_bounds__(REFINE_THREADS) void plan_select_refine_kernel(PlanRefineArgs a) {
  __shared__ float s_val[REFINE_THREADS / WAVE];
  __shared__ int s_idx[REFINE_THREADS / WAVE];
  __shared__ int s_pick;
  __shared__ float h[MAX_STATE], hid[MAX_STATE], gi[3 * MAX_STATE], gh[3 * MAX_STATE], xin[8], xs[2];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6, b = blockIdx.x;
  const int N = a.N, T = a.T, S = a.S;
  const float* __restrict__ cs = a.cs + (size_t)b * N;
  float bv = __builtin_inff();
  int bi = 0x7fffffff;
  for (int n = tid; n < N; n += REFINE_THREADS) {
    const float v = cs[n];
    if (better(v, n, bv, bi)) bv = v, bi = n;
  }
#pragma unroll
  for (int o = WAVE / 2; o; o >>= 1) {
    const float ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (better(ov, oi, bv, bi)) bv = ov, bi = oi;
  }
  if (lane == 0) s_val[wave] = bv, s_idx[wave] = bi;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < REFINE_THREADS / WAVE; ++w)
      if (better(s_val[w], s_idx[w], bv, bi)) bv = s_val[w], bi = s_idx[w];
    s_pick = (bi < 0 || bi >= N) ? 0 : bi;      // nothing compares below +inf (all NaN): take index 0, never an index outside the row
  }
  __syncthreads();
  const float* __restrict__ pick = a.trajs + ((size_t)b * N + s_pick) * T * a.stride;
  for (int i = tid; i < T * 3; i += REFINE_THREADS) a.selected[(size_t)b * T * 3 + i] = pick[(i / 3) * a.stride + i % 3];
  if (S <= 0) return;

  if (tid < S) h[tid] = a.h0[(size_t)b * S + tid];
  if (tid < 2) xs[tid] = 0.f;
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    if (tid < 2) xin[tid] = xs[tid];
    else if (tid < 4) xin[tid] = pick[t * a.stride + tid - 2];
    else if (tid < 6) xin[tid] = a.target[2 * b + tid - 4];
    __syncthreads();
    for (int row = wave; row < 3 * S; row += REFINE_THREADS / WAVE) {
      const float hh = wave_dot(a.w_hh + (size_t)row * S, h, S, lane);
      const float ii = wave_sum(lane < 6 ? a.w_ih[row * 6 + lane] * xin[lane] : 0.f);
      if (lane == 0) gi[row] = ii + a.b_ih[row], gh[row] = hh + a.b_hh[row];
    }
    __syncthreads();
    if (tid < S) {
      const float r = 1.f / (1.f + expf(-(gi[tid] + gh[tid])));
      const float z = 1.f / (1.f + expf(-(gi[S + tid] + gh[S + tid])));
      const float n = tanhf(gi[2 * S + tid] + r * gh[2 * S + tid]);
      h[tid] = n + z * (h[tid] - n);
    }
    __syncthreads();
    for (int row = wave; row < S; row += REFINE_THREADS / WAVE) {
      const float v = wave_dot(a.w1 + (size_t)row * S, h, S, lane);
      if (lane == 0) hid[row] = fmaxf(v + a.b1[row], 0.f);
    }
    __syncthreads();
    if (wave < 2) {
      const float v = wave_dot(a.w2 + (size_t)wave * S, hid, S, lane);
      if (lane == 0) {
        xs[wave] = v + a.b2[wave];
        a.refined[((size_t)b * T + t) * 3 + wave] = xs[wave];
      }
    } else if (tid == 2 * WAVE) {
      a.refined[((size_t)b * T + t) * 3 + 2] = 0.f;
    }
    __syncthreads();
  }
}

struct PlanMetricArgs {
  const float* trajs;
  const float* gt;
  long stride;
  const uint8_t* seg;
  const int32_t* rc0;
  const float* dx;
  const float* bx;
  int n0, B, T, G;
  float* obj_col;
  float* obj_box_col;
  float* l2;
  long long* total;
};

// evaluate_single_coll: does the ego rectangle at (x, y) (already mirrored) touch an occupied cell?  The reference swaps, divides by dx
// in fp32, adds the integer table in numpy (float64) and truncates.
__device__ __forceinline__ bool box_hit(const uint8_t* __restrict__ seg, const int32_t* __restrict__ rc, int n, float x, float y, float dx0, float dx1,
                                        int G, int lane) {
  const float qr = y / dx0, qc = x / dx1;
  bool hit = false;
#pragma unroll 1
  for (int i = lane; i < n; i += WAVE) {
    const int r = cell((double)qr + (double)rc[2 * i], G), c = cell((double)qc + (double)rc[2 * i + 1], G);
    hit |= seg[(size_t)r * G + c] != 0;
  }
  return __ballot(hit) != 0;
}

// One wavefront per frame t; it walks the batch in order and is the only writer of its counters: no atomics, the same sums on every run.
__global__ __launch_bounds__(WAVE) void plan_metric_kernel(PlanMetricArgs a) {
#pragma clang fp contract(off)
  const int t = blockIdx.x, lane = threadIdx.x, G = a.G;
  const float dx0 = a.dx[0], dx1 = a.dx[1], bx0 = a.bx[0], bx1 = a.bx[1];
  float col = 0.f, box = 0.f, l2 = 0.f;
#pragma unroll 1
  for (int b = 0; b < a.B; ++b) {
    const float* __restrict__ p = a.trajs + ((size_t)b * a.T + t) * a.stride;
    const float* __restrict__ g = a.gt + ((size_t)b * a.T + t) * a.stride;
    const uint8_t* __restrict__ seg = a.seg + ((size_t)b * a.T + t) * (size_t)G * G;
    const float x = p[0] * -1.f, y = p[1];
    const bool gt_hit = box_hit(seg, a.rc0, a.n0, g[0] * -1.f, g[1], dx0, dx1, G, lane);
    const bool own_hit = box_hit(seg, a.rc0, a.n0, x, y, dx0, dx1, G, lane);
    // the in-range test is on the truncated index: anything in (-1, 0) is cell 0
    const float vy = (y - bx0) / dx0, vx = (x - bx1) / dx1;
    const bool inside = vy > -1.f && vy < (float)G && vx > -1.f && vx < (float)G;
    if (inside && !gt_hit) col += (float)seg[(size_t)(int)vy * G + (int)vx];
    if (!gt_hit) box += own_hit ? 1.f : 0.f;
    const float ex = p[0] - g[0], ey = p[1] - g[1];
    l2 += sqrtf(ex * ex + ey * ey);
  }
  if (lane) return;
  a.obj_col[t] += col;
  a.obj_box_col[t] += box;
  a.l2[t] += l2;
  if (t == 0) *a.total += a.B;
}

}  // namespace
}  // namespace sf

using namespace sf;

extern "C" {

size_t sf_plan_cost_ws_bytes(void) { return 256; }

int sf_plan_cost_fwd(const float* trajs, long traj_stride, const float* cost_volume, const uint8_t* occupancy, const float* lane_divider,
                     const float* drivable, const float* target_points, const int32_t* rc0, int n0, const int32_t* rc_lambda, int n_lambda,
                     const float* dx, const float* bx, const float* safety_w, const float* factors, float headway_L, float divider_L, int B,
                     int N, int T, int H, int W, float* cost_fo, float* cost_fc, float* cs, void* ws, size_t ws_bytes, void* stream) {
  if (!trajs || !cost_volume || !occupancy || !lane_divider || !drivable || !target_points || !rc0 || !rc_lambda || !dx || !bx || !safety_w ||
      !factors || !cost_fo || !cost_fc || !cs || !ws)
    return SF_ERR_INVALID;
  if (B < 1 || N < 1 || T < 1 || H < 1 || H != W || H > 32768 || n0 < 0 || n_lambda < 0 || traj_stride < 2) return SF_ERR_INVALID;
  if ((long)B * N >= (1L << 31) - 8 || (long)B * 2 >= (1L << 31)) return SF_ERR_INVALID;
  if (ws_bytes < sf_plan_cost_ws_bytes()) return SF_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  PlanCostArgs a;
  a.trajs = trajs, a.stride = traj_stride, a.cost_volume = cost_volume, a.occ = occupancy, a.lane = lane_divider, a.drv = drivable;
  a.target = target_points, a.rc0 = rc0, a.rcl = rc_lambda, a.dx = dx, a.bx = bx, a.w = safety_w, a.drop_target = static_cast<const int*>(ws);
  a.n0 = n0, a.nl = n_lambda, a.B = B, a.N = N, a.T = T, a.G = H;
  a.f_safety = factors[0], a.f_headway = factors[1], a.f_divider = factors[2], a.f_comfort = factors[3], a.f_progress = factors[4];
  a.f_rule = factors[5], a.f_volume = factors[6], a.headway_L = headway_L, a.divider_L = divider_L;
  a.cost_fo = cost_fo, a.cost_fc = cost_fc, a.cs = cs;
  hipLaunchKernelGGL(plan_target_flag_kernel, dim3(1), dim3(WAVE), 0, st, target_points, 2 * B, static_cast<int*>(ws));
  const long waves = (long)B * N;
  hipLaunchKernelGGL(plan_cost_kernel, dim3((unsigned)((waves + COST_WAVES - 1) / COST_WAVES)), dim3(COST_WAVES * WAVE), 0, st, a);
  return hipGetLastError() == hipSuccess ? SF_OK : SF_ERR_LAUNCH;
}

int sf_plan_select_refine_fwd(const float* cs, const float* trajs, long traj_stride, const float* target_points, const float* h0,
                              const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const float* w1, const float* b1,
                              const float* w2, const float* b2, int B, int N, int T, int S, float* selected, float* refined, void* stream) {
  if (!cs || !trajs || !selected || B < 1 || N < 1 || T < 1 || S < 0 || S > MAX_STATE || traj_stride < 3) return SF_ERR_INVALID;
  if (S > 0 && (!target_points || !h0 || !w_ih || !w_hh || !b_ih || !b_hh || !w1 || !b1 || !w2 || !b2 || !refined)) return SF_ERR_INVALID;
  PlanRefineArgs a;
  a.cs = cs, a.trajs = trajs, a.stride = traj_stride, a.target = target_points, a.h0 = h0;
  a.w_ih = w_ih, a.w_hh = w_hh, a.b_ih = b_ih, a.b_hh = b_hh, a.w1 = w1, a.b1 = b1, a.w2 = w2, a.b2 = b2;
  a.N = N, a.T = T, a.S = S, a.selected = selected, a.refined = refined;
  hipLaunchKernelGGL(plan_select_refine_kernel, dim3((unsigned)B), dim3(REFINE_THREADS), 0, static_cast<hipStream_t>(stream), a);
  return hipGetLastError() == hipSuccess ? SF_OK : SF_ERR_LAUNCH;
}

int sf_plan_metric_fwd(const float* trajs, const float* gt_trajs, long traj_stride, const uint8_t* segmentation, const int32_t* rc0, int n0,
                       const float* dx, const float* bx, int B, int T, int H, int W, float* obj_col, float* obj_box_col, float* l2,
                       int64_t* total, void* stream) {
  if (!trajs || !gt_trajs || !segmentation || !rc0 || !dx || !bx || !obj_col || !obj_box_col || !l2 || !total) return SF_ERR_INVALID;
  if (B < 1 || T < 1 || H < 1 || H != W || H > 32768 || n0 < 0 || traj_stride < 2) return SF_ERR_INVALID;
  PlanMetricArgs a;
  a.trajs = trajs, a.gt = gt_trajs, a.stride = traj_stride, a.seg = segmentation, a.rc0 = rc0, a.dx = dx, a.bx = bx;
  a.n0 = n0, a.B = B, a.T = T, a.G = H, a.obj_col = obj_col, a.obj_box_col = obj_box_col, a.l2 = l2;
  a.total = reinterpret_cast<long long*>(total);
  hipLaunchKernelGGL(plan_metric_kernel, dim3((unsigned)T), dim3(WAVE), 0, static_cast<hipStream_t>(stream), a);
  return hipGetLastError() == hipSuccess ? SF_OK : SF_ERR_LAUNCH;
}

}  // extern "C"
