// Instance tracking for gfx950: the frame-to-frame assignment of make_instance_id_temporally_consistent[_short_interval]
// (streamingflow/utils/instance.py:171-368) on the moments sf_instance_moments_fwd leaves on the device.
//   sf_instance_track_fwd   tables[frame][raw id] = consistent id, for B samples of T frames, in two launches:
//     assign  one workgroup per (sample, frame pair): cost matrix of centre distances in LDS, the rectangular assignment by shortest
//             augmenting paths (Jonker-Volgenant as Crouse states it, the method of scipy.optimize.linear_sum_assignment), the accepted
//             partner of every raw id of frame t+1 into the workspace;
//     chain   one wavefront per sample: hands the ids down t = 0 .. T-2 from those lists and counts the new ids.
// The arithmetic is the host path's (streamingflow_amd/instance.py: _means, _consistent_tables) operation for operation: centres are
// fp64 quotients rounded to fp32, a distance is sqrt(dr*dr + dc*dc) in fp32 with every operation rounded on its own (the compiler's
// contraction is off in both kernels; the build passes no fast-math flag, so `/` and sqrtf are the correctly rounded ones), duals and
// path costs are fp64 in scipy's operation order.  Where a pair has ONE optimal assignment the tables are therefore the host's; where it
// has several, the solver takes the lowest column among equal path costs and so returns one of them, the same on every run
// (DESIGN.md §6b N4).
// Every loop is bounded by a row or column count.  A cost that is NaN or infinite ends the pair (no column can be chosen) and sets the
// sample's flag; so does a frame t+1 whose raw ids are not 1..n, where the host path's scipy call raises.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "../../include/sfnative.h"

namespace sf {
namespace {

constexpr int WAVE = 64;
constexpr int TRACK_MAX_N = 128;                  // instances of a frame: raw ids 1 .. K-1 <= 128
constexpr int TRACK_ID_SLOTS = 3 * WAVE;          // ids 0 .. 128 in whole wavefront passes
constexpr int PAIR_OK = 0, PAIR_EMPTY = 1, PAIR_BAD = 2;
constexpr double TRACK_INF = __builtin_huge_val();

__host__ __device__ constexpr size_t a256t(size_t v) { return (v + 255) & ~size_t(255); }

struct TrackLayout {
  size_t pairs, match_bytes, total;      // workspace: match int32 [pairs][K] | status int32 [pairs]
};
static bool track_layout(int B, int T, int K, TrackLayout* L) {
  if (B < 1 || T < 1 || K < 1 || K - 1 > TRACK_MAX_N) return false;
  if ((size_t)B * T * K >= (size_t(1) << 31)) return false;
  L->pairs = (size_t)B * (T > 1 ? T - 1 : 1);
  L->match_bytes = a256t(L->pairs * K * sizeof(int32_t));
  L->total = L->match_bytes + a256t(L->pairs * sizeof(int32_t));
  return true;
}

// (value, column) minimum: the lower value, the lower column among equal values.  A NaN never wins (both comparisons are false).
__device__ __forceinline__ void take_lower(double& v, int& j, double ov, int oj) {
  if (ov < v || (ov == v && oj < j)) v = ov, j = oj;
}

// sum / count in fp64, rounded to fp32 (instance.py: _means)
__device__ __forceinline__ float mean32(long long sum, double scale, int count) { return (float)((double)sum * scale / (double)count); }

// One workgroup of THREADS per (sample b, pair t -> t+1).  prev = the present raw ids of frame t in ascending order, next = raw ids
// 1 .. n_next of frame t+1.  The smaller side takes the rows (scipy transposes the same way), the cost matrix [rows][cols] is fp32 in
// dynamic LDS.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void track_assign_kernel(const int* __restrict__ counts, const long long* __restrict__ pos,
                                                               const long long* __restrict__ warped, int T, int K, float threshold,
                                                               int* __restrict__ match, int* __restrict__ status) {
#pragma clang fp contract(off)
  constexpr int WAVES = THREADS / WAVE;
  extern __shared__ __attribute__((aligned(16))) float cost[];
  __shared__ double u[TRACK_MAX_N], v[TRACK_MAX_N], reach[TRACK_MAX_N];      // duals; reach[j] = shortest path cost to column j
  __shared__ double red_v[WAVES];
  __shared__ int red_j[WAVES];
  __shared__ int path[TRACK_MAX_N], col4row[TRACK_MAX_N], row4col[TRACK_MAX_N], prev_ids[TRACK_MAX_N], partner[TRACK_MAX_N + 1];
  __shared__ unsigned char in_rows[TRACK_MAX_N], in_cols[TRACK_MAX_N];
  __shared__ float next_c[TRACK_MAX_N][2], prev_a[TRACK_MAX_N][2];
  __shared__ int head[3];      // instances of t, largest raw id of t+1, instances of t+1

  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
  const int pair = blockIdx.x, b = pair / (T - 1), t = pair - b * (T - 1);
  const size_t f0 = (size_t)b * T + t, f1 = f0 + 1;
  const int* __restrict__ cnt0 = counts + f0 * K;
  const int* __restrict__ cnt1 = counts + f1 * K;
  int* __restrict__ out = match + (size_t)pair * K;

  if (wave == 0) {      // present ids of t in ascending order; the id range of t+1
    int n_prev = 0, top_next = 0, n_next = 0;
#pragma unroll
    for (int base = 0; base < TRACK_ID_SLOTS; base += WAVE) {
      const int id = base + lane;
      const bool live = id >= 1 && id < K;
      const bool here = live && cnt0[id] > 0, there = live && cnt1[id] > 0;
      const unsigned long long m0 = __ballot(here), m1 = __ballot(there);
      if (here) prev_ids[n_prev + __popcll(m0 & ((1ull << lane) - 1))] = id;
      n_prev += __popcll(m0);
      n_next += __popcll(m1);
      if (m1) top_next = base + 63 - __clzll(m1);
    }
    if (lane == 0) head[0] = n_prev, head[1] = top_next, head[2] = n_next;
  }
  for (int k = tid; k <= TRACK_MAX_N; k += THREADS) partner[k] = -1;
  __syncthreads();
  const int n_prev = head[0], n_next = head[1];
  int state = PAIR_OK;
  if (n_prev == 0 || head[2] == 0) state = PAIR_EMPTY;
  else if (head[2] != n_next) state = PAIR_BAD;      // a gap inside 1..n_next: its centre is NaN on the host
  if (state == PAIR_OK) {
    const double scale = warped ? 1.0 / 1048576.0 : 1.0;
    const long long* __restrict__ anchor_sums = (warped ? warped : pos) + f0 * K * 2;
    const long long* __restrict__ next_sums = pos + f1 * K * 2;
    for (int i = tid; i < n_prev; i += THREADS) {
      const int id = prev_ids[i];
      prev_a[i][0] = mean32(anchor_sums[2 * id], scale, cnt0[id]);
      prev_a[i][1] = mean32(anchor_sums[2 * id + 1], scale, cnt0[id]);
    }
    for (int j = tid; j < n_next; j += THREADS) {
      next_c[j][0] = mean32(next_sums[2 * (j + 1)], 1.0, cnt1[j + 1]);
      next_c[j][1] = mean32(next_sums[2 * (j + 1) + 1], 1.0, cnt1[j + 1]);
    }
    __syncthreads();
    const bool flipped = n_prev > n_next;      // rows = next, columns = prev
    const int nr = flipped ? n_next : n_prev, nc = flipped ? n_prev : n_next;
    for (int e = tid; e < nr * nc; e += THREADS) {
      const int r = e / nc, c = e - r * nc;
      const int ip = flipped ? c : r, in = flipped ? r : c;
      const float dr = next_c[in][0] - prev_a[ip][0], dc = next_c[in][1] - prev_a[ip][1];
      cost[e] = sqrtf(dr * dr + dc * dc);
    }
    for (int k = tid; k < TRACK_MAX_N; k += THREADS) u[k] = 0.0, v[k] = 0.0, path[k] = -1, col4row[k] = -1, row4col[k] = -1;
    __syncthreads();

#pragma unroll 1
    for (int cur = 0; cur < nr && state == PAIR_OK; ++cur) {
      for (int k = tid; k < TRACK_MAX_N; k += THREADS) reach[k] = TRACK_INF, in_rows[k] = 0, in_cols[k] = 0;
      __syncthreads();
      double low = 0.0;
      int i = cur, sink = -1;
      // a step moves one column into the tree, and an unassigned column ends the walk: at most cur + 1 steps
#pragma unroll 1
      for (int step = 0; step <= cur && sink < 0; ++step) {
        const double ui = u[i];
        double best = TRACK_INF;
        int at = TRACK_MAX_N;
        for (int j = tid; j < nc; j += THREADS) {
          if (in_cols[j]) continue;
          const double r = low + (double)cost[i * nc + j] - ui - v[j];
          double s = reach[j];
          if (r < s) reach[j] = s = r, path[j] = i;
          take_lower(best, at, s, j);
        }
#pragma unroll
        for (int o = WAVE / 2; o; o >>= 1) take_lower(best, at, __shfl_xor(best, o), __shfl_xor(at, o));
        if constexpr (WAVES > 1) {
          if (lane == 0) red_v[wave] = best, red_j[wave] = at;
          __syncthreads();
          best = red_v[0], at = red_j[0];
#pragma unroll
          for (int w = 1; w < WAVES; ++w) take_lower(best, at, red_v[w], red_j[w]);
        }
        if (at >= nc || !(best < TRACK_INF)) {      // NaN or infinite costs: no column to go to (the same for every thread)
          state = PAIR_BAD;
          break;
        }
        low = best;
        if (tid == 0) in_rows[i] = 1, in_cols[at] = 1;
        const int owner = row4col[at];
        if (owner < 0) sink = at;
        else i = owner;
        __syncthreads();
      }
      if (state != PAIR_OK) break;
      if (sink < 0) {      // not reachable with finite costs
        state = PAIR_BAD;
        break;
      }
      for (int r = tid; r < nr; r += THREADS)
        if (in_rows[r]) u[r] += r == cur ? low : low - reach[col4row[r]];
      for (int j = tid; j < nc; j += THREADS)
        if (in_cols[j]) v[j] -= low - reach[j];
      __syncthreads();
      if (tid == 0) {      // flip the path back from the sink: at most cur + 1 rows long
        int j = sink;
        for (int hop = 0; hop <= cur; ++hop) {
          const int r = path[j];
          row4col[j] = r;
          const int before = col4row[r];
          col4row[r] = j;
          j = before;
          if (r == cur) break;
        }
      }
      __syncthreads();
    }

    if (state == PAIR_OK) {
      for (int r = tid; r < nr; r += THREADS) {
        const int c = col4row[r];
        if (c < 0 || c >= nc) continue;
        if (cost[r * nc + c] < threshold) partner[(flipped ? r : c) + 1] = prev_ids[flipped ? c : r];
      }
    }
    __syncthreads();
  }
  for (int k = tid; k < K; k += THREADS) out[k] = state == PAIR_OK ? partner[k] : -1;
  if (tid == 0) status[pair] = state;
}

// One wavefront per sample.  The table of frame t stays in LDS while frame t+1 is written from it.
__global__ __launch_bounds__(WAVE) void track_chain_kernel(const int* __restrict__ counts, const int* __restrict__ match,
                                                           const int* __restrict__ status, int T, int K, long long* __restrict__ tables,
                                                           int* __restrict__ flags) {
  __shared__ long long held[2][TRACK_ID_SLOTS];
  const int lane = threadIdx.x, b = blockIdx.x;
  const int* __restrict__ cnt = counts + (size_t)b * T * K;
  long long* __restrict__ tab = tables + (size_t)b * T * K;
  long long next_new = 0;      // the largest id of the first frame
#pragma unroll
  for (int base = 0; base < TRACK_ID_SLOTS; base += WAVE) {
    const int id = base + lane;
    const unsigned long long m = __ballot(id < K && cnt[id] > 0);
    if (m) next_new = base + 63 - __clzll(m);
    held[0][id] = id;
    if (id < K) tab[id] = id;
  }
  __syncthreads();
  int bad = 0;
#pragma unroll 1
  for (int t = 0; t + 1 < T; ++t) {
    const size_t pair = (size_t)b * (T - 1) + t;
    const int state = status[pair];
    bad |= state == PAIR_BAD;
    const long long* __restrict__ from = held[t & 1];
    long long* __restrict__ to = held[(t + 1) & 1];
    const int* __restrict__ here = cnt + (size_t)(t + 1) * K;
    const int* __restrict__ mt = match + pair * K;
#pragma unroll
    for (int base = 0; base < TRACK_ID_SLOTS; base += WAVE) {
      const int id = base + lane;
      long long val = id;
      if (state != PAIR_EMPTY) {      // the same for the whole wavefront
        const bool present = id >= 1 && id < K && here[id] > 0;
        const int m = present ? mt[id] : -1;
        const bool fresh = present && (m < 0 || m >= K);
        const unsigned long long mask = __ballot(fresh);
        if (fresh) val = next_new + 1 + __popcll(mask & ((1ull << lane) - 1));
        else if (present) val = from[m];
        next_new += __popcll(mask);
      }
      to[id] = val;
      if (id < K) tab[(size_t)(t + 1) * K + id] = val;
    }
    __syncthreads();
  }
  if (lane == 0) flags[b] = bad;
}

template <int THREADS>
static hipError_t launch_assign(const int* counts, const long long* pos, const long long* warped, int pairs, int T, int K, float threshold,
                                int* match, int* status, hipStream_t st) {
  void (*kern)(const int*, const long long*, const long long*, int, int, float, int*, int*) = track_assign_kernel<THREADS>;
  constexpr int lds_max = TRACK_MAX_N * TRACK_MAX_N * (int)sizeof(float);
  static bool attr_done[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;
  if (!attr_done[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    if (e != hipSuccess) return e;
    attr_done[dev] = true;
  }
  const size_t lds = (size_t)(K - 1) * (K - 1) * sizeof(float);
  hipLaunchKernelGGL(kern, dim3((unsigned)pairs), dim3(THREADS), lds, st, counts, pos, warped, T, K, threshold, match, status);
  return hipGetLastError();
}

}  // namespace
}  // namespace sf

using namespace sf;

extern "C" {

size_t sf_instance_track_ws_bytes(int B, int T, int K) {
  TrackLayout L;
  return track_layout(B, T, K, &L) ? L.total : 0;
}

int sf_instance_track_fwd(const int32_t* counts, const int64_t* pos_sums, const int64_t* warped_fx, int B, int T, int K,
                          float matching_threshold, int64_t* tables, int32_t* flags, void* ws, size_t ws_bytes, void* stream) {
  TrackLayout L;
  if (!counts || !pos_sums || !tables || !flags || !ws || !track_layout(B, T, K, &L)) return SF_ERR_INVALID;
  if (ws_bytes < L.total) return SF_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  int* match = static_cast<int*>(ws);
  int* status = reinterpret_cast<int*>(static_cast<char*>(ws) + L.match_bytes);
  const long long* pos = reinterpret_cast<const long long*>(pos_sums);
  const long long* warped = reinterpret_cast<const long long*>(warped_fx);
  if (T > 1 && K > 1) {
    const char* e = getenv("SF_TRACK_WAVES");      // measurement switch (tools/trackbench.py): 1 or 4 wavefronts per pair; unset: the default
    const int waves = e && (e[0] == '1' || e[0] == '4') ? e[0] - '0' : 1;
    const int pairs = B * (T - 1);
    hipError_t err = waves == 4 ? launch_assign<4 * WAVE>(counts, pos, warped, pairs, T, K, matching_threshold, match, status, st)
                                : launch_assign<WAVE>(counts, pos, warped, pairs, T, K, matching_threshold, match, status, st);
    if (err != hipSuccess) return SF_ERR_LAUNCH;
  } else if (T > 1) {
    if (hipMemsetAsync(status, 0, L.pairs * sizeof(int32_t), st) != hipSuccess) return SF_ERR_LAUNCH;      // K == 1: no instance anywhere
    if (hipMemsetAsync(match, 0xff, L.pairs * K * sizeof(int32_t), st) != hipSuccess) return SF_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(track_chain_kernel, dim3((unsigned)B), dim3(WAVE), 0, st, counts, match, status, T, K,
                     reinterpret_cast<long long*>(tables), flags);
  return hipGetLastError() == hipSuccess ? SF_OK : SF_ERR_LAUNCH;
}

}  // extern "C"
