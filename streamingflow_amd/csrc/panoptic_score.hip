// Panoptic-quality scoring for gfx950: PanopticMetric.update's bookkeeping (streamingflow/metrics.py:143-229, as
// streamingflow_amd/metrics.py: _score_frame and the loop around it state it) on the per-frame joint histograms that
// sf_confusion_frames_fwd leaves on the device.
//   sf_panoptic_score_fwd   hist [B*T][K][K] (rows = ground-truth id, columns = predicted id) -> ADDS one update's tallies into the four
//                           fp32 counters, in two launches:
//     frames  one workgroup per frame: row and column sums (the segment areas) through LDS, then per ground-truth id g the column of
//             its hit (IoU > 0.5) and that IoU into the workspace, and the frame's unmatched ground-truth / predicted things;
//     tally   ONE workgroup: a lane per (sample, g) walks the sample's frames with g's partner in a register (id switches), the frames'
//             unmatched counts and background hits are summed beside it, and one thread performs the single add per counter.
// The arithmetic is the host path's operation for operation: areas and unions are integers, an IoU is
// (float(joint) + 1e-9f) / (float(union) + 1e-9f) in fp32 with every operation rounded on its own (contraction is off; the build passes
// no fast-math flag, so __fdiv_rn is the correctly rounded quotient).  The entry point refuses frames of 2^23 pixels or more, so every
// integer is exact in fp32, IoU > 0.5 means joint > union / 2, and a row or a column holds at most one hit.  IoU sums are fp64: fewer
// than 2^28 values from (0.5, 1], each a multiple of 2^-24, sum exactly in any order; the sum is rounded to fp32 once and added once,
// which is what the host path does with its float64 tally.  Counts are integers until that add.
// Nothing is indexed by a value read from memory: a histogram that no label map could have produced gives unspecified tallies, never
// an access outside the buffers.  Every loop is bounded by K, T or B*T.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/sfnative.h"

namespace sf {
namespace {

constexpr int WAVE = 64;
constexpr int PQ_MAX_K = SF_PANOPTIC_MAX_K;       // ids 0 .. 255: four wavefront-wide column chunks
constexpr int PQ_CHUNKS = PQ_MAX_K / WAVE;
constexpr int FRAME_THREADS = 256, FRAME_WAVES = FRAME_THREADS / WAVE;
constexpr int TALLY_THREADS = 1024, TALLY_WAVES = TALLY_THREADS / WAVE;
constexpr int STAT_INTS = 4;                      // per frame: unmatched ground truth, unmatched predictions, background pixels in gt, unused
constexpr long PQ_MAX_PIXELS = 1L << 23;
constexpr int ERR_RANGE = SF_PANOPTIC_ERR_RANGE, ERR_NO_BACKGROUND = SF_PANOPTIC_ERR_NO_BACKGROUND;

static_assert(PQ_MAX_K == FRAME_THREADS, "one thread per column in the margin and false-positive passes");

__host__ __device__ constexpr size_t a256p(size_t v) { return (v + 255) & ~size_t(255); }

struct ScoreLayout {
  size_t frames, col_bytes, iou_bytes, total;      // workspace: hit column int32 [F][K] | hit IoU fp32 [F][K] | stats int32 [F][4]
};
static bool score_layout(int B, int T, int K, ScoreLayout* L) {
  if (B < 1 || T < 1 || K < 1 || K > PQ_MAX_K) return false;
  if ((size_t)B * T * K >= (size_t(1) << 31)) return false;
  L->frames = (size_t)B * T;
  L->col_bytes = a256p(L->frames * K * sizeof(int32_t));
  L->iou_bytes = a256p(L->frames * K * sizeof(float));
  L->total = L->col_bytes + L->iou_bytes + a256p(L->frames * STAT_INTS * sizeof(int32_t));
  return true;
}

template <typename V>
__device__ __forceinline__ V wave_sum(V v) {
#pragma unroll
  for (int o = WAVE / 2; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// One workgroup per frame.  A wavefront takes the rows g = wave, wave + 4, ..; its lanes take the columns lane + 64 j.
__global__ __launch_bounds__(FRAME_THREADS) void panoptic_frame_kernel(const long long* __restrict__ hist, int K, int* __restrict__ hit_col,
                                                                      float* __restrict__ hit_iou, int* __restrict__ stats) {
#pragma clang fp contract(off)
  __shared__ long long area_gt[PQ_MAX_K], area_pred[PQ_MAX_K];
  __shared__ long long col_part[FRAME_WAVES][PQ_MAX_K];
  __shared__ unsigned char col_hit[PQ_MAX_K];
  __shared__ int unmatched[2];      // ground truth, predictions

  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
  const size_t f = blockIdx.x;
  const long long* __restrict__ H = hist + f * K * K;
  const int chunks = (K + WAVE - 1) / WAVE;

  long long col[PQ_CHUNKS] = {};
  for (int g = wave; g < K; g += FRAME_WAVES) {
    long long row = 0;
#pragma unroll
    for (int j = 0; j < PQ_CHUNKS; ++j) {
      const int p = lane + WAVE * j;
      if (j < chunks && p < K) {
        const long long v = H[(size_t)g * K + p];
        col[j] += v;
        row += v;
      }
    }
    row = wave_sum(row);
    if (lane == 0) area_gt[g] = row;
  }
#pragma unroll
  for (int j = 0; j < PQ_CHUNKS; ++j) col_part[wave][lane + WAVE * j] = col[j];
  col_hit[tid] = 0;
  if (tid < 2) unmatched[tid] = 0;
  __syncthreads();
  {
    long long s = 0;
#pragma unroll
    for (int w = 0; w < FRAME_WAVES; ++w) s += col_part[w][tid];
    area_pred[tid] = s;      // zero past K
  }
  __syncthreads();

  int lost = 0;      // lane 0: present ground-truth things of this wavefront's rows without a hit
  for (int g = wave; g < K; g += FRAME_WAVES) {
    const long long ag = area_gt[g];
    int found = -1;
    float found_iou = 0.0f;
#pragma unroll
    for (int j = 0; j < PQ_CHUNKS; ++j) {
      if (j >= chunks) break;      // the same for the whole wavefront
      const int p = lane + WAVE * j;
      float iou = 0.0f;
      // thing rows are scored against thing columns, the background row against the background column only
      if (p < K && (g == 0 ? p == 0 : p >= 1)) {
        const long long joint = H[(size_t)g * K + p];
        const float uni = (float)(ag + area_pred[p] - joint);
        if (uni > 0.0f) iou = __fdiv_rn(__fadd_rn((float)joint, 1e-9f), __fadd_rn(uni, 1e-9f));
      }
      const bool hit = iou > 0.5f;
      const unsigned long long m = __ballot(hit);
      const int first = m ? __ffsll((long long)m) - 1 : 0;
      const float first_iou = __shfl(iou, first);
      if (m && found < 0) found = WAVE * j + first, found_iou = first_iou;
      if (hit && g >= 1) col_hit[p] = 1;
    }
    if (lane == 0) {
      hit_col[f * K + g] = found;
      hit_iou[f * K + g] = found_iou;
      lost += g >= 1 && found < 0 && ag > 0;
    }
  }
  if (lane == 0 && lost) atomicAdd(&unmatched[0], lost);
  __syncthreads();
  {
    const unsigned long long m = __ballot(tid >= 1 && tid < K && area_pred[tid] > 0 && !col_hit[tid]);
    if (lane == 0 && m) atomicAdd(&unmatched[1], __popcll(m));
  }
  __syncthreads();
  if (tid == 0) {
    int* __restrict__ s = stats + f * STAT_INTS;
    s[0] = unmatched[0], s[1] = unmatched[1], s[2] = area_gt[0] > 0, s[3] = 0;
  }
}

// One workgroup.  Items (sample b, ground-truth id g >= 1) are independent walks over the sample's frames; the frames' own tallies are
// summed by the same threads.  Thread 0 reads the flags and makes the one add per counter.
__global__ __launch_bounds__(TALLY_THREADS) void panoptic_tally_kernel(const int* __restrict__ hit_col, const float* __restrict__ hit_iou,
                                                                      const int* __restrict__ stats, int B, int T, int K, int track,
                                                                      const int* __restrict__ bad, float* __restrict__ iou,
                                                                      float* __restrict__ tp, float* __restrict__ fp, float* __restrict__ fn,
                                                                      int* __restrict__ errors) {
#pragma clang fp contract(off)
  __shared__ long long part_n[TALLY_WAVES][5];
  __shared__ double part_s[TALLY_WAVES][2];
  __shared__ int part_bg[TALLY_WAVES];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
  long long n_tp = 0, n_switch = 0, n_fn = 0, n_fp = 0, n_bg = 0;
  double s_thing = 0.0, s_bg = 0.0;
  int gt_bg = 0;

  const int things = K - 1;
  const long items = (long)B * things;
  for (long i = tid; i < items; i += TALLY_THREADS) {
    const long b = i / things;
    const int g = 1 + (int)(i - b * things);
    const size_t at = (size_t)b * T * K + g;
    int partner = -1;      // predicted id of g's latest hit in this sample
    for (int t = 0; t < T; ++t) {
      const int p = hit_col[at + (size_t)t * K];
      if (p < 1) continue;
      const bool switched = track && partner >= 0 && partner != p;
      partner = p;
      if (switched) ++n_switch;
      else ++n_tp, s_thing += (double)hit_iou[at + (size_t)t * K];
    }
  }
  const long frames = (long)B * T;
  for (long f = tid; f < frames; f += TALLY_THREADS) {
    const int* __restrict__ s = stats + f * STAT_INTS;
    n_fn += s[0], n_fp += s[1], gt_bg |= s[2];
    if (hit_col[f * K] == 0) ++n_bg, s_bg += (double)hit_iou[f * K];
  }

  n_tp = wave_sum(n_tp), n_switch = wave_sum(n_switch), n_fn = wave_sum(n_fn), n_fp = wave_sum(n_fp), n_bg = wave_sum(n_bg);
  s_thing = wave_sum(s_thing), s_bg = wave_sum(s_bg);
  gt_bg = __any(gt_bg);
  if (lane == 0) {
    part_n[wave][0] = n_tp, part_n[wave][1] = n_switch, part_n[wave][2] = n_fn, part_n[wave][3] = n_fp, part_n[wave][4] = n_bg;
    part_s[wave][0] = s_thing, part_s[wave][1] = s_bg;
    part_bg[wave] = gt_bg;
  }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < TALLY_WAVES; ++w) {
    n_tp += part_n[w][0], n_switch += part_n[w][1], n_fn += part_n[w][2], n_fp += part_n[w][3], n_bg += part_n[w][4];
    s_thing += part_s[w][0], s_bg += part_s[w][1];
    gt_bg |= part_bg[w];
  }
  const int bits = (*bad ? ERR_RANGE : 0) | (gt_bg ? 0 : ERR_NO_BACKGROUND);
  if (bits) {      // a wrong update adds nothing
    *errors |= bits;
    return;
  }
  // an id switch is one false negative and one false positive; counts go through fp64 as the host path's tally does
  tp[0] = __fadd_rn(tp[0], (float)(double)n_bg);
  iou[0] = __fadd_rn(iou[0], (float)s_bg);
  tp[1] = __fadd_rn(tp[1], (float)(double)n_tp);
  iou[1] = __fadd_rn(iou[1], (float)s_thing);
  fp[1] = __fadd_rn(fp[1], (float)(double)(n_fp + n_switch));
  fn[1] = __fadd_rn(fn[1], (float)(double)(n_fn + n_switch));
}

}  // namespace
}  // namespace sf

using namespace sf;

extern "C" {

size_t sf_panoptic_score_ws_bytes(int B, int T, int K) {
  ScoreLayout L;
  return score_layout(B, T, K, &L) ? L.total : 0;
}

int sf_panoptic_score_fwd(const int64_t* hist, long n_per_frame, int B, int T, int K, int n_classes, int track, const int32_t* bad,
                          float* iou, float* true_positive, float* false_positive, float* false_negative, int32_t* errors, void* ws,
                          size_t ws_bytes, void* stream) {
  ScoreLayout L;
  if (!hist || !bad || !iou || !true_positive || !false_positive || !false_negative || !errors || !ws) return SF_ERR_INVALID;
  if (!score_layout(B, T, K, &L) || n_classes < 2 || n_per_frame < 1 || n_per_frame >= PQ_MAX_PIXELS) return SF_ERR_INVALID;
  if (ws_bytes < L.total) return SF_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* p = static_cast<char*>(ws);
  int* hit_col = reinterpret_cast<int*>(p);
  float* hit_iou = reinterpret_cast<float*>(p + L.col_bytes);
  int* stats = reinterpret_cast<int*>(p + L.col_bytes + L.iou_bytes);
  hipLaunchKernelGGL(panoptic_frame_kernel, dim3((unsigned)L.frames), dim3(FRAME_THREADS), 0, st, reinterpret_cast<const long long*>(hist), K,
                     hit_col, hit_iou, stats);
  if (hipGetLastError() != hipSuccess) return SF_ERR_LAUNCH;
  hipLaunchKernelGGL(panoptic_tally_kernel, dim3(1), dim3(TALLY_THREADS), 0, st, hit_col, hit_iou, stats, B, T, K, track != 0, bad, iou,
                     true_positive, false_positive, false_negative, errors);
  return hipGetLastError() == hipSuccess ? SF_OK : SF_ERR_LAUNCH;
}

}  // extern "C"
