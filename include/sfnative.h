/* sfnative.h — C ABI of libsfnative.so: the MI355X (gfx950) native GRU-ODE future-state path of
 * StreamingFlow.  Every entry point takes raw device pointers, sizes and a hipStream_t (passed as
 * void*), enqueues work on that stream and returns 0 on success or a negative sf_status.  No
 * entry point allocates, synchronises or keeps global mutable state, so a caller may capture any
 * sequence of them into a hipGraph (sf_graph_* below).
 *
 * Process model: one process per GPU and one host thread launching on a device at a time (the only process-wide
 * state are first-launch flags per device for the kernels' dynamic-LDS attribute and the opt-in profiler / debug
 * stamps below); calls on different streams of one device may be enqueued from that thread and overlap.
 *
 * The reference (synsin0/StreamingFlow) is pure Python/PyTorch on this path — it has no FFI.  The
 * functions below are therefore the operator boundary a maintainer would bind (ctypes stub in
 * INTEGRATION.md); each cites the reference function it replaces (paths relative to the reference
 * root).
 *
 * Data layout.  Activations are fp32 NHWC: a tensor of n images is [n][H][W][C] contiguous, C a
 * multiple of 8.  The reference API is NCHW; sf_nchw_to_nhwc / sf_nhwc_to_nchw convert at the
 * module boundary.
 *
 * Packed convolution weights (sf_conv_w).  A reference Conv2d weight [cout][cin][kh][kw] is stored
 * as w[cout_pad][kh*kw*cin_pad] with k = (ky*kw + kx)*cin_pad + c, cin_pad = round_up(cin, 32),
 * cout_pad = round_up(cout, 16), zero filled.  cin = c0 + c1 is the channel concat of the (up to)
 * two input tensors a layer reads.  scale/bias hold the per-output-channel affine applied to the
 * accumulator (conv bias, eval-mode BatchNorm fold, or LayerNorm weight/bias), length cout_pad.
 * ConvTranspose2d(k3,s1,p1) layers are stored as the equivalent convolution (spatially flipped,
 * in/out swapped).  The last p_model convolution is stored with its output rows interleaved
 * (row 16T+4g+r  <->  r<2: loc channel 8T+2g+r, r>=2: raw-scale channel 8T+2g+r-2).
 */
#ifndef SFNATIVE_H
#define SFNATIVE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum sf_status {
  SF_OK = 0,
  SF_ERR_INVALID = -1,    /* bad argument (null pointer, unsupported shape) */
  SF_ERR_WORKSPACE = -2,  /* workspace too small */
  SF_ERR_LAUNCH = -3,     /* HIP launch / runtime error */
  SF_ERR_UNSUPPORTED = -4
} sf_status;

enum { SF_ACT_NONE = 0, SF_ACT_LRELU = 1, SF_ACT_RELU = 2, SF_ACT_TANH = 3, SF_ACT_SIGMOID = 4, SF_ACT_GELU = 5 };
enum { SF_SOLVER_EULER = 0, SF_SOLVER_MIDPOINT = 1, SF_SOLVER_RK4 = 2 };
enum { SF_OP_JUMP = 0, SF_OP_STEP = 1 };
/* One coefficient record per ODE step, fp32, computed on the host in float64 and rounded once:
 * {dt, dt/2, dt/6, dt/3,  dt/2, dt/6,  dt/2, dt/3,  dt, dt/3,  dt/6, 0} (the last 8 = RK4 stage pairs) */
#define SF_COEF_STRIDE 12

typedef struct sf_conv_w {
  const float* w;
  const float* scale; /* may be NULL (= 1) */
  const float* bias;  /* may be NULL (= 0) */
  int32_t cout, cout_pad, c0, c1, cin_pad, kh, kw, dil, stride, pad, act;
  int32_t reserved;
  /* optional, NULL unless packed with SF_PACK_BF16X3: the same packed weights split into bf16 pieces for the opt-in
   * "bf16x3" math mode (a = hi + lo; a*b ~ hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16, fp32 accumulators).  Layers
   * whose struct carries it run the split-bf16 K loop where a kernel has one; results then differ from the exact-fp32
   * path by ~1e-5 (profiles/r03_bf16x3_*).  The default build of every module leaves it NULL: exact fp32. */
  const void* w_bf16x3;
  /* optional, NULL unless packed with SF_PACK_WINOGRAD and the layer qualifies (3x3, stride 1, pad 1, no dilation, cin a multiple of
   * 32, cout_pad a multiple of 64): the packed weights in Winograd F(2x2, 3x3) form, U = G g G^T as [cin/16][16][cout_pad][16].
   * Launches with enough pixels then run csrc/conv_wino.hip: exact fp32 arithmetic, 2.25x fewer multiplies, different rounding
   * (<= 7e-6 on the BEV outputs, profiles/r04_winograd_accuracy_study.json). */
  const float* w_wino;
} sf_conv_w;

/* ---- weight packing on the device (load time) ---------------------------------------------------------------------
 * sf_pack_conv packs ONE reference convolution into `blob` (device memory of at least sf_pack_conv_bytes) and fills
 * `out` with pointers into it:
 *   weight     Conv2d weight [cout][cin][kh][kw] fp32 (device); with SF_PACK_TRANSPOSED a ConvTranspose2d(k, s1, p=(k-1)/2)
 *              weight [cin][cout][kh][kw], stored as the equivalent convolution; with SF_PACK_FOLD_DUP a weight
 *              [cout][2*cin][kh][kw] of a layer that reads cat[s, s], folded to W[:, :cin] + W[:, cin:]
 *              (temporal_ode_bayes.py:148-161: gru_cell_2(s, s)); with SF_PACK_INTERLEAVE the output rows of the last
 *              p_model convolution are interleaved (loc, loc, raw, raw) for the sampling epilogue
 *   affine     either eval-mode BatchNorm2d buffers (bn_weight / bn_bias / bn_mean / bn_var, bn_eps: scale = w / sqrt(var + eps),
 *              bias = b - mean * scale + conv_bias * scale) or a plain per-channel `scale` (LayerNorm weight; NULL = 1) and
 *              `conv_bias` (NULL = 0)
 *   c0 + c1 = cin: channels read from the first / second input tensor; pad < 0 = "same" ((kh-1)*dil/2).
 * The composite structs below (sf_gru_w ... sf_deeplab_w) are assembled from packed convolutions by plain struct
 * assignment; [update ; reset] gate pairs are packed from the two weights stored one after the other (cout = 2*hidden). */
enum { SF_PACK_TRANSPOSED = 1, SF_PACK_FOLD_DUP = 2, SF_PACK_INTERLEAVE = 4, SF_PACK_BF16X3 = 8, SF_PACK_WINOGRAD = 16 };

/* conv-GRU cell: SpatialGRU.gru_cell (streamingflow/layers/temporal.py:44-57) */
typedef struct sf_gru_w {
  sf_conv_w gates;    /* [conv_update ; conv_reset] stacked on cout (2*hidden), sigmoid */
  sf_conv_w cand;     /* conv_state_tilde */
  sf_conv_w decoder;  /* 1x1 conv_decoder, w == NULL if absent */
} sf_gru_w;

/* DualGRUODECell / DualGRUCell (streamingflow/layers/temporal_ode_bayes.py:64-161 / 211-305) */
typedef struct sf_dual_w {
  sf_conv_w gates1, cand1;   /* gru_cell_1 on cat[x, s] */
  sf_conv_w gates2, cand2;   /* gru_cell_2 on cat[s, s]; gates2 has the duplicate input folded (cin = C) */
  sf_conv_w dec2;            /* conv_decoder_2 */
  sf_conv_w tg7, tgproj;     /* trusting_gate.0.layers.0 (7x7, LN in scale/bias), .projection.0 (1x1, GELU) */
  sf_conv_w tg1, tg3;        /* .layers.3 (1x1 + LN), .layers.6 (3x3 + LN) */
  const float* w_logit;      /* trusting_gate.1: [2][C] */
  int32_t C;
  /* optional (w == NULL: unused): the two input halves of gates1 packed on their own — gates1_x = W[:, :C] on x with the
   * bias and the sigmoid, gates1_s = W[:, C:] on s with neither.  In a rollout the s half is accumulated beside the
   * previous infer_state (the state is known five launches before x is) and added to the x half's sums. */
  sf_conv_w gates1_x, gates1_s;
} sf_dual_w;

/* ResBlock (streamingflow/layers/res_models.py:52-79) */
typedef struct sf_res_w {
  sf_conv_w conv1, conv2, proj; /* proj.w == NULL when in == out */
} sf_res_w;

/* ConvNet p_model + rsample (res_models.py:168-180, models/model_utils.py:60-109) */
typedef struct sf_pmodel_w {
  sf_res_w rb0, rb1;
  const float *se0_fc0, *se0_fc2, *se1_fc0, *se1_fc2; /* SELayer fc weights [2C/8][2C], [2C][2C/8] */
  sf_conv_w last;                                     /* interleaved rows, LeakyReLU */
  int32_t C;
} sf_pmodel_w;

/* SmallEncoder / SmallDecoder (res_models.py:82-147) */
typedef struct sf_encoder_w { sf_res_w blocks[5]; sf_conv_w last; int32_t C, F; } sf_encoder_w;
typedef struct sf_decoder_w { sf_conv_w first; sf_res_w blocks[5]; sf_conv_w last0, last1; int32_t C, F; } sf_decoder_w;

/* ConvNeXt Block (streamingflow/layers/convolutions.py:310-346) */
typedef struct sf_convnext_w {
  const float *dw_w /*[49][C]*/, *dw_b, *ln_w, *ln_b;
  sf_conv_w pw1, pw2; /* pw2: scale = gamma, bias = gamma*b2 */
  int32_t C;
} sf_convnext_w;

/* DeepLabHead / ASPP (convolutions.py:217-280) */
typedef struct sf_deeplab_w {
  sf_conv_w branch[4];   /* 1x1 and the three dilated 3x3, BN+ReLU */
  const float *pool_w /*[hid][C]*/, *pool_scale, *pool_bias; /* ASPPPooling conv + BN */
  const float* proj_pool_w; /* [hid][hid]: projection weights of the pooled branch */
  sf_conv_w project;     /* 1x1 over the 4 spatial branches (cin = 4*hid), BN+ReLU */
  sf_conv_w conv3, cls;  /* 3x3+BN+ReLU, final 1x1 (+bias) */
  int32_t C, hid;
} sf_deeplab_w;

/* Bottleneck (streamingflow/layers/convolutions.py:65-172 == beverse basic_modules.py:68-178) */
typedef struct sf_bottleneck_w {
  sf_conv_w down, conv, up, proj; /* BN folded; proj.w == NULL for the identity skip */
  int32_t downsample;
} sf_bottleneck_w;

/* Bottleblock (streamingflow/layers/convolutions.py:348-380), see sf_bottleblock_fwd */
typedef struct sf_bottle_w {
  sf_conv_w c7, c1, c3; /* layers.0 / .3 / .6 with the LayerNorm weight / bias in scale / bias */
  sf_conv_w proj;       /* projection.0; proj.w == NULL when in == out */
} sf_bottle_w;

int sf_version(void);
const char* sf_status_string(int status);
/* Persistent "flow" form of the single-latent rollout (csrc/conv_sp.hip: sp_flow_kernel): every launch group of sf_nnfo_rollout_* runs
 * as a phase of ONE resident launch ordered by tile-level dataflow — bitwise the results of the launch-per-layer form, ~5 % less time
 * per ODE step.  It needs every CU of an otherwise IDLE device (one workgroup per CU must be resident at once; waits are bounded, so a
 * device shared with another process or stream ends the launch with NaN results — see sf_flow_errors — instead of hanging): opt-in.  on: 1 / 0, -1 = the
 * SF_PERSIST environment variable (default 0).  Returns the previous setting.  Process-wide; set it before capturing a graph. */
int sf_set_flow_mode(int on);
/* Every dependency wait of the flow kernel is bounded (SF_FLOW_TIMEOUT polls).  A rollout in which one gave up does NOT return its
 * half-finished results: a tail kernel of the same call (captured with it in a graph) overwrites out_states / final_state with NaN.
 * sf_flow_errors synchronises `stream` and returns the number of timed-out waits of the calling thread's most recent persistent
 * rollout (0 = healthy), SF_ERR_INVALID if the thread's most recent rollout was not a persistent one.  The launch-per-layer form (the
 * default) has no such waits.
 * Lifetime and threads: the count lives in the WORKSPACE the caller passed to that rollout (the library owns no device memory), and
 * "most recent" means most recently ENQUEUED BY THIS THREAD — call sf_flow_errors from the thread that enqueued the rollout, before
 * that workspace is freed or reused, and not for a graph replay (a replay enqueues nothing: read the outputs — a rollout with a
 * timed-out wait has NaN in every element of out_states and final_state — as streamingflow_amd's checked mode does). */
int sf_flow_errors(void* stream);

/* ---- ABI guard ---------------------------------------------------------------------------------------------------------
 * The structs above are passed by pointer and sf_conv_w is embedded by value in every composite, so a host compiled
 * against an older header would hand the library mis-sized structs (round 3 grew sf_conv_w from 72 to 80 bytes and
 * sf_dual_w by two members; version 6 added two more to sf_dual_w, the input halves of the trusting gate's 7x7, and version 7
 * removed them again).  SF_ABI_VERSION changes whenever a public struct changes layout.  A host calls sf_abi_check_header()
 * once after loading the library — it passes the sizes ITS compiler saw — and must not call anything else unless it returns SF_OK; bindings without a C compiler (ctypes, cgo, JNI) compare their own struct sizes
 * with sf_abi_sizeof() the same way (streamingflow_amd/_lib.py does, INTEGRATION.md shows it).  Hosts must zero-initialise
 * the structs (optional members are "NULL = absent") and recompile when SF_ABI_VERSION changes. */
#define SF_ABI_VERSION 7
enum {
  SF_STRUCT_CONV_W = 0, SF_STRUCT_GRU_W, SF_STRUCT_DUAL_W, SF_STRUCT_RES_W, SF_STRUCT_PMODEL_W, SF_STRUCT_ENCODER_W,
  SF_STRUCT_DECODER_W, SF_STRUCT_CONVNEXT_W, SF_STRUCT_DEEPLAB_W, SF_STRUCT_BOTTLENECK_W, SF_STRUCT_BOTTLE_W, SF_STRUCT_COUNT
};
int sf_abi_version(void);                 /* the library's SF_ABI_VERSION */
size_t sf_abi_sizeof(int which);          /* sizeof(struct SF_STRUCT_<which>) as the library was compiled; 0 for an unknown id */
/* SF_OK when abi_version and all n = SF_STRUCT_COUNT sizes equal the library's, SF_ERR_INVALID otherwise */
int sf_abi_check(int abi_version, const size_t* struct_sizes, int n);
static inline int sf_abi_check_header(void) {
  const size_t sizes[SF_STRUCT_COUNT] = {sizeof(sf_conv_w),     sizeof(sf_gru_w),      sizeof(sf_dual_w),     sizeof(sf_res_w),
                                         sizeof(sf_pmodel_w),   sizeof(sf_encoder_w),  sizeof(sf_decoder_w),  sizeof(sf_convnext_w),
                                         sizeof(sf_deeplab_w),  sizeof(sf_bottleneck_w), sizeof(sf_bottle_w)};
  return sf_abi_check(SF_ABI_VERSION, sizes, SF_STRUCT_COUNT);
}

/* layout: [n][C][HW] <-> [n][HW][C] */
int sf_nchw_to_nhwc(const float* src, float* dst, int n, int C, int HW, void* stream);
int sf_nhwc_to_nchw(const float* src, float* dst, int n, int C, int HW, void* stream);
/* the same with the n images src_stride / dst_stride floats apart: frames read out of / written into a
 * [B][T][C][H][W] tensor (future_prediction_ode.py:36-49, :63-64) without an intermediate stack */
int sf_nchw_to_nhwc_strided(const float* src, size_t src_stride, float* dst, size_t dst_stride, int n, int C, int HW,
                            void* stream);
int sf_nhwc_to_nchw_strided(const float* src, size_t src_stride, float* dst, size_t dst_stride, int n, int C, int HW,
                            void* stream);

/* generic fused conv (test hook and building block): y = act(conv(cat[in0,in1])*scale + bias) + add */
int sf_conv2d_fwd(const sf_conv_w* w, const float* in0, const float* in1, const float* add, float* out,
                  int n_img, int Hin, int Win, int in_up, void* stream);

/* benchmarking aid: sf_conv2d_fwd enqueued `reps` times from C++; ws may be NULL */
int sf_conv2d_repeat(const sf_conv_w* w, const float* in0, const float* in1, const float* add, float* out,
                     int n_img, int Hin, int Win, int in_up, int reps, float* ws, size_t ws_bytes, void* stream);

/* ---- Workspaces of the model entry points below (sf_gru_cell_fwd ... sf_dist_head_fwd, sf_channel_mean_fwd, sf_camera_neck_fwd, sf_effnet_trunk_fwd) ----------
 * Each takes caller-owned scratch `ws` of `ws_bytes` bytes and has a size query beside it.  The query IS the call's own layout,
 * measured: it depends on the query's arguments only (and, where said, on the flow mode in force), never on the weights; a call derives
 * those arguments from its weights and carves exactly what the query returns for them.  So exactly that size is enough, and with less
 * (or ws NULL) the call returns SF_ERR_WORKSPACE before it has enqueued or written anything — whatever the call at hand would have
 * used of it (a block without projection, a head without pooling).  The entry points whose scratch is optional say so
 * (sf_conv2d_ex_fwd, the sparse convolutions, sf_conv2d_repeat: NULL or short runs without split-K and is not refused). */

/* SpatialGRU.gru_cell — temporal.py:44-57.  x [P][Cx], s [P][C] -> out [P][C] (P = n*H*W) */
int sf_gru_cell_fwd(const sf_gru_w* w, const float* x, const float* s, float* out, int n_img, int H, int W,
                    float* ws, size_t ws_bytes, void* stream);
size_t sf_gru_cell_ws_bytes(int C, int n_img, int H, int W);   /* exactly that size is enough; less (or ws NULL): SF_ERR_WORKSPACE, nothing enqueued or written */
/* SpatialGRUODECell.forward — temporal_ode_bayes.py:35-61 (defined, unused by the shipped model):
 * dh = u * (h~ - s), candidate = conv + BN + ReLU.  Same workspace as sf_gru_cell_fwd. */
int sf_gru_ode_cell_fwd(const sf_gru_w* w, const float* x, const float* s, float* out, int n_img, int H, int W,
                        float* ws, size_t ws_bytes, void* stream);

/* SpatialGRU.forward — temporal.py:26-42 on n_img samples at once.
 * x [T][n_img][H*W][Cx], state0 [n_img][H*W][C] -> out [T][n_img][H*W][Cx] */
int sf_spatial_gru_fwd(const sf_gru_w* w, const float* x, const float* state0, float* out, int T, int n_img, int H,
                       int W, float* ws, size_t ws_bytes, void* stream);
size_t sf_spatial_gru_ws_bytes(int C, int n_img, int H, int W);   /* exactly that size is enough; less (or ws NULL): SF_ERR_WORKSPACE, nothing enqueued or written */

/* The latent-space operators below take n_img >= 1 samples ([n_img][H][W][C] tensors) that are
 * processed as one pixel space: the reference handles one sample per call (its dual cell is only
 * well defined at batch 1); batching samples here is what fills the chip at a 50x50 latent. */

/* DualGRUODECell.forward (derivative != 0) / DualGRUCell.forward (derivative == 0) —
 * temporal_ode_bayes.py:92-131 / :239-275, fused with the integrator update:
 *   derivative: out = base + coef[0]*(cur - s); optional out2 = (acc2 ? out2 : base) + coef[1]*(cur - s)
 *   jump:       out = cur
 * coef points at device fp32 scalars (shared by all images).  out may not alias x/s/base. */
int sf_dual_cell_fwd(const sf_dual_w* w, const float* x, const float* s, float* out, int derivative,
                     const float* base, const float* coef, float* out2, int acc2, int n_img, int H, int W,
                     float* ws, size_t ws_bytes, void* stream);
size_t sf_dual_cell_ws_bytes(int C, int n_img, int H, int W);   /* exactly that size is enough; less (or ws NULL): SF_ERR_WORKSPACE, nothing enqueued or written */

/* The tail of both dual cells on given branch states — temporal_ode_bayes.py:122-131 / :266-275 and the loop body of
 * Dual_GRU.forward (layers/temporal.py:118-124): gate = softmax(trusting_gate(cat[r1, r2])); cur = r2*gate0 + r1*gate1;
 * derivative != 0: out = base + coef[0]*(cur - s), else out = cur (s, base, coef may then be NULL).
 * Workspace: sf_dual_cell_ws_bytes. */
int sf_trust_mix_fwd(const sf_dual_w* w, const float* r1, const float* r2, const float* s, float* out, int derivative,
                     const float* base, const float* coef, int n_img, int H, int W, float* ws, size_t ws_bytes, void* stream);

/* Bottleblock.forward — convolutions.py:348-380 on cat[x0, x1] (x1 may be NULL): 7x7 + LN + GELU -> 1x1 + LN + GELU ->
 * 3x3 + LN + GELU, plus projection(x) (1x1 + GELU) or x itself when in == out (then x1 must be NULL).
 * Channel counts of the LayerNorm layers <= 64.  Weights: struct sf_bottle_w, above.  Workspace: the query's cin = c0 + c1 of the 7x7 layer,
 * cout = the 3x3 layer's; the two hidden layers are at most cin / 2 wide (SF_ERR_INVALID otherwise). */
int sf_bottleblock_fwd(const sf_bottle_w* w, const float* x0, const float* x1, float* out, int n_img, int H, int W,
                       float* ws, size_t ws_bytes, void* stream);
size_t sf_bottleblock_ws_bytes(int cin, int cout, int n_img, int H, int W);   /* exactly that size is enough; less (or ws NULL): SF_ERR_WORKSPACE, nothing enqueued or written */

/* NNFOwithBayesianJumps.infer_state — temporal_ode_bayes.py:463-477: p = loc + eps*(softplus(raw)+1e-8).
 * q_out (raw p_model output, [P][2C], reference channel order) may be NULL.  n_img <= 64. */
int sf_infer_state_fwd(const sf_pmodel_w* w, const float* s, const float* eps, float* p_out, float* q_out,
                       int n_img, int H, int W, float* ws, size_t ws_bytes, void* stream);
size_t sf_infer_state_ws_bytes(int C, int n_img, int H, int W);   /* exactly that size is enough; less (or ws NULL): SF_ERR_WORKSPACE, nothing enqueued or written */

/* NNFOwithBayesianJumps.ode_step — temporal_ode_bayes.py:436-461 (euler, midpoint) and the
 * build-defined classical RK4.  coef: one device coefficient record (SF_COEF_STRIDE floats).
 * eps: [n_draws][n_img][H*W][C] with n_draws = 1 (euler), 2 (midpoint), 4 (rk4).  If impute == 0
 * the cell input is zeros (:442-443).  state_out / p_out must not alias state_in / p_in.
 * Workspace: sized for any solver. */
int sf_ode_step_fwd(const sf_dual_w* gru_c, const sf_pmodel_w* pm, int solver, int impute, const float* state_in,
                    const float* p_in, const float* coef, const float* eps, float* state_out, float* p_out,
                    int n_img, int H, int W, float* ws, size_t ws_bytes, void* stream);
size_t sf_ode_step_ws_bytes(int C, int n_img, int H, int W);   /* exactly that size is enough; less (or ws NULL): SF_ERR_WORKSPACE, nothing enqueued or written */

/* The observation/prediction loop of NNFOwithBayesianJumps.forward — temporal_ode_bayes.py:539-604,
 * driven by a schedule computed on the host (streamingflow_amd.schedule); all n_img samples share
 * the op sequence.  ops[2*i] = SF_OP_JUMP (ops[2*i+1] = observation index) or SF_OP_STEP
 * (ops[2*i+1] = step index).  coef: [n_steps][SF_COEF_STRIDE] (coef_per_image == 0) or
 * [n_steps][n_img][SF_COEF_STRIDE] (per-sample step sizes).  After op i (1-based count k = i+1)
 * the state is copied to out_states[t] for every target t with sel_nops[t] == k (:606-622).
 * hx_obs [n_obs][n_img][H*W][C]; eps [n_draws][n_img][H*W][C] in reference draw order;
 * out_states [n_targets][n_img][H*W][C]; final_state [n_img][H*W][C] (may be NULL). */
int sf_nnfo_rollout_fwd(const sf_dual_w* gru_c, const sf_dual_w* gru_obs, const sf_pmodel_w* pm, int solver,
                        int impute, const int32_t* ops, int n_ops, const float* hx_obs, const float* eps,
                        const float* coef, int coef_per_image, const int32_t* sel_nops, int n_targets,
                        float* out_states, float* final_state, int n_img, int H, int W, float* ws,
                        size_t ws_bytes, void* stream);
/* Throughput mode: the Gaussian noise of every infer_state is generated inside the sampling epilogue instead of being read
 * from an eps tensor (Philox4x32-10, Box-Muller; csrc/sf_math.h).  philox_state: device record {uint64 seed, uint64 offset};
 * the draw of an element is a function of (seed, offset, draw index, pixel, channel) only, so results do not depend on the
 * kernel / tile / batch, and a captured graph gives fresh noise when the host rewrites the 16-byte record between replays.
 * Same distribution as the reference's Normal.rsample (temporal_ode_bayes.py:474-476), different stream: parity tests use
 * the eps-fed entry points above. */
int sf_nnfo_rollout_philox_fwd(const sf_dual_w* gru_c, const sf_dual_w* gru_obs, const sf_pmodel_w* pm, int solver, int impute,
                               const int32_t* ops, int n_ops, const float* hx_obs, const uint64_t* philox_state, const float* coef,
                               int coef_per_image, const int32_t* sel_nops, int n_targets, float* out_states, float* final_state,
                               int n_img, int H, int W, float* ws, size_t ws_bytes, void* stream);
/* Resumable forms: the same rollout cut into SEGMENTS that separate calls run one after the other (a streaming caller appends one
 * observation per call and forks predictions from the carried state; streamingflow_amd.StreamSession).  The arguments of the entry
 * points above, plus:
 *   state_in, p_in  [n_img][H*W][C]: latent state and imputed input the segment starts from; NULL = zeros (both NULL, draw_base 0 and
 *                   the three outputs below NULL: exactly the entry points above, which are implemented that way).  Never written.
 *   draw_base       index of the segment's first noise draw in the numbering of the whole rollout.  The Philox form keys draw k of the
 *                   segment by draw_base + k under the same {seed, offset} record.  eps is the segment's OWN tensor — the caller passes
 *                   the whole rollout's pointer advanced by draw_base draws — and draw k of the segment reads eps[k].
 *   p_out           [n_img][H*W][C] or NULL: the imputed input after the last op.  Non-NULL keeps the infer_state pass of the last op,
 *                   which the entry points above skip; the next segment may start with a step that reads it.
 *   carry_in/_out   sf_nnfo_rollout_carry_bytes each, or NULL.  With IMPUTE the unsplit rollout computes part of the ODE cell that follows
 *                   an infer_state inside that infer_state's launches, and the launch grouping fixes the split-K summation order.  A segment
 *                   given carry_out (needs p_out) does the same for the cell behind the boundary and the next segment, given it as
 *                   carry_in (needs state_in and p_in of the same boundary), consumes it when its first op is a step: the segments then
 *                   reproduce the unsplit rollout BITWISE.  With NULL the boundary cell is computed on its own: same arithmetic,
 *                   a different summation order (differences of rounding size).  Opaque; valid only next to the state_in / p_in it was
 *                   written with.
 * sel_nops counts the ops of THIS segment (1-based); n_targets may be 0 (sel_nops, out_states NULL).  hx_obs holds the segment's
 * own observations (a jump's argument indexes it) and may be NULL for a segment without jumps.  n_ops may be 0: final_state and
 * p_out are then copies of state_in and p_in, and carry_out must be NULL (SF_ERR_INVALID: there is no infer_state to compute it
 * beside; keep the carry the boundary already has).
 * Aliasing: final_state may be state_in, p_out may be p_in and carry_out may be carry_in (in-place update of a carried boundary): the
 * inputs are consumed by the segment's first cell, the outputs written after its last.  Otherwise outputs must not overlap inputs,
 * out_states or the workspace.
 * Enqueue only (no allocation, no synchronisation): a segment is captured into a graph like any rollout.
 * Persistent flow (sf_set_flow_mode / SF_PERSIST): a call with state_in, p_in or p_out runs in the launch-per-layer form whatever the
 * switch says (never from zeros, never with bounded waits); sf_flow_errors then reports SF_ERR_INVALID as for any launch-path rollout.
 * The forked 7x7 stream (SF_FORK7) no longer exists in the library, so there is no second rollout form a segment could take. */
int sf_nnfo_rollout_resume_fwd(const sf_dual_w* gru_c, const sf_dual_w* gru_obs, const sf_pmodel_w* pm, int solver, int impute,
                               const int32_t* ops, int n_ops, const float* hx_obs, const float* eps, const float* coef,
                               int coef_per_image, const int32_t* sel_nops, int n_targets, float* out_states, float* final_state,
                               const float* state_in, const float* p_in, const float* carry_in, int draw_base, float* p_out,
                               float* carry_out, int n_img, int H, int W, float* ws, size_t ws_bytes, void* stream);
int sf_nnfo_rollout_resume_philox_fwd(const sf_dual_w* gru_c, const sf_dual_w* gru_obs, const sf_pmodel_w* pm, int solver, int impute,
                                      const int32_t* ops, int n_ops, const float* hx_obs, const uint64_t* philox_state,
                                      const float* coef, int coef_per_image, const int32_t* sel_nops, int n_targets, float* out_states,
                                      float* final_state, const float* state_in, const float* p_in, const float* carry_in,
                                      int draw_base, float* p_out, float* carry_out, int n_img, int H, int W, float* ws,
                                      size_t ws_bytes, void* stream);
size_t sf_nnfo_rollout_carry_bytes(int C, int n_img, int H, int W);   /* exactly that size is enough (carry_in / carry_out come without a size: not checked) */
int sf_infer_state_philox_fwd(const sf_pmodel_w* w, const float* s, const uint64_t* philox_state, int draw, float* p_out, float* q_out,
                              int n_img, int H, int W, float* ws, size_t ws_bytes, void* stream);

/* workspace of the four sf_nnfo_rollout_*_fwd.  It holds the persistent flow's tables (5 MB) exactly while the flow mode is on: query and
 * call must see the same mode (sf_set_flow_mode / SF_PERSIST) */
size_t sf_nnfo_rollout_ws_bytes(int C, int n_img, int H, int W);   /* exactly that size is enough; less (or ws NULL): SF_ERR_WORKSPACE, nothing enqueued or written */

/* SmallEncoder.forward — res_models.py:98-109: [n][H][W][C] -> [n][H/4][W/4][C] */
int sf_small_encoder_fwd(const sf_encoder_w* w, const float* x, float* out, int n, int H, int W,
                         float* ws, size_t ws_bytes, void* stream);
size_t sf_small_encoder_ws_bytes(int C, int F, int n, int H, int W);   /* exactly that size is enough; less (or ws NULL): SF_ERR_WORKSPACE, nothing enqueued or written */
/* SmallDecoder.forward — res_models.py:134-147: [n][h][w][C] -> [n][4h][4w][C] */
int sf_small_decoder_fwd(const sf_decoder_w* w, const float* z, float* out, int n, int h, int wd,
                         float* ws, size_t ws_bytes, void* stream);
size_t sf_small_decoder_ws_bytes(int C, int F, int n, int h, int w);   /* exactly that size is enough; less (or ws NULL): SF_ERR_WORKSPACE, nothing enqueued or written */

/* ConvNeXt Block.forward — convolutions.py:333-346 */
int sf_convnext_block_fwd(const sf_convnext_w* w, const float* x, float* out, int n, int H, int W,
                          float* ws, size_t ws_bytes, void* stream);
size_t sf_convnext_block_ws_bytes(int C, int n, int H, int W);   /* exactly that size is enough; less (or ws NULL): SF_ERR_WORKSPACE, nothing enqueued or written */
/* DeepLabHead.forward — convolutions.py:272-280 */
int sf_deeplab_head_fwd(const sf_deeplab_w* w, const float* x, float* out, int n, int H, int W,
                        float* ws, size_t ws_bytes, void* stream);
size_t sf_deeplab_head_ws_bytes(int C, int hid, int n, int H, int W);   /* exactly that size is enough; less (or ws NULL): SF_ERR_WORKSPACE, nothing enqueued or written */
/* the same, the classifier writing the boundary's planar layout itself: image i as [cout][H][W] planes at
 * out + (i / group) * stride_major + (i % group) * stride_minor floats.  Frames (t, b) of a [T][B] run into the reference's
 * [B][T][C][H][W] result (future_prediction_ode.py:62-64): group = B, stride_major = C*H*W, stride_minor = T*C*H*W — no
 * transpose launches after the head.  Same workspace as sf_deeplab_head_fwd. */
int sf_deeplab_head_planar_fwd(const sf_deeplab_w* w, const float* x, float* out, int n, int H, int W, int group,
                               size_t stride_major, size_t stride_minor, float* ws, size_t ws_bytes, void* stream);

/* Bottleneck.forward — convolutions.py:164-172: [n][H][W][Cin] -> [n][Ho][Wo][Cout].  Workspace: the query's Cin / Cout are the first / last
 * layer's; the hidden layers are at most Cin / 2 wide (SF_ERR_INVALID otherwise) */
int sf_bottleneck_fwd(const sf_bottleneck_w* w, const float* x, float* out, int n, int H, int W, float* ws,
                      size_t ws_bytes, void* stream);
size_t sf_bottleneck_ws_bytes(int Cin, int Cout, int n, int H, int W);   /* exactly that size is enough; less (or ws NULL): SF_ERR_WORKSPACE, nothing enqueued or written */
/* elementwise LogSigmoid, min(x, 0) - log1p(exp(-|x|)): the decoder of DistributionModule(method='BERNOULLI')
 * (streamingflow/models/distributions.py:29-33, :46-47) */
int sf_logsigmoid_fwd(const float* x, float* out, size_t n, void* stream);
/* last_conv of DistributionModule / SpatialDistributionModule — beverse motion_modules.py:34-46,74-88
 * (and streamingflow/models/distributions.py:35-49 with clamp == 0): [global avg-pool +] 1x1 conv + bias,
 * second half of the channels clamped to [lo, hi].  Workspace: required with and without global_pool */
int sf_dist_head_fwd(const sf_conv_w* w, const float* enc, float* out, int n, int H, int W, int global_pool,
                     int clamp, float lo, float hi, float* ws, size_t ws_bytes, void* stream);
size_t sf_dist_head_ws_bytes(int C, int n);   /* exactly that size is enough; less (or ws NULL): SF_ERR_WORKSPACE, nothing enqueued or written */

/* ---- N3 building blocks: BEV Decoder (streamingflow/models/decoder.py:8-140) ---------------------------
 * The decoder is a ResNet-18 U-Net of plain convolutions; its host mirror
 * (streamingflow_amd/models/decoder.py) drives these two entry points layer by layer.
 * sf_conv2d_ex_fwd: sf_conv2d_fwd with channel-sliced operands (in0/in1/add/out may be channel ranges
 * of wider NHWC tensors: *_cs = channel stride of the tensor, out_co = first output channel) and
 * `act_after_add` (torchvision BasicBlock: relu(bn2(conv2(.)) + identity)); ws/ws_bytes: optional
 * split-K scratch (sf_conv2d_ex_ws_bytes()), may be NULL. */
int sf_conv2d_ex_fwd(const sf_conv_w* w, const float* in0, int in0_cs, const float* in1, int in1_cs, const float* add,
                     int add_cs, int act_after_add, float* out, int out_cs, int out_co, int n_img, int Hin, int Win,
                     int in_up, float* ws, size_t ws_bytes, void* stream);
size_t sf_conv2d_ex_ws_bytes(void);
/* UpsamplingAdd — convolutions.py:204-215: out [n][2H][2W][C] = bilinear_x2(in, align_corners=False) + skip.
 * (The 1x1 conv + BatchNorm of the module commute with the interpolation and run before it, at the
 * low resolution: a quarter of the MACs.) */
int sf_upsample_bilinear2_add_fwd(const float* in, const float* skip, float* out, int n, int Hin, int Win, int C,
                                  void* stream);

/* TemporalBlock helpers (streamingflow/layers/temporal.py:394-432, :435-490): per-image channel means of
 * an NHWC tensor (the spatial part of PyramidSpatioTemporalPooling's AvgPool3d) and the broadcast of a
 * per-image channel vector over a channel slice (its bilinear upsampling of a 1x1 map is a constant). */
size_t sf_channel_mean_ws_bytes(int C, int n);   /* exactly that size is enough; less (or ws NULL): SF_ERR_WORKSPACE, nothing enqueued or written */
int sf_channel_mean_fwd(const float* x, float* out, int n, int HW, int C, float* ws, size_t ws_bytes, void* stream);
int sf_broadcast_channels_fwd(const float* vec, float* out, int n, int HW, int k, int out_cs, int out_co, void* stream);

/* ---- N1: camera lift-splat voxel pooling ---------------------------------------
 * Layouts: frustum point p = ((cam*D + d)*fH + h)*fW + w of batch element b, points of a call are
 * numbered b-major; BEV cell id = ((b*Z + z)*X + x)*Y + y; pooled output [n_cells][C] = [B][Z][X][Y][C]
 * (the reference kernel's own output layout, NHWC for Z == 1).  `lo`, `res` (3 floats) and `dim`
 * (X, Y, Z) are HOST arrays; lo = bev_start_position - bev_resolution / 2 evaluated in fp32. */

/* bev_pool_forward — mmdet3d/ops/bev_pool/src/bev_pool.cpp:26-49 + bev_pool_cuda.cu:20-42: x [n][c]
 * already in sorted order, geom_feats [n][4] = (x, y, z, b) int32, one interval per occupied cell;
 * out [b][d][h][w][c] is zero-filled, each interval is summed in the given order (fp32, sequential:
 * bit-identical to the reference kernel). */
int sf_bev_pool_fwd(const float* x, const int32_t* geom_feats, const int32_t* interval_lengths,
                    const int32_t* interval_starts, int n, int c, int n_intervals, int b, int d, int h, int w,
                    float* out, void* stream);

/* Quantise + filter + rank + sort of streamingflow.bev_pool (streamingflow.py:353-368) and
 * bev_pool() (bev_pool.py:85-93), without host round trips: geom [n_points][3] float ->
 * order [n_points] (point ids, points of a cell contiguous, ascending inside a cell; points outside
 * the grid last), cell_start [n_cells + 1] (CSR row starts; cell_start[n_cells] = number of kept
 * points), optional coords [n_points][4] = (x, y, z, b) per point in input order, -1 when outside. */
size_t sf_lift_index_ws_bytes(int n_points, int n_cells);
int sf_lift_index_fwd(const float* geom, int n_points, int n_batch, const float* lo, const float* res,
                      const int32_t* dim, int32_t* coords, int32_t* order, int32_t* cell_start, void* ws,
                      size_t ws_bytes, void* stream);
/* Same index from integer coordinates [n_points][4] = (x, y, z, b) — the input of mmdet3d's
 * bev_pool(feats, coords, B, D, H, W) (bev_pool.py:85-93; its D, H, W are Z, X, Y here). */
int sf_lift_index_coords_fwd(const int32_t* coords, int n_points, int B, int Z, int X, int Y, int32_t* order,
                             int32_t* cell_start, void* ws, size_t ws_bytes, void* stream);
/* Same index, geometry computed in the kernel from the camera rig instead of being read:
 * position = affine[b*n_cam + cam] (3x4 row major, device) applied to (us[w]*ds[d], vs[h]*ds[d], ds[d], 1)
 * — create_frustum (streamingflow.py:149-168), get_geometry (:277-292) and the ego-motion warps of
 * projection_to_birds_eye_view (:386-396) composed by the host into one affine per (frame, camera). */
int sf_lift_index_rig_fwd(const float* affine, const float* us, const float* vs, const float* ds, int n_batch,
                          int n_cam, int D, int fH, int fW, const float* lo, const float* res, const int32_t* dim,
                          int32_t* order, int32_t* cell_start, void* ws, size_t ws_bytes, void* stream);
/* Those affines computed on the device, in one launch a graph can record (N10): intrinsics [b*s*n_cam][3][3] (a general 3x3, inverted by
 * cofactors over the determinant), extrinsics [b*s*n_cam][4][4], future_egomotion [b][s][6] (tx, ty, tz, rx, ry, rz), all fp32 ->
 * affine [b*s*n_cam][12] = R_cam * K^-1 | t_cam, left-multiplied by pose_vec2mat(future_egomotion[b][t]) for t = own frame .. s-2 in
 * that order; fp64 throughout, rounded to fp32 once at the store.  A camera whose determinant is zero or non-finite, or whose inputs
 * (its K, its extrinsics' first three rows, the poses of its chain) hold a non-finite value, gets twelve NaNs — sf_lift_index_rig_fwd
 * sends its points outside the grid — and ORs SF_RIG_BAD_CAMERA into *flags (device, int32; the caller zeroes it and reads it when it
 * chooses to synchronise).  SF_ERR_INVALID, nothing written: a NULL pointer, or b, s or n_cam <= 0. */
#define SF_RIG_BAD_CAMERA 2
int sf_rig_affines_fwd(const float* intrinsics, const float* extrinsics, const float* future_egomotion, int b, int s, int n_cam,
                       float* affine, int32_t* flags, void* stream);

/* Pooling proper (bev_pool_cuda.cu:20-42 over every cell, empty ones included) fused with the temporal
 * blend of projection_to_birds_eye_view (streamingflow.py:419): out = prev*discount + sum (prev NULL:
 * plain sum).  x [n_points][C] is the materialised depth (x) feature tensor in point order. */
int sf_lift_pool_fwd(const float* x, const int32_t* order, const int32_t* cell_start, int n_cells, int C,
                     const float* prev, float discount, float* out, void* stream);
/* Same with the outer product of encoder_forward (streamingflow.py:304-307) folded in:
 * x[p][c] = depth_prob[p] * feat[ray(p)][c]; feat [n_batch*n_cam*fHW][C], depth_prob [n_points]. */
int sf_lift_pool_fused_fwd(const float* feat, const float* depth_prob, int D, int fHW, const int32_t* order,
                           const int32_t* cell_start, int n_cells, int C, const float* prev, float discount,
                           float* out, void* stream);
/* depth.softmax(dim=1) of streamingflow.py:304 on [rows][D][fHW] */
int sf_depth_softmax_fwd(const float* logits, float* prob, int rows, int D, int fHW, void* stream);
/* The same softmax for logits that are still NHWC — rows * fHW pixels of cs floats each, the D logits of a pixel contiguous from channel
 * co (a channel slice of a wider tensor; cs, co multiples of 4, the pointer 16-byte aligned) — written out planar in the same pass:
 * out_logits [rows][D][fHW] (bitwise the input, transposed) and out_prob [rows][D][fHW] = expf(x - max) / sum.  What follows the depth
 * branch of the camera neck: the model returns the planar logits (depth_prediction) and the lift reads the planar probabilities.
 * SF_ERR_UNSUPPORTED, before anything is written: D not a multiple of 4 or D > 128. */
int sf_depth_softmax_planar_fwd(const float* logits_nhwc, int cs, int co, float* out_logits, float* out_prob, int rows, int D, int fHW,
                                void* stream);

/* ---- N7: camera encoder neck (streamingflow/models/encoder.py:107-112, layers/convolutions.py:183-201) --------------------------------
 * Both DeepLabHead + UpsamplingConcat branches (features, depth) of Encoder.get_features_depth after its endpoint selection, on one stream:
 *   head   ONE sf_deeplab_w for both heads, which read the same input: hid = 2 * 64, the branch and pooling weights of the two heads
 *          stacked on cout, projection / 3x3 / classifier block-diagonal, cls.cout = 2 * c_hi = [feature | depth]
 *          (streamingflow_amd/models/encoder.py packs it; the zero blocks contribute exact zeros)
 *   convs  [4] = feature conv1, feature conv2, depth conv1, depth conv2 of the two UpsamplingConcat: 3x3, pad 1, BN + ReLU folded;
 *          conv1 has c0 = c_lo (the /8 endpoint) and c1 = c_hi (its half of the upsampled head output) — cat[x, upsampled], never written
 *   hi [n][H][W][c_hi], lo [n][2H][2W][c_lo]  ->  rays [n * 4HW][C] (NHWC features, the rows the lift gathers), depth_logits and
 *   depth_prob [n][D][4HW] (planar, as sf_depth_softmax_planar_fwd writes them).
 * SF_ERR_INVALID: a NULL tensor pointer or structs that are not such a neck; SF_ERR_UNSUPPORTED (nothing written): D % 4 != 0 or D > 128;
 * SF_ERR_WORKSPACE: ws_bytes < sf_camera_neck_ws_bytes(c_hi, c_lo, C, D, hid, n, H, W) (hid = head->hid; 0 for invalid sizes). */
size_t sf_camera_neck_ws_bytes(int c_hi, int c_lo, int C, int D, int hid, int n, int H, int W);   /* exactly that size is enough; less (or ws NULL): SF_ERR_WORKSPACE, nothing enqueued or written */
int sf_camera_neck_fwd(const sf_deeplab_w* head, const sf_conv_w* convs, const float* hi, const float* lo, float* rays,
                       float* depth_logits, float* depth_prob, int n, int H, int W, float* ws, size_t ws_bytes, void* stream);

/* ---- N8: EfficientNet trunk of the camera encoder (streamingflow/models/encoder.py:64-105; efficientnet_pytorch 0.7.x model.py) ----------------
 * Eval mode, fp32: image [n][3][H][W] (planar != 0) or [n][H][W][3] -> the two endpoints the neck reads, NHWC:
 *   out_hi = reduction_{index + 1} and out_lo = reduction_{index}, by the reference's rule: an endpoint is the tensor in front of every
 *   block that lowers the resolution, and the last block's output is the final one.  Their sizes follow from the pads in the structs.
 * MBConv: expand 1x1 + BN + swish (absent at ratio 1) -> depthwise k x k + BN + swish -> SE (mean over H x W -> reduce 1x1 + bias -> swish
 * -> expand 1x1 + bias -> sigmoid -> scale) -> project 1x1 + BN (+ input).  The SE's channel sums are accumulated in 2^-24 fixed point
 * with integer atomics, so results are bitwise reproducible run to run and between eager and captured runs.
 * Weights: sf_effnet_w over a host array of sf_mbconv_w, both defined in include/sfnative_effnet.h — an extension header with its own
 * layout guard (SF_EFFNET_ABI_VERSION, sf_effnet_abi_sizeof), so the struct set and SF_ABI_VERSION of this header are what they were; the
 * entry points below take them as `const void*`.  A host compares SF_EFFNET_ABI_VERSION with sf_effnet_abi_version() and its struct sizes
 * with sf_effnet_abi_sizeof(SF_EFFNET_STRUCT_*) once after loading (the static inline sf_effnet_abi_check_header of the extension header does).
 * The workspace queries read the integers of the structs only (channel counts, kernel sizes, strides, pads, n_blocks, expand.w as a
 * flag), never device memory.  SF_ERR_UNSUPPORTED, before anything is enqueued: k not 3 or 5, stride not 1 or 2, a channel count that is
 * not a multiple of 8; SF_ERR_INVALID: NULL or misaligned pointers, structs that are no such block, an image too small to reach the endpoint;
 * SF_ERR_WORKSPACE as everywhere. */
#define SF_EFFNET_ABI_VERSION 1
enum { SF_EFFNET_STRUCT_MBCONV_W = 0, SF_EFFNET_STRUCT_EFFNET_W, SF_EFFNET_STRUCT_COUNT };
int sf_effnet_abi_version(void);          /* the library's SF_EFFNET_ABI_VERSION */
size_t sf_effnet_abi_sizeof(int which);   /* sizeof(struct SF_EFFNET_STRUCT_<which>) as the library was compiled; 0 for an unknown id */
size_t sf_effnet_trunk_ws_bytes(const void* w, int n, int H, int W);   /* exactly that size is enough; less (or ws NULL): SF_ERR_WORKSPACE, nothing enqueued or written */
int sf_effnet_trunk_fwd(const void* w, const float* image, int planar, float* out_hi, float* out_lo, int n, int H, int W, float* ws,
                        size_t ws_bytes, void* stream);
/* one MBConv block: x [n][H][W][cin] -> out [n][Ho][Wo][cout], Ho = (H + pad_t + pad_b - k) / stride + 1 */
size_t sf_mbconv_ws_bytes(const void* b, int n, int H, int W);   /* exactly that size is enough; less (or ws NULL): SF_ERR_WORKSPACE, nothing enqueued or written */
int sf_mbconv_fwd(const void* b, const float* x, float* out, int n, int H, int W, float* ws, size_t ws_bytes, void* stream);
/* The trunk's launches on their own (test hooks and building blocks).
 * stem: out [n][Ho][Wo][c_stem].  dwconv: depthwise + BN + swish of block b on x [n][H][W][cexp] -> out [n][Ho][Wo][cexp], and
 * sums [n][cexp] (zeroed by the call) = sum over the image's pixels of llrint(out * 2^24).  se_gate: sums of HW pixels -> gate [n][cexp].
 * pointwise: out [n * HW][cout] = act((x * gate[image]) . w * scale + bias) + residual on a 1x1 pack; gate [n][cin] and residual may be
 * NULL; swish != 0: act = swish, else none. */
int sf_effnet_stem_fwd(const void* w, const float* image, int planar, float* out, int n, int H, int W, void* stream);
int sf_effnet_dwconv_fwd(const void* b, const float* x, float* out, uint64_t* sums, int n, int H, int W, void* stream);
int sf_effnet_se_gate_fwd(const void* b, const uint64_t* sums, float* gate, int n, int HW, void* stream);
int sf_effnet_pointwise_fwd(const sf_conv_w* w, const float* x, const float* gate, const float* residual, float* out, int swish, int n, int HW,
                            void* stream);

/* ---- N9: camera image front end (streamingflow/datas/NuscenesData.py:251-269, utils/geometry.py:9-13) -----------------------------------
 * Decoded frames to the trunk's input: src [n][Hs][Ws][3] uint8 -> PIL's resize((Wr, Hr), BILINEAR) — the antialiased triangle filter in
 * 22-bit fixed point, horizontal then vertical pass with a uint8 image between them (Pillow, Resample.c) — -> crop((l, t, r, b)) in
 * resized coordinates (any box; positions outside the resized image are 0) -> ((float)u / 255 - mean[c]) / std[c].  Bit for bit what PIL
 * and torch (on the CPU) compute.
 * sf_resample_ksize / sf_resample_table — one axis' table as Pillow's precompute_coeffs + normalize_coeffs_8bpc build it, host code, in
 *   double: bounds [out_size][2] = (xmin, n), k [out_size][ksize] int32 (zero past n), ksize = ceil(max(in_size / out_size, 1)) * 2 + 1
 *   (0 for sizes < 1).  SF_ERR_UNSUPPORTED: ksize > SF_IMAGE_FRONTEND_MAX_TAPS (33: downscales up to 16 x).
 * sf_image_frontend_plan — fills host_blob (sf_image_frontend_plan_bytes(...) bytes; 0 for what the plan call refuses) with everything
 *   the kernel reads: a header of 24 int32 words, both axes' tables and the 3 x 256 fp32 normalise table.  Built once per geometry; the
 *   caller uploads the bytes as they are (16-byte aligned) and keeps the host copy: the forward call reads its launch sizes from it.
 *   Header words: 0 magic, 1 Hs, 2 Ws, 3 Hr, 4 Wr, 5 l, 6 t, 7 w = r - l, 8 h = b - t, 9 ksize x, 10 ksize y, 11..13 LDS tile sizes,
 *   14 / 15 word offsets of the x bounds / coefficients, 16 / 17 of the y ones, 18 of the normalise table [c][u], 19 words in all,
 *   20 LDS bytes of a workgroup, 21 rows are 16-byte multiples.  mean, std: HOST arrays of 3 floats.
 *   SF_ERR_INVALID: a NULL pointer, a size < 1 or > 32768, an empty box, a blob too small; SF_ERR_UNSUPPORTED: more taps than the cap.
 * sf_image_frontend_fwd — one launch, no workspace, enqueues only (no allocation, copy, host read of device memory or synchronisation):
 *   out fp32 [n][3][h][w] (planar != 0) or [n][h][w][3]; out_u8 [n][h][w][3] (may be NULL): the resized and cropped image before the
 *   normalisation.  A workgroup stages the source rows and columns its 8 x 64 output tile needs in LDS — 16 bytes per lane when Ws * 3 is
 *   a multiple of 16, byte by byte otherwise — and keeps the image between the two passes there; rows the crop drops are not read.
 *   SF_ERR_INVALID, nothing enqueued: NULL src / out / plan_host / plan_dev, n or a size < 1, sizes that are not the plan's, plan_dev not
 *   16-byte aligned, or src not 16-byte aligned where Ws * 3 is a multiple of 16. */
#define SF_IMAGE_FRONTEND_MAX_TAPS 33
int sf_resample_ksize(int in_size, int out_size);
int sf_resample_table(int in_size, int out_size, int32_t* bounds, int32_t* k);
size_t sf_image_frontend_plan_bytes(int Hs, int Ws, int Hr, int Wr, int l, int t, int r, int b);
int sf_image_frontend_plan(int Hs, int Ws, int Hr, int Wr, int l, int t, int r, int b, const float* mean, const float* std, void* host_blob,
                           size_t blob_bytes);
int sf_image_frontend_fwd(const uint8_t* src, const void* plan_host, const void* plan_dev, float* out, int planar, uint8_t* out_u8, int n,
                          int Hs, int Ws, int h, int w, void* stream);

/* ---- N2 (first half): LiDAR hard voxelisation ------------------------------------------------------
 * hard_voxelize — mmdet3d/ops/voxel/src/voxelization.h:63-85, deterministic GPU path
 * voxelization_cuda.cu:262-420 (same result as voxelization_cpu.cpp:45-102): points [num_points][F]
 * (x, y, z first), voxel_size / coors_range HOST arrays of 3 / 6 floats.  Outputs sized for
 * max_voxels and zero-filled as in voxelize.py:52-54: voxels [max_voxels][max_points][F] (may be NULL),
 * coors [max_voxels][3] = (x, y, z), num_points_per_voxel [max_voxels]; voxel_num: device int = the
 * reference's return value.  mean_feats (may be NULL) [max_voxels][F] = sum over the voxel's points /
 * their number — the reduction streamingflow.voxelize applies right after (streamingflow.py:190-195). */
/* Dynamic voxelisation (mmdet3d/ops/voxel/voxelize.py:46-49, the max_points == -1 / max_voxels == -1 branch of _Voxelization.forward ->
 * dynamic_voxelize; src/voxelization_cpu.cpp:8-43, src/voxelization_cuda.cu:25-60): coors [num_points][3] int32 = the (x, y, z) voxel of
 * every point, floor((p - min) / size) in fp32, or (-1, -1, -1) for a point outside the range on any axis. */
int sf_dynamic_voxelize_fwd(const float* points, int num_points, int num_features, const float* voxel_size, const float* coors_range,
                            int32_t* coors, void* stream);
size_t sf_hard_voxelize_ws_bytes(int num_points);
int sf_hard_voxelize_fwd(const float* points, int num_points, int num_features, const float* voxel_size,
                         const float* coors_range, int max_points, int max_voxels, float* voxels, int32_t* coors,
                         int32_t* num_points_per_voxel, float* mean_feats, int32_t* voxel_num, void* ws,
                         size_t ws_bytes, void* stream);

/* ---- N2 (second half): LiDAR SparseEncoder — sparse 3-D convolutions (mmdet3d/ops/spconv, spconv 1.x) ---------
 * Sites are rows of coords [n][4] = (batch, x, y, z) int32 in a grid `shape` = (X, Y, Z); ksize / stride /
 * padding are HOST arrays of 3 ints; kernel tap t = (kx*KY + ky)*KZ + kz.
 * sf_sparse_out_sites_fwd — output sites of a strided SparseConv3d (spconv/ops.py:19-33 output size; a
 *   site is active when some active input p and tap k satisfy p = o*stride - padding + k): sorted unique
 *   coordinates into out_coords (capacity `cap` rows), their number into the device int n_out.
 * sf_sparse_table_fwd — neighbour table nbr [n_out][ntaps]: input row read by output site j through tap t,
 *   or -1 (subm != 0: submanifold conv, out_coords == in_coords, offsets centred, stride/padding ignored).
 * sf_sparse_conv_fwd — the convolution (spconv/conv.py:114-214 + BatchNorm1d + ReLU of
 *   make_sparse_convmodule / SparseBasicBlock, sparse_block.py:88-107, :110-176):
 *   out[j] = act(scale * sum_t W_t^T . feats[nbr[j][t]] + bias) + add   (act_after_add: act(... + add));
 *   w packs [Cout][Cin][ntaps][1] (kh = ntaps, kw = 1); feats has n_in rows of feats_cs floats.
 * sf_sparse_to_dense_fwd — SparseConvTensor.dense() + permute/view of sparse_encoder.py:131-137 as NHWC:
 *   out [batch][X][Y][C*D], channel c*D + z (zero where no site is active).
 * Workspace of the two index entry points: sf_sparse_index_ws_bytes(n_in, ntaps) bytes (exactly that size is enough; 0 for n_in < 1 or
 *   ntaps < 1); SF_ERR_WORKSPACE when ws_bytes is smaller, whatever the call itself would have used.  SF_ERR_INVALID: a NULL pointer,
 *   n_in < 1, cap < 1, or a grid of batch * X * Y * Z >= 2^32 - 1 cells, input or output (keys are 32 bits, 0xFFFFFFFF is a sentinel).
 *   sf_sparse_out_sites_fwd writes the TRUE number of sites into n_out even where it exceeds cap; rows from cap on are not written. */
size_t sf_sparse_index_ws_bytes(int n_in, int ntaps);
int sf_sparse_out_sites_fwd(const int32_t* in_coords, int n_in, int batch, const int32_t* shape, const int32_t* ksize,
                            const int32_t* stride, const int32_t* padding, int32_t* out_coords, int cap, int32_t* n_out,
                            void* ws, size_t ws_bytes, void* stream);
int sf_sparse_table_fwd(const int32_t* in_coords, int n_in, const int32_t* out_coords, int n_out, int batch,
                        const int32_t* shape, const int32_t* ksize, const int32_t* stride, const int32_t* padding, int subm,
                        int32_t* nbr, void* ws, size_t ws_bytes, void* stream);
int sf_sparse_conv_fwd(const sf_conv_w* w, const float* feats, int feats_cs, int n_in, const int32_t* nbr, int n_out,
                       const float* add, int act_after_add, float* out, float* ws, size_t ws_bytes, void* stream);
/* sf_sparse_conv_masked_fwd — the same convolution with a TAP MASK (round 6): tile_mask64[i], i < ceil(n_out / 64), has bit t set when at
 *   least one of the output rows 64 i .. 64 i + 63 reads an input row through tap t (nbr[j][t] >= 0).  A pixel tile of the kernel then
 *   walks only the taps that are live for its rows; a skipped tap would have gathered zero rows, so the sums are bitwise those of
 *   sf_sparse_conv_fwd.  It pays when the caller keeps the output rows of a stage sorted by neighbour mask (rows with equal masks
 *   together: streamingflow_amd/models/sparse_encoder.py does; 38 % of the (site, tap) products of the shipped cloud have no input row and
 *   a tile of stored-order rows can drop < 1 % of them, a tile of mask-sorted rows 25 %).  NULL mask = sf_sparse_conv_fwd. */
int sf_sparse_conv_masked_fwd(const sf_conv_w* w, const float* feats, int feats_cs, int n_in, const int32_t* nbr, const uint32_t* tile_mask64,
                              int n_out, const float* add, int act_after_add, float* out, float* ws, size_t ws_bytes, void* stream);
int sf_sparse_to_dense_fwd(const float* feats, const int32_t* coords, int n, int C, int batch, int X, int Y, int D, float* out,
                           void* stream);
/* ---- static form of the index entry points: sizes fixed in advance, counts stay on the device ---------------------------------------
 * INACTIVE ROWS.  A site row coords[i] = (batch, x, y, z) is inactive when batch < 0; the entry points below write (-1, -1, -1, -1).
 *   Inactive rows may lie anywhere in a buffer (holes between per-cloud blocks, not only a tail); their feature rows may hold anything
 *   finite; no table entry of an active row ever points at one.  Every index kernel honours the convention, the entry points above
 *   included: an inactive input row has the sentinel key (never found, feeds no output site), an inactive output row reads -1 under
 *   every tap, and sf_sparse_to_dense_fwd skips inactive rows — it is its own static form.  The convolution needs nothing new: a -1
 *   entry gathers a zero row, so an inactive output row comes out as act(bias) (+ add), finite, and nothing reads it.
 * sf_voxel_rows_fwd — block k of a K-cloud row buffer from the padded outputs of sf_hard_voxelize_fwd for cloud k (coors
 *   [max_voxels][3], mean_feats [max_voxels][F], the device voxel_num): rows k*max_voxels + v of coords4 [K*max_voxels][4] and of
 *   feats [K*max_voxels][feats_cs] (feats_cs >= F, the rest zeros) = (k, x, y, z) and the mean for v < *voxel_num, inactive rows with
 *   zero features from there on; counts[k] = *voxel_num.  One launch, nothing read back.
 * sf_sparse_out_sites_static_fwd — sf_sparse_out_sites_fwd over cap_in input rows, some of them inactive: the sorted unique output
 *   sites into rows [0, min(count, cap_out)) of out_coords, inactive rows from there up to cap_out, the TRUE count into the device int
 *   n_out also where it exceeds cap_out (the caller compares when it chooses); nothing is written from cap_out on.
 * sf_sparse_table_static_fwd — sf_sparse_table_fwd over cap_in / cap_out rows with inactive rows on either side, plus the tap masks of
 *   sf_sparse_conv_masked_fwd: tile_mask64[i], i < ceil(cap_out / 64), = OR over the rows of the tile of their live taps (wave ballots).
 *   ONE-BIT RULE: a tile without any live tap (inactive rows only) gets bit 0 alone, never a zero word — the convolution reads zero as
 *   "walk every tap", one bit costs it one tap of zero rows instead of all of them, and the OR over an aligned 128-row pair of dead
 *   tiles is still one bit.  ntaps > 32: zero words (no mask).  The split-K launch ignores the mask and is correct without it.
 * Workspace: sf_sparse_index_ws_bytes(cap_in, ntaps), as above.  Enqueue-only (no allocation, no synchronisation, no atomics): the
 *   calls can be recorded into a graph.  SF_ERR_INVALID as above, or tile_mask64 NULL / cap_out < 1. */
int sf_voxel_rows_fwd(const int32_t* coors, const float* mean_feats, const int32_t* voxel_num, int max_voxels, int num_features, int k,
                      int feats_cs, int32_t* coords4, float* feats, int32_t* counts, void* stream);
int sf_sparse_out_sites_static_fwd(const int32_t* in_coords, int cap_in, int batch, const int32_t* shape, const int32_t* ksize,
                                   const int32_t* stride, const int32_t* padding, int32_t* out_coords, int cap_out, int32_t* n_out,
                                   void* ws, size_t ws_bytes, void* stream);
int sf_sparse_table_static_fwd(const int32_t* in_coords, int cap_in, const int32_t* out_coords, int cap_out, int batch,
                               const int32_t* shape, const int32_t* ksize, const int32_t* stride, const int32_t* padding, int subm,
                               int32_t* nbr, uint32_t* tile_mask64, void* ws, size_t ws_bytes, void* stream);

/* ---- N4: evaluation harness kernels (streamingflow/metrics.py, streamingflow/utils/instance.py) ------------
 * sf_confusion_fwd — out[b[i]*K + a[i]] += 1 over n int64 labels in [0, K) (zero-filled here); *bad != 0 when
 *   a label was outside the range.  IntersectionOverUnion.update (metrics.py:37: tp/fp/fn/support are sums of
 *   this matrix) and PanopticMetric.panoptic_metrics (:171-176: bincount of prediction + K * target).
 * sf_instance_centers_fwd — find_instance_centers (instance.py:80-92) on one [H][W] heat map: (row, col) of
 *   the thresholded 3x3 local maxima in row-major order (as torch.nonzero), count in the device int.
 * sf_group_pixels_fwd — group_pixels * foreground (instance.py:95-116, :136-137): offsets [2][H][W],
 *   foreground [H][W] bytes, instance [H][W] int64 = 1 + index of the nearest centre of (pixel + offset), 0 on background.
 * sf_instance_moments_fwd — F frames [F][H][W] of instance ids in one launch: per (frame, id in 1..max_id) pixel count,
 *   exact integer sums of (row, col) and — when flow [F][2][H][W] and warped_fx are given — sums of (row + flow0,
 *   col + flow1) in 2^-20 fixed point (int64).  Integer atomics only, so the sums do not depend on the arrival order:
 *   the masked means of instance.py:213-236 for every frame of a sequence at once.
 * sf_confusion_frames_fwd — sf_confusion_fwd per frame of F equally sized label-map pairs: out[F][K][K].
 * sf_instance_seq_fwd — get_instance_segmentation_and_centers (instance.py:119-144) for F frames at once: center [F][H][W],
 *   offsets [F][2][H][W], foreground [F][H][W] bytes.  Per frame: the centres as sf_instance_centers_fwd finds them (one flag
 *   pass and one exclusive scan over all F*H*W pixels; rank within a frame = scan value - the frame's first scan value) cut to
 *   the first `cap` -> centers [F][cap][2] (row, col), rows past min(n, cap) zero, and the UNCAPPED count -> n_centers [F];
 *   the grouping of sf_group_pixels_fwd over the frame's own min(n, cap) centres (a frame without centres is all zeros); ids
 *   made consecutive in the order of their values (lut[v] = number of present values < v, so a frame without a background
 *   pixel starts at 0, as the reference's does) -> instance [F][H][W] int64, every id <= cap.  Enqueues only: no allocation,
 *   no synchronisation, nothing read back.  SF_ERR_INVALID: a NULL pointer, F / H / W / cap < 1, F*H*W or F*(cap+1) >= 2^31,
 *   or F * ceil(H*W / 256) * 256 >= 2^32 (the grouping launch pads each frame to whole workgroups of 256 pixels);
 *   SF_ERR_WORKSPACE: ws_bytes < sf_instance_seq_ws_bytes(F, H, W, cap) (exactly that size is enough; 0 for invalid sizes).
 * sf_instance_track_fwd — the frame-to-frame matching of make_instance_id_temporally_consistent[_short_interval] (instance.py:171-368)
 *   for B samples of T frames on the moments sf_instance_moments_fwd wrote with max_id = K - 1: counts [B*T][K], pos_sums [B*T][K][2],
 *   warped_fx [B*T][K][2] (2^-20 fixed point) or NULL -> tables [B*T][K] int64, tables[frame][raw id] = the id that follows the instance
 *   through its sample; flags [B] int32, 0 = fine.  An instance of frame t+1 takes the id of the frame-t instance it is assigned to
 *   (minimum total distance between its centre and the frame-t anchors: the flow-displaced centres, or with warped_fx == NULL the plain
 *   centres, the short-interval matcher) when they are closer than matching_threshold, otherwise the next new id (new ids in ascending
 *   raw-id order, counted on from the largest id of frame 0); frame 0, absent ids and a frame next to an empty one keep their raw ids.
 *   Centres are fp64 quotients rounded to fp32, distances fp32 with every operation rounded on its own, duals and path costs fp64:
 *   the tables are those of the host statement (streamingflow_amd/instance.py: _consistent_tables, scipy) wherever every pair has ONE
 *   optimal assignment; where it has several, one of them, the same on every run.
 *   Launch 1, assign: one workgroup per (sample, pair of frames), cost matrix fp32 in LDS, shortest augmenting paths (Jonker-Volgenant
 *   in Crouse's rectangular form), every loop bounded by a row or column count.  Launch 2, chain: one wavefront per sample hands the
 *   ids down the frames.  A sample with a frame t+1 (t >= 0, frame t not empty) whose raw ids are not 1..n, or with a cost that is not
 *   finite, gets flags[b] = 1 (the host path's scipy call raises there); its tables hold ids that are otherwise unspecified.
 *   Workspace: match int32 [B*(T-1)][K] (partner raw id of frame t, or -1) | status int32 [B*(T-1)], each part on a multiple of 256
 *   bytes.  Enqueues only: no allocation, no synchronisation, nothing read back.  SF_ERR_INVALID: a NULL pointer (warped_fx aside),
 *   B / T / K < 1, K - 1 > 128, B*T*K >= 2^31; SF_ERR_WORKSPACE: ws_bytes < sf_instance_track_ws_bytes(B, T, K) (0 for invalid sizes).
 * sf_instance_labels_fwd — convert_instance_mask_to_center_and_offset_label (instance.py:12-77) for B sequences of T frames,
 *   all F = B*T frames at once: instance [F][H][W] int64 ids, theta [F][6] the row-major 2x3 sampling matrix each frame is
 *   resampled with (nearest neighbour, as sf_warp_affine_fwd does it; frame t of a sequence takes the inverse of ego-motion t-1,
 *   frame 0 is never looked at warped and may take the identity), K = num_instances: ids outside 1..K are background.
 *   Launch 1, moments: per (frame, id) the pixel count and the integer (row, col) sums of the frame as it is and of the frame as
 *   resampled — looked up destination pixel by destination pixel, with the coordinate arithmetic of sf_warp_affine_fwd bit for
 *   bit; no warped map is stored.  Integer atomics only.  A centre is round_half_even(fp32(sum) / fp32(count)) per axis: what
 *   x[mask].mean().round() gives while the sums stay below 2^24, i.e. on every grid up to 256 x 256 (beyond that fp32(sum) is a
 *   rounded value here and the order of torch's summation matters there).
 *   Launch 2, labels: center [F][1][H][W] = exp(-min_k d_k^2 / sigma^2) over the instances present in the frame (d^2 the exact
 *   integer squared distance to centre k, one fp32 division and one expf; 0 in a frame without instances), offset [F][2][H][W]
 *   = centre - pixel of the pixel's own instance, flow [F][2][H][W] = warped centre in frame t+1 - centre in frame t on the
 *   pixels of an instance that is present in t and t+1 and whose warped mask in t+1 is not empty; ignore_index elsewhere.
 *   Workspace, n = F*(K+1) slots, slot = frame*(K+1) + id, every part on a multiple of 256 bytes, zero-filled here:
 *     plain counts int32 [n] | plain sums int64 [n][2] | warped counts int32 [n] | warped sums int64 [n][2].
 *   Enqueues one memset and two launches, whatever B, T and K: no allocation, no synchronisation, nothing read back.
 *   SF_ERR_INVALID: a NULL pointer, B / T / H / W < 1, K < 0 or >= 2^24, H or W > 32768, sigma not > 0, F*H*W or F*(K+1) >= 2^31,
 *   or F * ceil(H*W / 256) * 256 >= 2^32; SF_ERR_WORKSPACE: ws_bytes < sf_instance_labels_ws_bytes(B, T, H, W, K) (0 for
 *   invalid sizes). */
/* sf_warp_affine_fwd — warp_features (utils/geometry.py:196-236): F.affine_grid(theta [B][2][3], align_corners=False)
 *   + F.grid_sample(mode nearest | bilinear, padding zeros, align_corners=False) on NCHW maps x [B][C][H][W]. */
int sf_warp_affine_fwd(const float* x, const float* theta, int B, int C, int H, int W, int bilinear, float* out,
                       void* stream);
/* sf_flow_warp_fwd — warp_with_flow (mmdet3d/models/beverse/models/motion_modules.py:434-449) on NHWC maps: state [P][C], P = B*H*W,
 *   resampled along a flow PER PIXEL (sf_warp_affine_fwd above resamples by one matrix per image), bilinear, zeros outside,
 *   align_corners=True.  The flow (x first, then y, in pixels) is either given, flow_in [P][2], or computed here as the 2-channel 1x1
 *   head of the motion module (offset_pred / flow_pred[1]): f = w_off [2][Cf] . feat [P][Cf] + b_off [2], feat the NHWC output of the
 *   offset ConvBlock; exactly one of feat / flow_in is non-NULL (w_off, b_off, Cf are read with feat only).  Destination pixel (b, i, j)
 *   samples image b at (i + fy, j + fx) (what the reference's normalise / un-normalise pair comes to, a few ulp apart): four taps at
 *   floor and floor + 1, a tap outside [0, W) x [0, H) contributes zero and is never read, so no other image of the batch is.
 *   The C channels of pixel p go to out[p*out_cs + out_co + c]: a channel slice of a wider tensor (the [P][C+L] input of the GRU cell).
 *   flow_out [P][2] (may be NULL) receives the flow used.  One launch, no workspace; enqueues only.
 *   SF_ERR_INVALID, nothing launched: a NULL state / out, both or neither of feat / flow_in, feat without w_off / b_off, B < 1, H < 2 or
 *   W < 2 (the reference divides by W - 1), C, Cf, out_cs or out_co not a positive multiple of 4 (out_co may be 0), out_co + C > out_cs,
 *   B*H*W >= 2^31, state / feat / w_off / out not 16-byte or flow_in / flow_out not 8-byte aligned, or the written slice of out
 *   overlapping state, feat or flow_in (neighbouring pixels are read while others are written: in place is a race). */
int sf_flow_warp_fwd(const float* state, const float* feat, const float* w_off, const float* b_off, const float* flow_in, float* out,
                     float* flow_out, int B, int H, int W, int C, int Cf, int out_cs, int out_co, void* stream);
int sf_confusion_fwd(const int64_t* a, const int64_t* b, long n, int K, int64_t* out, int32_t* bad, void* stream);
size_t sf_instance_centers_ws_bytes(int H, int W);
int sf_instance_centers_fwd(const float* center, int H, int W, float conf_threshold, int32_t* centers, int cap,
                            int32_t* n_centers, void* ws, size_t ws_bytes, void* stream);
int sf_group_pixels_fwd(const int32_t* centers, int n_centers, const float* offsets, const uint8_t* foreground, int H,
                        int W, int64_t* instance, void* stream);
int sf_instance_moments_fwd(const int64_t* instance, const float* flow, int F, int H, int W, int max_id, int64_t* pos_sums,
                            int64_t* warped_fx, int32_t* counts, void* stream);
int sf_confusion_frames_fwd(const int64_t* a, const int64_t* b, long n_per_frame, int F, int K, int64_t* out, int32_t* bad,
                            void* stream);
size_t sf_instance_seq_ws_bytes(int F, int H, int W, int cap);
int sf_instance_seq_fwd(const float* center, const float* offsets, const uint8_t* foreground, int F, int H, int W,
                        float conf_threshold, int cap, int32_t* centers, int32_t* n_centers, int64_t* instance, void* ws,
                        size_t ws_bytes, void* stream);
size_t sf_instance_track_ws_bytes(int B, int T, int K);
int sf_instance_track_fwd(const int32_t* counts, const int64_t* pos_sums, const int64_t* warped_fx, int B, int T, int K,
                          float matching_threshold, int64_t* tables, int32_t* flags, void* ws, size_t ws_bytes, void* stream);
size_t sf_instance_labels_ws_bytes(int B, int T, int H, int W, int num_instances);
int sf_instance_labels_fwd(const int64_t* instance, const float* theta, int B, int T, int H, int W, int num_instances, double sigma,
                           float ignore_index, float* center, float* offset, float* flow, void* ws, size_t ws_bytes, void* stream);
/* sf_panoptic_score_fwd — PanopticMetric.update's scoring (metrics.py:143-229) of B samples of T frames on the joint histograms
 *   sf_confusion_frames_fwd wrote: hist [B*T][K][K] int64 (rows = ground-truth id, columns = predicted id, id 0 = background),
 *   n_per_frame = the pixels of a frame, `bad` = that call's flag.  ADDS one update's tallies into iou, true_positive, false_positive
 *   and false_negative (fp32, n_classes entries each; class 0 = background, class 1 = the vehicles; the others are left alone).
 *   Per frame: areas = row / column sums, union = area_gt[g] + area_pred[p] - joint, IoU = union > 0 ? (float(joint) + 1e-9f) /
 *   (float(union) + 1e-9f) : 0 in fp32, every operation rounded on its own, a hit when IoU > 0.5f.  A hit at [0][0]: one class-0 true
 *   positive and its IoU.  A hit at [g >= 1][p >= 1]: with `track` != 0 and g's latest hit in an earlier frame of the same sample on
 *   another p, one false negative and one false positive; otherwise one true positive and its IoU.  A ground-truth / predicted thing
 *   with pixels and no hit in its row / column: one false negative / false positive.  IoU sums are exact fp64 sums rounded to fp32
 *   once; every counter receives ONE add per call, from one thread: the counters are bitwise those of the host statement
 *   (streamingflow_amd/metrics.py: _score_frame) and the same on every run.
 *   *errors (int32) is OR-ed with SF_PANOPTIC_ERR_RANGE when *bad != 0 and with SF_PANOPTIC_ERR_NO_BACKGROUND when no frame of the
 *   call has a ground-truth pixel of id 0 (metrics.py:107); a call that sets a bit adds NOTHING to the counters.
 *   Launch 1: one workgroup per frame (areas through LDS; per g the hit column and IoU, the frame's unmatched counts, into the
 *   workspace).  Launch 2: one workgroup, a lane per (sample, g) walks the frames with the partner in a register.  Workspace: hit
 *   column int32 [B*T][K] | hit IoU fp32 [B*T][K] | frame tallies int32 [B*T][4], each part on a multiple of 256 bytes.  Enqueues only:
 *   no allocation, no synchronisation, nothing read back.  SF_ERR_INVALID: a NULL pointer, B / T / K / n_per_frame < 1, n_classes < 2,
 *   K > SF_PANOPTIC_MAX_K, n_per_frame >= 2^23 (beyond it fp32 no longer holds the areas exactly and a row could hold two hits),
 *   B*T*K >= 2^31; SF_ERR_WORKSPACE: ws_bytes < sf_panoptic_score_ws_bytes(B, T, K) (0 for invalid sizes). */
#define SF_PANOPTIC_MAX_K 256
#define SF_PANOPTIC_ERR_RANGE 1
#define SF_PANOPTIC_ERR_NO_BACKGROUND 2
size_t sf_panoptic_score_ws_bytes(int B, int T, int K);
int sf_panoptic_score_fwd(const int64_t* hist, long n_per_frame, int B, int T, int K, int n_classes, int track, const int32_t* bad,
                          float* iou, float* true_positive, float* false_positive, float* false_negative, int32_t* errors, void* ws,
                          size_t ws_bytes, void* stream);

/* ---- the planner (streamingflow/cost.py, models/planning_model.py, metrics.py:263-396).  Every pointer below is a device pointer
 * except `factors`; every call enqueues only: no allocation, no synchronisation, nothing read back.  Grids are square (H == W = G).
 * Trajectories are rows of traj_stride floats per waypoint (x, y first), so a [.., T, 3] tensor is passed as it is.
 * sf_plan_cost_fwd — Cost_Function.forward for trajs [B][N][T] waypoints: cost_volume [B][T][G][G] fp32, occupancy [B][T][G][G] uint8,
 *   lane_divider and drivable [B][G][G] fp32 already reduced to one channel, target_points [B][2], the footprint tables rc0 [n0][2] and
 *   rc_lambda [n_lambda][2] (int32 row, column offsets of the ego rectangle and of the rectangle grown by lambda), dx [2], bx [2],
 *   safety_w [2] (device), factors[7] (HOST: safety, headway, lane divider, comfort, progress, rule, cost volume), the headway and the
 *   divider distance in metres -> cost_fo [B][N][T], cost_fc [B][N], cs [B][N] = cost_fc + sum_t cost_fo.  Two launches: a one-thread
 *   launch forms target_points.sum() < 0.5 (over the whole batch) in the workspace, the second scores one trajectory per wavefront.
 *   SF_ERR_INVALID: a NULL pointer, B / N / T / H < 1, H != W, traj_stride < 2; SF_ERR_WORKSPACE: ws_bytes < sf_plan_cost_ws_bytes().
 * sf_plan_select_refine_fwd — one workgroup per sample: arg-min of cs [B][N] over N (lowest index on a tie), selected [B][T][3] = that
 *   trajectory, and, for S > 0, the refinement loop of Planning.forward on it: h = h0 [B][S], x = 0, per waypoint
 *   h = GRUCell([x, waypoint xy, target]), x = Linear(ReLU(Linear(h))) -> refined [B][T][3] with a zero third column.  Weights in
 *   torch's layout: w_ih [3S][6], w_hh [3S][S], b_ih, b_hh [3S] (gates r, z, n), w1 [S][S], b1 [S], w2 [2][S], b2 [2].  S == 0 selects
 *   only (the GRU arguments and refined may be NULL).  SF_ERR_INVALID: a NULL pointer, B / N / T < 1, S < 0 or > 256, traj_stride < 3.
 * sf_plan_metric_fwd — PlanningMetric.update: ADDS into obj_col [T], obj_box_col [T], l2 [T] (fp32) and total (int64) for trajs and
 *   gt_trajs [B][T] waypoints and segmentation [B][T][G][G] uint8.  One launch, one writer per counter (no atomics).
 *   SF_ERR_INVALID: a NULL pointer, B / T / H < 1, H != W, traj_stride < 2. */
size_t sf_plan_cost_ws_bytes(void);
int sf_plan_cost_fwd(const float* trajs, long traj_stride, const float* cost_volume, const uint8_t* occupancy, const float* lane_divider,
                     const float* drivable, const float* target_points, const int32_t* rc0, int n0, const int32_t* rc_lambda, int n_lambda,
                     const float* dx, const float* bx, const float* safety_w, const float* factors, float headway_L, float divider_L, int B,
                     int N, int T, int H, int W, float* cost_fo, float* cost_fc, float* cs, void* ws, size_t ws_bytes, void* stream);
int sf_plan_select_refine_fwd(const float* cs, const float* trajs, long traj_stride, const float* target_points, const float* h0,
                              const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const float* w1, const float* b1,
                              const float* w2, const float* b2, int B, int N, int T, int S, float* selected, float* refined, void* stream);
int sf_plan_metric_fwd(const float* trajs, const float* gt_trajs, long traj_stride, const uint8_t* segmentation, const int32_t* rc0, int n0,
                       const float* dx, const float* bx, int B, int T, int H, int W, float* obj_col, float* obj_box_col, float* l2,
                       int64_t* total, void* stream);

/* ---- the planner's trajectory sampler (streamingflow/utils/sampler.py:8-146 as datas/NuscenesData.py:526-551 calls it).  Device
 * pointers throughout; both entry points enqueue only (no allocation, no synchronisation, nothing read back) and may be captured.
 * sf_fresnel_fwd — S[i], C[i] = the Fresnel integrals int_0^z sin / cos(pi t^2 / 2) dt of z[i], i < n, in fp64 (scipy.special.fresnel's
 *   convention): odd in z, within 1e-12 of scipy on [-4, 24] (measured: DESIGN §6b N6), the phase pi z^2 / 2 reduced exactly beyond,
 *   +-1/2 for |z| >= 1e100, NaN for NaN.  SF_ERR_INVALID: a NULL pointer, n < 0.
 * sf_plan_sample_fwd — per sample b < B, M rows of n_t points (x, y, heading) from speed v0 [B], curvature kappa [B], frame t0, n0
 *   [B][2] (fp64) and uniforms [B][5][M] (fp64 in [0, 1): acceleration 10 (u - 0.5) + 2, random speed 15 u, speed choice (u >= 0.2
 *   takes the random speed, else v0), alpha 74 u + 6, curve choice (u < 0.2: circle, else clothoid); the last two are indexed by curve,
 *   n_left + n_right entries used).  Before the sort the rows are, for kappa > 0, [curves 0 .. n_left), n_straight lines, curves
 *   [n_left, n_left + n_right) mirrored (-x, y, -heading)], otherwise [curves [n_left, n_left + n_right) mirrored, lines, curves
 *   0 .. n_left)]; line i uses entry i of the first three draws, curve j entry n_straight + j.  Every row is evaluated at the n_t stamps
 *   tt_kept (fp64; tt_kept[0] is the stamp whose point the clothoids are shifted by) and at t_key; the rows are ordered by x at t_key,
 *   ascending and STABLY (equal keys keep their order before the sort), and written as out [B][M][n_t][3] fp32; order [B][M]
 *   (may be NULL) receives each written row's position before the sort.  All arithmetic is fp64, cast at the store.  Non-finite inputs
 *   give unspecified rows, never a write outside out / order.
 *   SF_ERR_INVALID: a NULL pointer other than order, B / M / n_t < 1, B > 65535, a negative count, counts that do not sum to M;
 *   SF_ERR_UNSUPPORTED: M > 4096; SF_ERR_WORKSPACE: ws_bytes < sf_plan_sample_ws_bytes(B, M, n_t) (0 for invalid sizes). */
int sf_fresnel_fwd(const double* z, long n, double* S, double* C, void* stream);
size_t sf_plan_sample_ws_bytes(int B, int M, int n_t);
int sf_plan_sample_fwd(const double* v0, const double* kappa, const double* t0, const double* n0, const double* tt_kept, double t_key,
                       const double* uniforms, int n_straight, int n_left, int n_right, int B, int M, int n_t, float* out, int32_t* order,
                       void* ws, size_t ws_bytes, void* stream);

/* hipGraph capture of whatever the caller enqueues between begin and end on `stream` (must not be
 * the legacy default stream). */
int sf_graph_begin(void* stream);
int sf_graph_end(void* stream, void** graph_exec_out);
int sf_graph_launch(void* graph_exec, void* stream);
int sf_graph_destroy(void* graph_exec);

/* hipEvent timing helper for bench.py (events recorded on the stream the kernels run on) */
int sf_event_create(void** ev);
int sf_event_record(void* ev, void* stream);
int sf_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on `stop` */
int sf_event_destroy(void* ev);

/* Per-launch profiler for bench.py (off by default): when enabled every implicit-GEMM launch is
 * bracketed by hipEvents on its own stream.  sf_prof_collect fills SF_PROF_KEYS-entry arrays indexed by
 * kernel key = tile_config*8 + epilogue (calls, total ms, algorithmic flops, algorithmic bytes). */
#define SF_PROF_KEYS 168      /* part of SF_ABI_VERSION: sf_prof_collect fills this many entries of each of its four arrays (160 -> 168 was version 5 -> 6) */
int sf_prof_enable(int on);
int sf_prof_collect(int32_t* calls, double* ms, double* flops, double* bytes);

size_t sf_pack_conv_bytes(int cout, int cin, int kh, int kw, int flags);
int sf_pack_conv(const float* weight, const float* conv_bias, const float* scale, const float* bn_weight, const float* bn_bias,
                 const float* bn_mean, const float* bn_var, float bn_eps, int cout, int cin, int kh, int kw, int c0, int c1, int act,
                 int dil, int stride, int pad, int flags, void* blob, size_t blob_bytes, sf_conv_w* out, void* stream);

/* The BatchNorm fold of sf_pack_conv on its own (the same device code): scale[i] = w[i] / sqrt(var[i] + eps),
 * bias[i] = b[i] - mean[i] * scale[i] (+ conv_bias[i] * scale[i]), i < n.  For callers that stack or zero-pad the folded
 * vectors of several layers before packing them as one convolution (streamingflow/models/decoder.py heads,
 * streamingflow/layers/temporal.py blocks).  There is no second implementation of the fold on the host side. */
int sf_bn_fold(const float* conv_bias, const float* bn_weight, const float* bn_bias, const float* bn_mean, const float* bn_var,
               float bn_eps, int n, float* scale, float* bias, void* stream);

/* Diagnostic builds of the library only (hipcc -DSF_STAMP; the product build returns SF_ERR_UNSUPPORTED): `buf` is a
 * device buffer of 64 slots x 4096 workgroups x 8 uint64; every implicit-GEMM launch then takes the next slot (mod 64)
 * and wave 0 of each workgroup records s_memrealtime (100 MHz) at entry / prologue done / first chunk landed / K loop
 * done / split-K hand-off done / epilogue stores issued / stores drained.  NULL switches it off. */
int sf_debug_stamps(void* buf);
/* diagnostic: workgroups per CU the runtime grants the large LDS-DMA tiles with their dynamic LDS
 * (0: 128x128 fp32, 1: 128x128 bf16x3, 2: 64x128 fp32, 3: 64x128 bf16x3); -1 on error */
int sf_debug_occupancy(int which);
/* diagnostic, host only (no HIP call, nothing dereferenced beyond *w: w->w / w->w_wino need only be non-NULL): what the conv dispatch will
 * decide for a launch of `nprob` (1..4) identical problems of packed layer `w` under epilogue family `epi` (0 affine, 1 blend, 2 LayerNorm +
 * GELU, 4 sampling) on n_img images of Hin x Win (in_up = 1: nearest x2 upsampling on read) — the Winograd plan of dispatch.hip (wino_plan)
 * under the switches in force.  flags: 1 = SE input scale present, 2 = residual present, 4 = second output present (the reset gate's).
 * out[0 .. SF_WINO_PLAN_INTS):
 *   [0] 1: the layer runs on the Winograd kernel (0: it does not, everything else is 0)
 *   [1] form: 2 plain, 3 dilated, 4 images concatenated along x
 *   [2] launches (segments): 1, or 2 = main launch + remainder band; 0: nothing is launched for these nprob problems together — a group
 *       (nprob > 1) cannot share a launch and runs one problem at a time; a single problem (nprob = 1) is beyond what the kernel's block
 *       decode computes exactly, and the call that asks for it returns SF_ERR_LAUNCH
 *   [3 + 4 s ..] per segment s: tile rows per block (4: 32-tile blocks, 2: 16-tile blocks), first tile row, tile rows, workgroups
 *   [11] workgroups of the whole launch on 32-tile blocks (what SF_WINO_SMALL_WGS is compared with)
 *   [12] arithmetic: bit s set = segment s runs the tall-tile form F(4,3) along y x F(2,3) along x (0: F(2x2, 3x3)) */
#define SF_WINO_PLAN_INTS 13
int sf_debug_wino_plan(const sf_conv_w* w, int epi, int n_img, int Hin, int Win, int in_up, int nprob, int flags, int32_t* out, int n_out);
/* diagnostic, host only (as above: no HIP call, only w[0 .. nprob) is read): what the conv dispatch will decide for ONE launch group of the
 * nprob (1..4) packed layers w[0 .. nprob) under epilogue family `epi` (0 affine, 1 blend, 2 LayerNorm + GELU, 3 trust, 4 sampling), each on
 * n_img images of Hin x Win — the plan of the tiled kernels (tiled_plan in dispatch.hip; the rows are TILES of csrc/sf_launch.h) under the
 * switches in force.  flags say what every problem carries beyond its layer: 1 = neighbour table (sparse gather), 2 = reset gate applied
 * while staging, 4 = SE input scale, 8 = split-bf16 weights, 16 = the call has split-K scratch.
 * out[0 .. SF_TILED_PLAN_INTS):
 * Returns what a launch of the group would: SF_ERR_UNSUPPORTED for a LayerNorm / trust group over 65..128 channels that carries a gate, a
 * neighbour table or an input scale, SF_ERR_LAUNCH where SF_NARROW names no tile.
 *   [0] the kernel family that runs the group: 0 the tiled kernels, 1 Winograd (at least one layer of the group; the others are then planned
 *       again as a group of their own), 2 small-P (1, 2: everything else is 0)
 *   [1] the table row planned, [2] the row whose instantiation runs (differs for SE-scaled / sampling launches of the larger LDS-DMA tiles)
 *   [3] mt, [4] ks: the direct kernel's run-time tile height and K groups (as planned; read by that row only)
 *   [5] the profiler key (kernel key = [5] * 8 + epi)
 *   [6 + i] K slices of problem i across workgroups (0: not split) */
#define SF_TILED_PLAN_INTS 10
int sf_debug_tiled_plan(const sf_conv_w* w, int epi, int n_img, int Hin, int Win, int in_up, int nprob, int flags, int32_t* out, int n_out);

#ifdef __cplusplus
}
#endif
#endif /* SFNATIVE_H */
