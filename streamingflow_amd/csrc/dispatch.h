// Conv dispatch, "which kernel, how tiled" (dispatch.hip): what the modules and entry points of api.hip need from it.  Host only.
// The mutable state behind it (profiler, split-K scratch, persistent flow, stamp slots) is private to dispatch.hip; the entry points reach
// it through the scopes and functions below.
#pragma once
#include "sf_launch.h"
#include "../../include/sfnative.h"

#include <algorithm>
#include <functional>

#define SF_TRY(expr) do { int _st = (expr); if (_st != SF_OK) return _st; } while (0)
#define SF_HIP(expr) do { if ((expr) != hipSuccess) return SF_ERR_LAUNCH; } while (0)

namespace sf {

inline size_t al(size_t n) { return (n + 63) & ~size_t(63); }
// A caller's workspace handed out in 256-byte blocks.  Every entry point has ONE layout struct whose take(Arena&, dims...) is the one place
// its buffers are laid out: the forward runs an arena over the caller's memory through it and checks ok() before it enqueues anything, the
// sf_*_ws_bytes query runs a measuring arena (no memory: take never fails, hands out null, and bytes() is the high-water mark) through the
// same function (layout_bytes).  So exactly the queried size is enough, and the layout may depend on nothing the query is not given.
struct Arena {
  float* base;
  size_t cap, off = 0, peak = 0;
  bool measuring, failed = false;
  Arena(float* b, size_t bytes) : base(b), cap(bytes / sizeof(float)), measuring(false) {}
  Arena() : base(nullptr), cap(~size_t(0)), measuring(true) {}
  float* take(size_t n) {
    const size_t a = al(n);
    if (!measuring && (!base || failed || a > cap - off)) { failed = true; return nullptr; }
    off += a;
    peak = std::max(peak, off);
    return measuring ? nullptr : base + (off - a);
  }
  bool ok() const { return !failed; }
  size_t bytes() const { return peak * sizeof(float); }
  // buffers that are never live together (a cell's against the infer_state's behind it): every alternative is carved from the same
  // offset, and the arena goes on behind the larger
  template <class... Alt>
  void larger_of(Alt&&... alt) {
    const size_t start = off;
    size_t end = off;
    ((off = start, alt(), end = std::max(end, off)), ...);
    off = end;
  }
};
template <class Layout, class... Dims>
size_t layout_bytes(Dims... dims) {      // the size query
  Arena A;
  Layout l{};
  l.take(A, dims...);
  return A.bytes();
}
template <class Layout, class... Dims>
bool carve(Layout& l, float* ws, size_t ws_bytes, Dims... dims) {      // the call: false = SF_ERR_WORKSPACE, with nothing enqueued yet
  Arena A(ws, ws_bytes);
  l.take(A, dims...);
  return A.ok();
}

// Switches, read once per process from the environment: the ones a test, bench.py, the package or a tools/*bench.py tool reads or sets, and
// the printing aids (INTEGRATION.md has the table; tests/test_switches.py pins the set).  Measured thresholds nobody varies are constants
// next to the planner that uses them (dispatch.hip).  geti (atoi) and
// getl (atol) in dispatch.hip are the only readers of the conv dispatch; isset: a debugging aid that is on when its variable is set at all.
// Three switches are LIVE — re-read at every Winograd plan (dispatch.hip: wino_live), because tests/test_gpu_wino_split.py and
// tests/test_gpu_wino_tall.py flip them inside one process to compare both forms on the same tensors: SF_WINO_SPLIT_WGS (default 512),
// SF_WINO_CAT_WIDE (default 1) and SF_WINO_TALL (0: F(2x2) everywhere, 1: the tall form wherever the kernel has it, unset: the measured rule); see wino_plan.
// One reader remains in a kernel file: SF_DWCONV_PK (aux_kernels.hip).
int geti(const char* name, int dflt);
long getl(const char* name, long dflt);
inline bool isset(const char* name) { return geti(name, INT32_MIN) != INT32_MIN; }
struct Tune {
  // 1: one latent: the launches of a rollout run as phases of ONE persistent flow kernel per cell boundary (conv_sp.hip: sp_flow_kernel;
  // workgroups flow from one layer's tile to the next on per-tile dependency counters, every wait bounded: sf_flow_errors).  Bitwise equal
  // to the launch-per-layer path in the same form of the layers, <= 1e-3 against the oracle (tests/test_gpu_persistent.py).  Round 6,
  // both measured in one session (profiles/r06_z_bench.json): 174.2 us per steady-state step against 141.5 for the launch path, whose
  // 3x3 / 7x7 layers run in the Winograd form the flow kernel does not have.  Off by default
  int persist = geti("SF_PERSIST", 0);
  int b3_small_tiles = geti("SF_B3_SMALL_TILES", 0);   // experiment: bf16x3 layers with 128-multiple cout on 64 x 128 tiles (3 workgroups per CU) instead of 128 x 128 (2)
  int wide64 = geti("SF_WIDE64", 0);               // 1: 64-cout layers at >= 131072 pixels on 64 x 256 tiles (TILE_DMA64x256) instead of 64 x 128
  int wino = geti("SF_WINO", 1);                   // layers packed with Winograd weights run conv_wino.hip from wino_min_p pixels (0: direct form everywhere)
  int wino_min_p = geti("SF_WINO_MIN_P", 14000);   // measured (profiles/r04_zz_wino_min_p_sweep.txt, r04_zz_step_min_p_batched_latents.txt): 6 or more batched 50x50 latents
                                                   // and one 200x200 latent gain 6-11 % per ODE step, 5 latents / one 100x100 latent lose 4-7 %; 32 latents +1.6 % on the headline
  int wino_sp = geti("SF_WINO_SP", 1);             // one latent (small-P kernel, launch path): its 3x3 layers run in the Winograd form too (conv_sp.hip; 0: direct form — the round-5 step)
  int flow_timeout = geti("SF_FLOW_TIMEOUT", 1 << 22);   // polls before a dependency wait of the flow kernel gives up (~1 us each: seconds); bring-up runs use a small value
  int fenced = geti("SF_HANDOFF_FENCED", 0);       // 1: split-K hand-offs also run the agent-scope release / acquire fences of round 1 (known-good reference for the fence-free sc1 form; gfx950 only either way)
  int pipe = geti("SF_PIPE", 2);                   // one latent: branch 2 of the NEXT dual cell (gates2 -> cand2, functions of the state only) rides in the launches of infer_state, its conv_decoder_2 in the candidate launch (0: every cell on its own, 5 launches)
  int sp = geti("SF_SP", 1);                       // small pixel counts: the loader / consumer kernel of conv_sp.hip (0: the round-1 kernels)
  int direct = geti("SF_DIRECT", 1);               // 0 disables the direct-fragment kernel
  int split = geti("SF_SPLIT", 1);                 // cross-workgroup split-K on 64x64 tiles (small P)
  int glds = geti("SF_GLDS", 31);                  // LDS-DMA staging for large plain layers: bit 0 = 128-cout tiles, bit 1 = 64-cout tiles, bit 2 = LayerNorm-epilogue tiles, bit 3 = cross-workgroup split-K launches (0: register staging everywhere)
                                                   // bits 4 and 5 are LIVE (glds_live, dispatch.hip): the ASPP head's 1x1 branch inside its projection launch / a test's forced 128 x 128 tile
  int small_dma = geti("SF_SMALL_DMA", 1);         // >= 0: plain layers below LARGE_P run on the LDS-DMA kernel (32x32 tiles); bit 0: GRU candidates too (pre-gated state)
  int narrow = geti("SF_NARROW", 9);               // tile for layers with <= 32 output channels (dispatch.hip: narrow_tile — 9: TILE_DMA32x128, 32 cout x 128 px; 4 / 6 / 7 / 10: 64 x 64 / 64 x 128 / 64 x 128 on four waves / 64 x 256; -1: the 64-row tiles as planned)
  // ---- what wino_plan / wino_runs decide by (conv_wino.hip's wino_takes says what the kernel CAN address)
  int wino_ln7 = geti("SF_WINO_LN7", 1);           // the 7x7 + LayerNorm layer of the batched cells as nine 3x3 tap groups on the Winograd kernel (0: direct form) ...
  int wino_ln7_min_p = geti("SF_WINO_LN7_MIN_P", 65536);   // ... from this many pixels: one cout block and 9 x cin/16 chunks per workgroup, so the launch needs a full round of
                                                   // workgroups (2 x 256 blocks of 32 tiles = 65536 pixels) to pay — 8 latents of 50x50 are 175 workgroups of ~200 us each and
                                                   // LOSE to the direct form (batch-8 step 549 -> 563 us, profiles/r06_ln7_ab.txt)
  int wino_sample = geti("SF_WINO_SAMPLE", 1);     // the sampling layer of the batched infer_state on the Winograd kernel (0: direct form)
  // 16-tile blocks where 32-tile blocks would leave the launch below this many workgroups (two rounds of the chip's 512 slots; 0: never).  The
  // 16-tile form runs THREE workgroups per CU (80 registers, 46 KB of LDS), so a launch of nominally 313 / 626 32-tile workgroups (10 000 tiles / 32; as launched 328 / 656: 25 x 13
  // blocks rounded up to 8) becomes about twice as many of 768 slots.  Measured per threshold (profiles/r06_wino16_ab.txt, single-sample forward): BLEND launches 0.608 -> 0.514 ms, AFFINE 2.880 ->
  // 2.841, forward 7.44 -> 7.27 ms; at two samples per forward 13.18 -> 13.14; above ~1 400 workgroups the 32-tile form wins (every workgroup
  // loads the whole U of its 64 output channels whatever its tile count: 16 tiles double the load instructions per MFMA)
  long wino_small_wgs = getl("SF_WINO_SMALL_WGS", 1000);
  bool wino_list = isset("SF_WINO_LIST");          // debugging aid (tools/r05/wino_layers.py): every Winograd launch timed by itself on stderr — SYNCHRONISES the stream
  bool wino_why = isset("SF_WINO_WHY");            // debugging aid: which large 3x3 launches keep the direct form
  bool prof_dump = isset("SF_PROF_DUMP");          // debugging aid: one line per profiled launch on stderr, in launch order
};
const Tune& tune();
// pixels from which the 64x64 / 64x128 tiles are used.  Measured: a 4-sample rollout (10000 px) is 18 % faster on the small-P kernels, 8 samples (20000 px) on the large tiles
constexpr int LARGE_P = 8192;
// the small-P kernel (conv_sp.hip) is used below this many pixels (one 50x50 latent; measured: from two samples on the round-1 kernels are as fast or faster)
constexpr int SP_MAX_P = 4096;

// Fill a problem from a packed layer + geometry.  Output spatial size follows the conv formula.
ConvProblem problem(const sf_conv_w& w, const float* in0, const float* in1, float* out, int n_img, int Hin, int Win, int in_up = 0);
// Launch a group of independent layers (1..SF_MAX_GROUP problems, one epilogue family) on the kernel family that takes it
int run(const ConvProblem* ps, int n, int epi, hipStream_t st);
inline int run1(const ConvProblem& p, int epi, hipStream_t st) { return run(&p, 1, epi, st); }
// what run() will decide, for the modules that shape their launch groups by it
bool wino_runs(const ConvProblem& q, int epi);                        // this problem runs on the Winograd kernel of the large launches
bool sp_takes(const ConvProblem* ps, int n, int epi);                 // this group runs on the small-P kernel
int chansum_tile_px(const ConvProblem* group, int n, int epi);
bool pregate(long P, const sf_conv_w& cand);
// the ASPP head's 128 x 128 LDS-DMA launches (dispatch.hip)
int glds_live();                                                      // SF_GLDS now: bit 4 (16) the producer form, bit 5 (32) a test's forced tile
bool plans_dma128(const ConvProblem& p, int epi);                     // run() would put this layer, alone, on TILE_DMA128x128
int run_dma128(const ConvProblem& p, bool producer, hipStream_t st);  // one plain AFFINE layer on that tile; producer: its first fuse_cout input channels computed in the launch
// zero fill / device-to-device copy as kernels (graph nodes like everything around them)
hipError_t zero_fill(void* p, size_t bytes, hipStream_t st);
hipError_t copy_floats(const float* src, float* dst, size_t n, hipStream_t st);

// ---- profiled launches: `launch` runs as it is while the profiler is off; while it is on, it is bracketed by two pooled events and
// recorded as `cost()` = {key (_lib.py KERNEL_NAMES), flops, bytes}.  Returns the launch's status (a failed launch records nothing)
struct Cost { int key; double flops, bytes; };
bool prof_on();
hipError_t prof_timed(const Cost& c, const std::function<hipError_t()>& launch, hipStream_t st);
template <class Launch, class CostFn>
hipError_t timed(Launch&& launch, CostFn&& cost, hipStream_t st) { return prof_on() ? prof_timed(cost(), launch, st) : launch(); }
void prof_enable(bool on);
int prof_collect(int32_t* calls, double* ms, double* flops, double* bytes);      // sf_prof_collect
int debug_stamps(void* buf);                                                     // sf_debug_stamps
int debug_wino_plan(const sf_conv_w& w, int epi, int n_img, int Hin, int Win, int in_up, int nprob, int flags, int32_t* out, int n_out);   // sf_debug_wino_plan
int debug_tiled_plan(const sf_conv_w* w, int epi, int n_img, int Hin, int Win, int in_up, int nprob, int flags, int32_t* out, int n_out);   // sf_debug_tiled_plan

// Scratch for the cross-workgroup split-K path, carved from the caller's workspace by the top-level entry points for the duration of one
// call (the pointer to it is thread-local inside dispatch.hip, no global allocation).  Two steps: SplitBufs::take is part of the entry
// point's layout; SplitScope arms it (RAII) once the whole layout is known to fit — it enqueues the zero fill of the counters.  Buffers
// that were not carved (null: the entry points whose scratch is optional) leave the call without split-K.
struct SplitCtx { float* slab; size_t slab_floats; unsigned* counters; int ncounters; };
constexpr size_t SPLIT_SLAB_FLOATS = size_t(8) << 20;   // 32 MB: 2048 (tile, slice) pairs of 64x64 fp32
constexpr int SPLIT_COUNTERS = 4096;
struct SplitBufs {
  float* slab = nullptr;
  unsigned* counters = nullptr;
  void take(Arena& A) {
    slab = A.take(SPLIT_SLAB_FLOATS);
    counters = reinterpret_cast<unsigned*>(A.take(SPLIT_COUNTERS));
  }
};
struct SplitScope {
  SplitCtx ctx{};
  SplitCtx* prev;
  SplitScope(const SplitBufs& b, hipStream_t st);
  ~SplitScope();
};

// ---- persistent flow (one latent inside a rollout, SF_PERSIST=1 / sf_set_flow_mode): while a FlowScope is active, run() records its
// small-P launch groups as phases of ONE persistent launch instead of launching them (dispatch.hip: FlowBuilder)
struct FlowBuilder;
struct FlowBufs {                   // the carve: tables and counters, flow_ws_floats() floats (nothing while the flow mode is off)
  unsigned char* table = nullptr;
  unsigned* done = nullptr;
  void take(Arena& A);
};
struct FlowScope {
  FlowBuilder* fb = nullptr;
  int status = SF_OK;
  // the arming step, after the layout is known to fit: `allow` and the flow mode and an armed split-K scratch: zeroes the counters (check status)
  FlowScope(bool allow, const FlowBufs& b, hipStream_t st);
  ~FlowScope();
  const unsigned* err() const;      // error word of the flow's bounded waits (null: no flow)
};
size_t flow_ws_floats();            // what FlowBufs::take carves under the flow mode in force now (0: off)
int seg_flush();                    // anything that is not a small-P launch first sends the recorded phases on their way (stream order)
int flow_copy_out(const float* src, float* dst, size_t n, hipStream_t st);      // state copy-out: rides in the next phase, or a copy launch
// end of a rollout: NaN over both outputs if a bounded wait of its flow timed out (err != null), and remember err for flow_errors()
int flow_close(const unsigned* err, float* a, size_t na, float* b, size_t nb, hipStream_t st);
int set_flow_mode(int on);          // sf_set_flow_mode
int flow_errors(hipStream_t st);    // sf_flow_errors

}  // namespace sf
