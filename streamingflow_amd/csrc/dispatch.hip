// Conv dispatch: which kernel a launch group runs on and how it is tiled (dispatch.h).  gfx950 only.
// run() only enqueues kernels on the caller's stream: no allocation, no sync (graph-capture safe).  The one exception is the SF_WINO_LIST
// debugging aid (wino_list_launch), which synchronises the stream to time every Winograd launch by itself: never set it in production.
#include "dispatch.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

// Zero fill as a KERNEL (16-byte stores): inside a captured rollout these are kernel nodes of the graph like everything
// around them.  (With hipMemsetAsync nodes the replayed 46-step RK4 rollout differed from eager by ~3e-6 from the third
// replay on — tools/r02, profiles/README.md "graph memset nodes" — while eager never did.)
__global__ void zero_fill_kernel(float4* __restrict__ p, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x)
    p[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}
__global__ void copy_kernel(const float4* __restrict__ src, float4* __restrict__ dst, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}
// persistent flow: a dependency wait that timed out leaves err[0] != 0 and the rollout's results undefined — make that loud instead of
// silent: every output of the call becomes NaN.  A kernel, so a captured graph carries the check with it.
__global__ void flow_poison_kernel(const unsigned* __restrict__ err, float* __restrict__ a, size_t na, float* __restrict__ b, size_t nb) {
  if (__builtin_nontemporal_load(err) == 0) return;
  const float q = __builtin_nanf("");
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < na + nb; i += (size_t)gridDim.x * blockDim.x) {
    if (i < na) a[i] = q;
    else b[i - na] = q;
  }
}

}  // namespace

namespace sf {

// device-to-device copy as a kernel node, for the same reason (n floats, a multiple of 4; both pointers 16-byte aligned)
hipError_t copy_floats(const float* src, float* dst, size_t n, hipStream_t st) {
  const size_t n4 = n / 4;
  if (n4 == 0 || (n & 3) || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15))
    return hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st);
  size_t blocks = (n4 + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(copy_kernel, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<const float4*>(src), reinterpret_cast<float4*>(dst), n4);
  return hipGetLastError();
}
hipError_t zero_fill(void* p, size_t bytes, hipStream_t st) {     // p 16-byte aligned, bytes a multiple of 16 (arena blocks are)
  const size_t n4 = bytes / 16;
  if (n4 == 0) return hipSuccess;
  size_t blocks = (n4 + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(zero_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, st, static_cast<float4*>(p), n4);
  return hipGetLastError();
}

int geti(const char* k, int d) { const char* v = std::getenv(k); return v ? std::atoi(v) : d; }
long getl(const char* k, long d) { const char* v = std::getenv(k); return v ? std::atol(v) : d; }
// the two LIVE switches of the Winograd plan (dispatch.h), read once per plan
struct WinoLive { long split_wgs; bool cat_wide; int tall; };
static WinoLive wino_live() { return {getl("SF_WINO_SPLIT_WGS", 512), geti("SF_WINO_CAT_WIDE", 1) != 0, geti("SF_WINO_TALL", -1)}; }
const Tune& tune() { static const Tune t; return t; }

static TileId pick_tile(int P, int epi) {
  if (epi == EPI_LNG || epi == EPI_TRUST) return P >= LARGE_P ? TILE_LN64x128 : TILE_S16x64K4;
  return P >= LARGE_P ? TILE_L64x64 : TILE_S16x64K4;
}

// Fill a problem from a packed layer + geometry.  Output spatial size follows the conv formula.
ConvProblem problem(const sf_conv_w& w, const float* in0, const float* in1, float* out, int n_img, int Hin, int Win, int in_up) {
  ConvProblem p;
  std::memset(&p, 0, sizeof(p));
  p.in0 = in0; p.in1 = in1; p.w = w.w; p.w3 = w.w_bf16x3; p.w_wino = w.w_wino; p.scale = w.scale; p.bias = w.bias; p.out = out;
  p.c0 = w.c0; p.c1 = w.c1; p.in0_cs = w.c0; p.in1_cs = w.c1;
  p.n_img = n_img; p.Hin = Hin; p.Win = Win; p.in_up = in_up;
  const int Hl = Hin << in_up, Wl = Win << in_up;
  p.KH = w.kh; p.KW = w.kw; p.dil = w.dil; p.stride = w.stride; p.pad = w.pad;
  p.Hout = (Hl + 2 * w.pad - w.dil * (w.kh - 1) - 1) / w.stride + 1;
  p.Wout = (Wl + 2 * w.pad - w.dil * (w.kw - 1) - 1) / w.stride + 1;
  p.cin_pad = w.cin_pad; p.ktot = w.kh * w.kw * w.cin_pad;
  p.cout = w.cout; p.cout_pad = w.cout_pad; p.act = w.act;
  p.add_cs = w.cout; p.out_cs = w.cout; p.out_co = 0; p.out2_cs = w.cout;
  p.eps = 1e-6f;
  p.clamp_from = -1;
  return p;
}

// ---- optional per-launch profiler (bench.py only; off by default) ---------
struct ProfRec { int key; double flops, bytes; hipEvent_t a, b; };
struct Profiler {
  bool on = false;
  std::vector<ProfRec> recs;
  std::vector<hipEvent_t> pool;
  hipEvent_t get() {
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
  }
};
static Profiler g_prof;
bool prof_on() { return g_prof.on; }
void prof_enable(bool on) { g_prof.on = on; }
hipError_t prof_timed(const Cost& c, const std::function<hipError_t()>& launch, hipStream_t st) {
  ProfRec r{c.key, c.flops, c.bytes, g_prof.get(), g_prof.get()};
  hipError_t e = hipEventRecord(r.a, st);
  if (e == hipSuccess) e = launch();
  if (e == hipSuccess) e = hipEventRecord(r.b, st);
  if (e == hipSuccess) {
    g_prof.recs.push_back(r);
  } else {
    g_prof.pool.push_back(r.a);
    g_prof.pool.push_back(r.b);
  }
  return e;
}
// Aggregates (and clears) the recorded launches by kernel key = (key of the tile row / kernel family, _lib.py KEY_NAMES) * 8 + epi.  Arrays of length SF_PROF_KEYS (include/sfnative.h; part of the ABI version):
// calls, total ms, total algorithmic flops, total algorithmic bytes.  Synchronises.
int prof_collect(int32_t* calls, double* ms, double* flops, double* bytes) {
  for (int i = 0; i < SF_PROF_KEYS; ++i) { calls[i] = 0; ms[i] = 0; flops[i] = 0; bytes[i] = 0; }
  for (auto& r : g_prof.recs) {
    float t = 0.f;
    SF_HIP(hipEventSynchronize(r.b));
    SF_HIP(hipEventElapsedTime(&t, r.a, r.b));
    if (r.key >= 0 && r.key < SF_PROF_KEYS) { calls[r.key] += 1; ms[r.key] += t; flops[r.key] += r.flops; bytes[r.key] += r.bytes; }
    if (tune().prof_dump) std::fprintf(stderr, "[sf-prof] key=%d us=%.1f gflop=%.3f mbytes=%.2f\n", r.key, t * 1e3, r.flops * 1e-9, r.bytes * 1e-6);
    g_prof.pool.push_back(r.a);
    g_prof.pool.push_back(r.b);
  }
  g_prof.recs.clear();
  return SF_OK;
}

// diagnostic builds (-DSF_STAMP): conv launches take consecutive slots (mod 64) of the stamp buffer
static int g_stamp_slot = 0;
static bool g_stamp_on = false;
static int next_stamp_slot() {
  const int slot = g_stamp_slot;
  if (g_stamp_on) g_stamp_slot = (g_stamp_slot + 1) % 64;
  return slot;
}
int debug_stamps(void* buf) {
  if (set_stamp_buffer((unsigned long long*)buf) != hipSuccess || set_stamp_buffer_sp((unsigned long long*)buf) != hipSuccess ||
      set_stamp_buffer_wino((unsigned long long*)buf) != hipSuccess)
    return SF_ERR_UNSUPPORTED;
  g_stamp_on = buf != nullptr;
  g_stamp_slot = 0;
  return SF_OK;
}

// ---- tile and chunk counts of a problem, each defined once
static long pixels(const ConvProblem& q) { return (long)q.n_img * q.Hout * q.Wout; }
static int tiles(const ConvProblem& q, int bn) { return (int)((pixels(q) + bn - 1) / bn) * ((q.cout_pad + 63) / 64); }      // bn pixels x 64 output channels
static int chunks32(const ConvProblem& q) { return q.KH * q.KW * (q.cin_pad / 32); }      // K chunks, 32 deep
static int chunks64(const ConvProblem& q) { return (chunks32(q) + 1) / 2; }               // ... 64 deep (the small-P kernel's direct form)

// LDS-DMA kernel: a 32-deep K chunk must come from ONE source tensor (a single input, or two whose channel counts are
// multiples of the chunk depth); channels past cin are zero-filled by the range check either way
static bool one_source_per_chunk(const ConvProblem& q) { return q.c1 == 0 || ((q.c0 % 32 == 0) && (q.c1 % 32 == 0)); }
// ... and an SE input scale is applied to the pixel fragments from a small LDS table: single input, <= 256 channels,
// a (<= 256-pixel) tile touching at most 4 images
static bool scale_ok(const ConvProblem& q) { return !q.in_scale || (q.c1 == 0 && q.cin_pad <= 256 && (long)q.Hout * q.Wout >= 128); }
// ... and its loaders keep 32-bit byte offsets: over the images a tile of `tile_px` pixels can touch (sparse: over all feature rows), and
// over the packed weights.  (Each family passes the width it always has: 64 for the small-P kernel, 256 elsewhere.)
static bool offsets_fit32(const ConvProblem& q, double tile_px) {
  const double span = q.gather ? 4.0 * q.Win : (tile_px / ((double)q.Hout * q.Wout) + 2.0) * q.Hin * q.Win * 4.0;   // bytes per channel stride unit
  return span * q.in0_cs < 2147483648.0 && span * q.in1_cs < 2147483648.0 && 4.0 * q.cout_pad * q.ktot < 2147483648.0;
}
// the Winograd kernel can address this problem (conv_wino.hip: wino_takes) and its family is switched on at this size: the 7x7 tap-group
// layer (SF_WINO_LN7, SF_WINO_LN7_MIN_P) and the sampling layer (SF_WINO_SAMPLE)
static bool wino_wanted(const ConvProblem& q, int epi) {
  if (epi == EPI_LNG && (!tune().wino_ln7 || pixels(q) < tune().wino_ln7_min_p)) return false;
  if (epi == EPI_SAMPLE && !tune().wino_sample) return false;
  return wino_takes(q, epi);
}
// this problem runs on the Winograd kernel of the large launches (conv_wino.hip)
bool wino_runs(const ConvProblem& q, int epi) {
  return tune().wino && (double)pixels(q) >= tune().wino_min_p && wino_wanted(q, epi) && !q.w3;
}

// the split-K scratch of the running top-level call (SplitScope)
static thread_local SplitCtx* g_split = nullptr;
// the persistent flow that records this thread's small-P launches (FlowScope; null: they are launched)
static thread_local FlowBuilder* g_seg = nullptr;

// Small-P kernel (conv_sp.hip): every problem of the launch must be stageable by its loaders — no reset-gate multiply
// while staging (the gates launch pre-gates the state), no neighbour table, one source tensor per 32-deep sub-chunk,
// an SE input scale only on a single input of <= 256 channels (all problems or none), 32-bit DMA offsets
bool sp_takes(const ConvProblem* ps, int n, int epi) {
  if (!tune().sp) return false;
  int scaled = 0, unscalable = 0;
  for (int i = 0; i < n; ++i) {
    const ConvProblem& q = ps[i];
    if (pixels(q) >= SP_MAX_P || q.gather || q.gate || q.out_planar || !one_source_per_chunk(q)) return false;
    if ((epi == EPI_LNG || epi == EPI_TRUST) && q.cout_pad > 64) return false;
    if (q.in_scale || q.se_sum) {
      ++scaled;
      if (q.c1 != 0 || q.cin_pad > 256 || (long)q.Hout * q.Wout < 32) return false;   // a 64-pixel tile touches <= 4 images
      if (q.se_sum && (q.n_img != 1 || q.c0 > 128 || q.c0 < 64 || q.se_cr < 1 || q.se_cr > 16 || q.c0 != q.cin_pad || q.se_nt > 20 * (512 / q.c0))) return false;
    } else if (q.c1 != 0 || q.cin_pad > 256 || (long)q.Hout * q.Wout < 32) {
      ++unscalable;      // could not ride in an SE-scaled launch (whose kernel multiplies every problem's input by a scale row: ones for this one)
    }
    if (!offsets_fit32(q, 64.0)) return false;
  }
  // an SE-scaled launch may carry problems without a scale as long as each fits the scaled kernel's staging — their rows of the scale
  // table are ones
  if (scaled && (unscalable || (epi != EPI_AFFINE && epi != EPI_SAMPLE))) return false;
  return true;
}
// ... and which of its 3x3 layers take the Winograd F(2x2, 3x3) form there (conv_sp.hip, ConvProblem::sp_wino): one image with even
// sides (a 64-pixel tile is then 16 whole Winograd tiles and the tile counts of both forms agree), stride 1, pad 1, no dilation, inputs in
// whole 32-channel sub-chunks, cout in whole 64-row tiles, transformed weights packed; not inside a persistent flow (its tile-level
// dependencies are in linear pixels), not the LayerNorm layers (the 7x7 and its fused 1x1)
static bool sp_wino_ok(const ConvProblem& q, int epi) {
  if (!tune().wino || !tune().wino_sp || g_seg || !q.w_wino) return false;
  // 3x3, or the trusting gate's 7x7 as nine 3x3 sub-kernels (144 instead of 196 products per 2x2 outputs)
  const bool k3 = q.KH == 3 && q.KW == 3 && q.pad == 1, k7 = q.KH == 7 && q.KW == 7 && q.pad == 3 && epi == EPI_LNG;      // (the kernel carries the tap groups in its LayerNorm instantiation only)
  if (!(k3 || k7) || q.stride != 1 || q.dil != 1 || q.in_up || q.gather || q.gate || q.out_planar || q.pool2 || q.add_up) return false;
  if (q.fuse_w && epi != EPI_LNG) return false;
  if (q.n_img != 1 || (q.Hout & 1) || (q.Wout & 1) || q.Hin != q.Hout || q.Win != q.Wout || q.Wout < 4 || q.Hout < 4) return false;
  if ((q.c0 % 32) || (q.c1 % 32) || q.c0 + q.c1 != q.cin_pad || (q.cout_pad % 64)) return false;
  if (q.w3) return false;
  return 4.0 * (k7 ? 9 : 1) * 16 * q.cout_pad * q.cin_pad < 2147483648.0;
}
// K units of a problem in the Winograd form: (tap group, 32-channel sub-chunk) pairs
static int sp_wino_units(const ConvProblem& q) { return (q.KH == 7 ? 9 : 1) * (q.cin_pad / 32); }
// pixels per tile of the small-P kernel.  Measured on the conv launches of an Euler step at 50x50 (profiles/r02_*):
// 64-pixel tiles with the K range split across workgroups win where a launch has a lot of work (both gate / candidate
// pairs, the 128 -> 128 layers of p_model, the 7x7), 32-pixel tiles without a hand-off elsewhere
constexpr double SP_WIDE_WORK = 1000;      // 64-pixel tiles + split K from this many (64x64 tile) x (64-deep chunk) units per launch
static int sp_bn(const ConvProblem* ps, int n, int epi) {
  for (int i = 0; i < n; ++i)
    if (sp_wino_ok(ps[i], epi)) return 64;      // the Winograd form lives on the 64-pixel tiles
  double work = 0;
  for (int i = 0; i < n; ++i)
    work += (double)tiles(ps[i], 64) * chunks64(ps[i]);
  return work >= SP_WIDE_WORK ? 64 : 32;
}
// pixels per SE partial-sum row the producing conv's epilogue writes (the SE gate kernel sums ceil(P / this) rows)
// (the producer's whole launch group decides its tile)
int chansum_tile_px(const ConvProblem* group, int n, int epi) { return sp_takes(group, n, epi) ? sp_bn(group, n, epi) : 16; }

// ---- persistent flow (one latent inside a rollout, SF_PERSIST=1): run() records its small-P launch groups as phases of ONE
// persistent launch (conv_sp.hip: sp_flow_kernel) instead of launching them.  The phase / problem tables are built on the host,
// written into the caller's workspace by small writer kernels (table pieces travel as kernel arguments: stateless and
// graph-capturable) and the flow kernel is launched when the rollout ends or something that is not a small-P launch intervenes.
constexpr size_t FLOW_TABLE_BYTES = size_t(1) << 20;       // phases + problems of one flow
constexpr int FLOW_DONE_COUNTERS = 1 << 20;                // counter dwords of one flow (SP_FLOW_PHASE_DWORDS = 1536 per phase: every polled counter on its own line)
constexpr size_t FLOW_WS_FLOATS = FLOW_TABLE_BYTES / 4 + FLOW_DONE_COUNTERS + 64;      // what FlowBufs::take carves
struct FlowBuilder {
  std::vector<FlowPhase> phases;
  std::vector<ConvProblem> probs;
  hipStream_t st;
  unsigned char* table;          // device: [phases | problems]
  unsigned* done;                // device: tile counters (zeroed at the start of the rollout), done[-64 .. -1] = error words
  unsigned* err;
  int next_done = 0;
  int recorded = 0;              // phases recorded so far in this rollout (never reset: picks the split-K scratch half of the next phase)
  bool b3 = false;
  int grid = 0;
  int launches = 0;
  // a pending state copy-out (src = an output of the last recorded phase): rides in the next phase
  const float* copy_src = nullptr; float* copy_dst = nullptr; int copy_n4 = 0;
  FlowBuilder(unsigned char* t, unsigned* d, unsigned* e, hipStream_t s) : st(s), table(t), done(d), err(e) {}
  int problem_index(const ConvProblem& q) {      // identical problems (steady-state steps ping-pong between two sets) are stored once
    for (size_t i = probs.size(); i-- > 0 && probs.size() - i <= 64;)
      if (std::memcmp(&probs[i], &q, sizeof(q)) == 0) return (int)i;
    probs.push_back(q);
    return (int)probs.size() - 1;
  }
  int flush() {
    if (copy_n4 > 0 && !phases.empty()) {      // no later phase to ride in: a copy kernel behind the flow (kernel boundary = visibility)
      const int rc = launch();
      if (rc != SF_OK) return rc;
      if (copy_floats(copy_src, copy_dst, (size_t)copy_n4 * 4, st) != hipSuccess) return SF_ERR_LAUNCH;
      copy_n4 = 0;
      return SF_OK;
    }
    return launch();
  }
  int launch() {
    if (phases.empty()) return SF_OK;
    const size_t pb = phases.size() * sizeof(FlowPhase), qb = ((probs.size() * sizeof(ConvProblem)) + 15) & ~size_t(15);
    if (pb + qb > FLOW_TABLE_BYTES) return SF_ERR_WORKSPACE;
    // tables of the PREVIOUS flow launch of this call are dead once that launch has run: stream order
    std::vector<unsigned char> tmp(pb + qb, 0);
    std::memcpy(tmp.data(), phases.data(), pb);
    std::memcpy(tmp.data() + pb, probs.data(), probs.size() * sizeof(ConvProblem));
    if (launch_flow_write(tmp.data(), table, pb + qb, st) != hipSuccess) return SF_ERR_LAUNCH;
    SpFlow F;
    std::memset(&F, 0, sizeof(F));
    F.nphase = (int)phases.size();
    F.timeout_polls = tune().flow_timeout;      // ~1 us per poll round: seconds, then the wait gives up instead of hanging the GPU
    F.ph = reinterpret_cast<const FlowPhase*>(table);
    F.p = reinterpret_cast<const ConvProblem*>(table + pb);
    F.done = done;
    F.err = err;
    if (launch_sp_flow(F, grid, b3, st) != hipSuccess) return SF_ERR_LAUNCH;
    ++launches;
    phases.clear(); probs.clear();
    return SF_OK;
  }
  // record one launch group as a phase.  SF_ERR_UNSUPPORTED: the caller launches it the ordinary way (after flush()).
  int add(const ConvLaunch& L, int epi, bool scaled, int bn) {
    const bool all3 = launch_runs_bf16x3(L);
    const int cap = sp_flow_capacity(all3);
    if (L.wg_base[L.nprob] < 1 || L.wg_base[L.nprob] > cap || !sp_flow_has(epi, scaled, bn)) return SF_ERR_UNSUPPORTED;
    if (!phases.empty() && all3 != b3) SF_TRY(flush());
    if ((phases.size() + 1) * sizeof(FlowPhase) + (probs.size() + L.nprob) * sizeof(ConvProblem) + 64 > FLOW_TABLE_BYTES ||
        next_done + SP_FLOW_PHASE_DWORDS > FLOW_DONE_COUNTERS) {
      SF_TRY(flush());
      if (next_done + SP_FLOW_PHASE_DWORDS > FLOW_DONE_COUNTERS) {      // counters used up: start over (stream order: the flow that used them is done)
        if (zero_fill(done, (size_t)FLOW_DONE_COUNTERS * sizeof(unsigned), st) != hipSuccess) return SF_ERR_LAUNCH;
        next_done = 0;
      }
    }
    b3 = all3;
    grid = cap;
    FlowPhase ph;
    std::memset(&ph, 0, sizeof(ph));
    // the problems of a phase sit next to each other in the table
    const int first = (int)probs.size();
    bool contiguous = true;
    int idx[SF_MAX_GROUP];
    for (int i = 0; i < L.nprob; ++i) { idx[i] = problem_index(L.p[i]); contiguous = contiguous && idx[i] == idx[0] + i; }
    if (!contiguous) {      // some were found earlier, some not: store the group again, in order
      probs.resize(first);
      for (int i = 0; i < L.nprob; ++i) probs.push_back(L.p[i]);
      idx[0] = first;
    }
    ph.nprob = L.nprob; ph.prob0 = idx[0];
    ph.epi = epi; ph.scaled = scaled ? 1 : 0; ph.nt = bn / 16;
    ph.n_wg = L.wg_base[L.nprob];
    for (int i = 0; i <= SF_MAX_GROUP; ++i) ph.wg_base[i] = L.wg_base[i];
    // every problem of a phase covers the same pixels (one latent): its tiles are counted per pixel tile
    const int Ptot = L.p[0].n_img * L.p[0].Hout * L.p[0].Wout;
    int expect = 0, halo = 0, full = 0;
    for (int i = 0; i < L.nprob; ++i) {
      const ConvProblem& q = L.p[i];
      if (q.n_img * q.Hout * q.Wout != Ptot || q.n_img != 1 || q.stride != 1 || q.in_up || q.Hin != q.Hout || q.Win != q.Wout) return SF_ERR_UNSUPPORTED;
      expect += (q.cout_pad + 63) / 64;
      const int ry = (q.KH - 1) / 2 * q.dil, rx = (q.KW - 1) / 2 * q.dil;
      const int h = ry * q.Win + rx;
      halo = h > halo ? h : halo;
      full = full || q.se_sum != nullptr;      // the SE gate of the prologue is a reduction over the whole producer
    }
    ph.bn = bn; ph.n_ptiles = (Ptot + bn - 1) / bn;
    if (ph.n_ptiles > SP_FLOW_MAX_TILES) return SF_ERR_UNSUPPORTED;
    ph.tile_base = next_done; ph.tile_expect = expect;
    ph.tot_base = next_done + SP_FLOW_MAX_TILES * SP_FLOW_TILE_STRIDE;
    next_done += SP_FLOW_PHASE_DWORDS;
    if (copy_n4 > 0) { ph.copy_n4 = copy_n4; ph.copy_src = copy_src; ph.copy_dst = copy_dst; copy_n4 = 0; }
    // finished items (every (problem, cout tile, pixel tile) once) + the workgroups that copy
    ph.tot_expect = expect * ph.n_ptiles + (ph.copy_n4 > 0 ? (grid - ph.n_wg > 0 ? grid - ph.n_wg : grid) : 0);
    ph.halo_px = halo; ph.dep_full = full;
    const size_t n = phases.size();
    if (n >= 1) {
      const FlowPhase& a = phases[n - 1];
      ph.prev_bn = a.bn; ph.prev_ntiles = a.n_ptiles; ph.prev_tile_base = a.tile_base; ph.prev_tile_expect = a.tile_expect;
      ph.prev_tot_base = a.tot_base; ph.prev_tot_expect = a.tot_expect;
    }
    if (n >= 2) {
      const FlowPhase& a = phases[n - 2];
      ph.lag_tot_base = a.tot_base; ph.lag_tot_expect = a.tot_expect;
    }
    phases.push_back(ph);
    ++recorded;
    return SF_OK;
  }
  int add_copy(const float* src, float* dst, size_t nfloats) {
    if ((nfloats & 3) || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15) || nfloats / 4 > 0x7fffffff || phases.empty() || copy_n4 > 0) return SF_ERR_UNSUPPORTED;
    copy_src = src; copy_dst = dst; copy_n4 = (int)(nfloats / 4);
    return SF_OK;
  }
};
static int g_flow_mode = -1;      // -1: SF_PERSIST from the environment (default 0); 0 / 1: set by sf_set_flow_mode
static thread_local const unsigned* g_flow_err_last = nullptr;      // error word of this thread's most recent persistent rollout (sf_flow_errors)
static bool flow_mode_on() { return g_flow_mode < 0 ? tune().persist != 0 : g_flow_mode != 0; }
int seg_flush() { return g_seg ? g_seg->flush() : SF_OK; }
// the persistent flow's tables and counters (5 MB) only where the flow form is switched on at the time of the query: the size query and
// the call see the same setting (a workspace sized without them makes a flow-mode call fail with SF_ERR_WORKSPACE, not overrun)
size_t flow_ws_floats() { return flow_mode_on() ? FLOW_WS_FLOATS : 0; }
void FlowBufs::take(Arena& A) {
  if (!flow_mode_on()) return;
  table = reinterpret_cast<unsigned char*>(A.take(FLOW_TABLE_BYTES / 4));
  done = reinterpret_cast<unsigned*>(A.take(FLOW_DONE_COUNTERS + 64));
}
FlowScope::FlowScope(bool allow, const FlowBufs& b, hipStream_t st) {
  if (!(allow && flow_mode_on() && g_split != nullptr && b.table && b.done)) return;
  g_seg = fb = new FlowBuilder(b.table, b.done, b.done + FLOW_DONE_COUNTERS, st);
  if (zero_fill(b.done, (FLOW_DONE_COUNTERS + 64) * sizeof(unsigned), st) != hipSuccess) status = SF_ERR_LAUNCH;
}
FlowScope::~FlowScope() {
  if (fb) g_seg = nullptr;
  delete fb;
}
const unsigned* FlowScope::err() const { return fb ? fb->err : nullptr; }
int flow_copy_out(const float* src, float* dst, size_t n, hipStream_t st) {
  if (g_seg && g_seg->add_copy(src, dst, n) == SF_OK) return SF_OK;
  SF_TRY(seg_flush());
  SF_HIP(copy_floats(src, dst, n, st));
  return SF_OK;
}
int flow_close(const unsigned* err, float* a, size_t na, float* b, size_t nb, hipStream_t st) {
  if (err) {      // the flow kernel's bounded waits: a timeout must not pass as a result
    hipLaunchKernelGGL(flow_poison_kernel, dim3(256), dim3(256), 0, st, err, a, na, b, nb);
    SF_HIP(hipGetLastError());
  }
  g_flow_err_last = err;      // null: this thread's most recent rollout has no bounded waits: sf_flow_errors says so instead of reporting an older one
  return SF_OK;
}
int set_flow_mode(int on) {
  const int was = g_flow_mode < 0 ? tune().persist : g_flow_mode;
  g_flow_mode = on < 0 ? -1 : (on ? 1 : 0);
  return was;
}
int flow_errors(hipStream_t st) {
  if (!g_flow_err_last) return SF_ERR_INVALID;
  unsigned v = 0;
  if (hipMemcpyAsync(&v, g_flow_err_last, sizeof(v), hipMemcpyDeviceToHost, st) != hipSuccess) return SF_ERR_LAUNCH;
  if (hipStreamSynchronize(st) != hipSuccess) return SF_ERR_LAUNCH;
  return (int)(v > 0x3fffffffu ? 0x3fffffffu : v);
}

// direct form: 2 P cout K flops; algorithmic bytes: each input pixel and each weight once, output once
static Cost direct_cost(int key, const ConvProblem* ps, int n) {
  Cost c{key, 0, 0};
  for (int i = 0; i < n; ++i) {
    const ConvProblem& q = ps[i];
    const double Pi = (double)q.n_img * q.Hout * q.Wout;
    const double K = (double)q.KH * q.KW * (q.c0 + q.c1);
    c.flops += 2.0 * Pi * q.cout * K;
    c.bytes += 4.0 * ((double)q.n_img * q.Hin * q.Win * (q.c0 + q.c1) + (double)q.cout * K + Pi * q.cout);
  }
  return c;
}
// Winograd form, priced at its EXECUTED flops: 16 products per 2x2 outputs, (cin, cout) pair and tap group (nine for the 7x7); the
// plan's form names the launch (_lib.KERNEL_NAMES: wino128x32t / wino64x64t / wino64x32t2, also its form with concatenated images /
// wino64x32t2dil)
// (tall_frac: the part of the layer's tile rows that runs in the tall form, 12 products per 2x2-tile equivalent and tap group; the tall
// tap groups of the 7x7 leave out the two y-positions of 18 whose weights are zero: 9 x 12 x 16 / 18 = 96 executed products)
static double wino_products(const ConvProblem& q, double tall_frac) {
  return q.KH == 7 ? 144.0 - 48.0 * tall_frac : 16.0 - 4.0 * tall_frac;
}
static Cost wino_cost(const ConvProblem* ps, int n, int epi, WinoForm form, double tall_frac) {
  Cost c{(16 + (form == WINO_CAT ? 2 : (int)form)) * 8 + epi, 0, 0};
  for (int i = 0; i < n; ++i) {
    const ConvProblem& q = ps[i];
    const double grp = q.KH == 7 ? 9.0 : 1.0;
    c.flops += 2.0 * wino_products(q, tall_frac) * wino_tiles(q) * q.cout * (q.c0 + q.c1);
    c.bytes += 4.0 * ((double)q.n_img * q.Hin * q.Win * (q.c0 + q.c1) + 16.0 * grp * q.cout * (q.c0 + q.c1) + (double)q.n_img * q.Hout * q.Wout * q.cout);
  }
  return c;
}
// opt-in math mode: a launch runs the bf16x3 K loop only when every problem of it was packed with split-bf16 weights
static void select_bf16x3(ConvLaunch& L) {
  bool all3 = true;
  for (int i = 0; i < L.nprob; ++i) all3 = all3 && L.p[i].w3 != nullptr;
  for (int i = 0; i < L.nprob; ++i) L.p[i].use_w3 = all3 ? 1 : 0;
}

// ---- run(): validate the group, then the four kernel families in order — wide LayerNorm, Winograd, small-P, tiled / LDS-DMA.  Each planner
// either answers NOT_MINE or runs the group and returns its status.
constexpr int NOT_MINE = 1;      // (every SF_* status is <= 0)

// A LayerNorm / trust epilogue over 65..128 channels (hidden sizes above every shipped config): all channels of a pixel must sit in one
// wave: 128 cout x 64 px tiles of the LDS-DMA kernel, whatever the pixel count
static bool wide_ln_takes(const ConvLaunch& L) {
  for (int i = 0; i < L.nprob; ++i) {
    const ConvProblem& q = L.p[i];
    if (q.gate || q.gather || q.in_scale || q.se_sum || !one_source_per_chunk(q) || !offsets_fit32(q, 256.0)) return false;
  }
  return true;
}
static int run_wide_ln(ConvLaunch& L, int epi, hipStream_t st) {
  SF_TRY(seg_flush());
  if (!wide_ln_takes(L)) return SF_ERR_UNSUPPORTED;
  select_bf16x3(L);
  SF_HIP(timed([&] { return launch_conv_glds(L, epi, TILE_DMA_LN128x64, st); }, [&] { return direct_cost(TILES[TILE_DMA_LN128x64].key * 8 + epi, L.p, L.nprob); }, st));
  return SF_OK;
}

// ---- Winograd launches, deciding: wino_plan is a pure function of the problems and the switches — form, one or two launches (segments),
// per segment the window of tile rows, the block height, the grid and the reciprocals of the kernel's block decode, and whether the kernel's
// arithmetic covers all of it.  Nothing is launched before the whole plan stands.
struct WinoSeg {
  int th, row0, rows;      // blocks of th tile rows over the tile rows [row0, row0 + rows) of every image
  bool tall;               // the launch's arithmetic: F(4,3) x F(2,3) tall tiles (wino_tall) or F(2x2)
  long grid1;              // workgroups per problem (the launch has grid1 * nprob)
  unsigned m[5];           // ConvLaunch::wn_m
};
struct WinoPlan {
  bool ok = false;         // false: not one launch of this kernel (a group then runs one by one)
  WinoForm form = WINO_PLAIN;
  int nprob = 0, nseg = 0;
  long wgs32 = 0;          // workgroups of the whole layer / group on 32-tile blocks: what SF_WINO_SMALL_WGS is compared with
  WinoSeg seg[2];
};
// Concatenated images pay where blocks of 8 tile columns fit the image badly and no epilogue operand but an SE scale is per image (round 6: the SE scales of both images of a block)
static WinoForm wino_form(const ConvProblem& q, const WinoLive& live) {
  if (q.dil > 1) return WINO_DIL;
  const int tpi = (q.Wout + 1) / 2;
  if (q.in_up || q.n_img < 2 || tpi < WN_TW || q.bias_per_img) return WINO_PLAIN;
  const int plain = (tpi + WN_TW - 1) / WN_TW * WN_TW;
  // less than 10 % empty columns: the plain form, whose patch is two columns narrower — except at 128 or more output channels and at
  // least 4 % empty columns (100 tile columns run 104: the 200x200 gates and 128 -> 128 layers), where CAT measured 1.7 - 2.8 % faster and
  // the 64-channel layers within +-1 % (SF_WINO_CAT_WIDE=0: the 10 % rule alone)
  if (plain * 100 < tpi * 110 && (q.cout_pad < 128 || plain * 100 < tpi * 104 || !live.cat_wide)) return WINO_PLAIN;
  const double img_bytes = 4.0 * q.Hin * q.Win;
  const int cs = std::max(q.in0_cs, q.in1_cs), cm = std::max({q.out_cs, q.add_cs, q.e0_cs, q.e1_cs, q.out2_cs});
  return 2.0 * img_bytes * cs < 2147483648.0 && 2.0 * img_bytes * cm < 2147483648.0 ? WINO_CAT : WINO_PLAIN;      // two images behind one base
}
// tile blocks of one problem over `rows` tile rows of every image (tiles_x tile columns each) on blocks of th tile rows; nbx: block columns
static long wino_blocks(const ConvProblem& P, WinoForm form, int tiles_x, int rows, int th, long* nbx_out = nullptr) {
  const long nbx = ((form == WINO_CAT ? (long)P.n_img * tiles_x : tiles_x) + WN_TW - 1) / WN_TW, nby = (rows + th - 1) / th;
  if (nbx_out) *nbx_out = nbx;
  return form == WINO_CAT ? nby * nbx : (long)P.n_img * nby * nbx;
}
// ... and the workgroups of a launch of nprob such problems (the choice between the two block sizes and the split rule count the window a
// launch covers, not the layer)
static long wino_wgs(const ConvProblem& P, int nprob, WinoForm form, int tiles_x, int rows, int th) {
  return ((wino_blocks(P, form, tiles_x, rows, th) + 7) / 8) * 8 * (P.cout_pad / WN_COUT_T) * nprob;
}
// One launch.  false: the window is not one the kernel walks (it must end with the image or be whole blocks; the dilated form takes the
// whole image only), or the launch is beyond what the block decode computes exactly: it divides by multiplication with ceil(2^32 / d),
// exact while dividend x d < 2^32
static bool wino_segment(const ConvProblem& P, int nprob, WinoForm form, int th, int row0, int rows, WinoSeg& s) {
  int tiles_x, tiles_all;
  wino_tile_grid(P, tiles_x, tiles_all);
  if (row0 < 0 || rows < 1 || row0 + rows > tiles_all || (form == WINO_DIL && rows != tiles_all) || (row0 + rows < tiles_all && rows % th)) return false;
  long nbx;
  const long blocks = wino_blocks(P, form, tiles_x, rows, th, &nbx), nby = (rows + th - 1) / th, ncb = P.cout_pad / WN_COUT_T;
  const long grid1 = ((blocks + 7) / 8) * 8 * ncb, grid = grid1 * nprob;
  if (grid > 0x7fffffffL) return false;
  if ((grid1 / 8 + 1) * ncb >= 0x100000000L || (blocks + 8) * nbx >= 0x100000000L || (blocks + 8) * nby >= 0x100000000L ||
      (nbx * WN_TW + WN_TW) * tiles_x >= 0x100000000L)
    return false;
  if (nprob > 1 && grid * grid1 >= 0x100000000L) return false;
  s = WinoSeg{th, row0, rows, false, grid1, {nprob > 1 ? magic(grid1) : 1u, magic(ncb), magic(nbx), magic(nby), magic(tiles_x)}};
  return true;
}
// The arithmetic of a planned launch, decided apart from the plan (forms, blocks, grids and windows do not depend on it).  SF_WINO_TALL: 0 =
// F(2x2) everywhere, 1 = the tall form wherever the kernel has it (conv_wino.hip: wino_takes_tall — 32-tile blocks of the plain /
// concatenated AFFINE and BLEND forms and of the 7x7 LayerNorm layer's tap groups), unset = the measured rule, which is the same: profiles/wino_tall_layers_{off,on}.txt show no layer
// class of the batched forward slower in the tall form.  Remainder launches of split layers are 16-tile blocks: F(2x2)
static bool wino_tall(const ConvProblem& P, int epi, WinoForm form, const WinoSeg& s, const WinoLive& live) {
  return live.tall != 0 && wino_takes_tall(P, epi, form, s.th);
}
static double wino_tall_frac(const WinoPlan& W) {
  double rows = 0, tall = 0;
  for (int s = 0; s < W.nseg; ++s) { rows += W.seg[s].rows; tall += W.seg[s].tall ? W.seg[s].rows : 0; }
  return rows > 0 ? tall / rows : 0.0;
}
static WinoPlan wino_plan(const ConvProblem* ps, int n, int epi) {
  WinoPlan W;
  if (n < 1 || n > SF_MAX_GROUP) return W;
  const WinoLive live = wino_live();
  const ConvProblem& P = ps[0];
  W.form = wino_form(P, live);
  W.nprob = n;
  // a group: one geometry, one form, and — the rule of the groups — few enough tile blocks for the group decode by multiplication (< 2^32 /
  // workgroups; the exact tests of wino_segment cannot fail below this bound)
  for (int i = 1; i < n; ++i)
    if (!wino_same_geometry(P, ps[i]) || wino_form(ps[i], live) != W.form) return W;
  if (n > 1 && !(wino_tiles(P) * (P.cout_pad / 64.0) * n < 1.0e6)) return W;
  if (P.cout_pad % WN_COUT_T || (W.form == WINO_DIL && epi != EPI_AFFINE)) return W;
  int tiles_x, tiles_y;
  wino_tile_grid(P, tiles_x, tiles_y);
  W.wgs32 = wino_wgs(P, n, W.form, tiles_x, tiles_y, WN_TH);
  // the dilated form, the sampling layer, the tap groups and SE-scaled concatenated images have no 16-tile form and stay whole
  const bool only32 = W.form == WINO_DIL || epi == EPI_SAMPLE || epi == EPI_LNG || (W.form == WINO_CAT && P.in_scale);
  // 16-tile blocks where 32-tile blocks would leave the launch below SF_WINO_SMALL_WGS workgroups (Tune::wino_small_wgs)
  const bool small = !only32 && W.wgs32 < tune().wino_small_wgs;
  // Vertical remainder band: 25 / 50 tile rows end in a band of four with one / two real rows.  Such a layer runs as two launches: rows
  // [0, 4 floor(tiles_y / 4)) on 32-tile blocks, the rest on 16-tile blocks (28 -> 26 / 52 -> 50 tile rows executed) — where the remainder
  // launch has at least SF_WINO_SPLIT_WGS workgroups (default 512; 0: never, the layer stays whole).  Measured: the encoder / decoder
  // layers of 224 - 256 images (704 - 3 200 remainder workgroups) gain 3 - 6 %, the rollout's 32-image layers (208) nothing: every workgroup loads
  // the whole U and the launch has one more tail
  const int main_rows = tiles_y & ~(WN_TH - 1), rem_rows = tiles_y - main_rows;
  if (!small && !only32 && live.split_wgs > 0 && rem_rows > 0 && main_rows > 0 && wino_wgs(P, n, W.form, tiles_x, rem_rows, WN_TH_SMALL) >= live.split_wgs) {
    const bool main_small = wino_wgs(P, n, W.form, tiles_x, main_rows, WN_TH) < tune().wino_small_wgs;
    W.nseg = 2;
    W.ok = wino_segment(P, n, W.form, main_small ? WN_TH_SMALL : WN_TH, 0, main_rows, W.seg[0]) &&
           wino_segment(P, n, W.form, WN_TH_SMALL, main_rows, rem_rows, W.seg[1]);
  } else {
    W.nseg = 1;
    W.ok = wino_segment(P, n, W.form, small ? WN_TH_SMALL : WN_TH, 0, tiles_y, W.seg[0]);
  }
  for (int s = 0; W.ok && s < W.nseg; ++s) W.seg[s].tall = wino_tall(P, epi, W.form, W.seg[s], live);
  return W;
}
// the plan's launches, in order
static hipError_t wino_issue(ConvLaunch& L, const WinoPlan& W, int epi, hipStream_t st) {
  for (int s = 0; s < W.nseg; ++s) {
    const WinoSeg& g = W.seg[s];
    L.wg_base[0] = 0; L.wg_base[1] = (int)g.grid1;
    L.wn_ty0 = g.row0; L.wn_nty = g.rows;
    for (int k = 0; k < 5; ++k) L.wn_m[k] = g.m[k];
    const hipError_t e = launch_conv_wino(L, epi, W.form, g.th, g.tall, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
// sf_debug_wino_plan (include/sfnative.h): what run() will decide for nprob identical problems of this layer.  Host only: the pointers that
// decide are non-null placeholders, nothing is dereferenced, no HIP call
int debug_wino_plan(const sf_conv_w& w, int epi, int n_img, int Hin, int Win, int in_up, int nprob, int flags, int32_t* out, int n_out) {
  if (!out || n_out < SF_WINO_PLAN_INTS || nprob < 1 || nprob > SF_MAX_GROUP || n_img < 1 || Hin < 1 || Win < 1 || in_up < 0 || in_up > 1) return SF_ERR_INVALID;
  float* const ph = reinterpret_cast<float*>(uintptr_t(64));
  ConvProblem g[SF_MAX_GROUP];
  g[0] = problem(w, ph, w.c1 > 0 ? ph : nullptr, ph, n_img, Hin, Win, in_up);
  if (flags & 1) g[0].in_scale = ph;
  if (flags & 2) g[0].add = ph;
  if (flags & 4) { g[0].out2 = ph; g[0].out2_cs = w.cout / 2; g[0].e1 = ph; g[0].e1_cs = w.cout / 2; g[0].gate_from = w.cout / 2; }      // (the reset gate's second output)
  if (epi == EPI_SAMPLE) g[0].e0 = ph;
  for (int i = 1; i < nprob; ++i) g[i] = g[0];
  for (int i = 0; i < SF_WINO_PLAN_INTS; ++i) out[i] = 0;
  if (!wino_runs(g[0], epi)) return SF_OK;
  const WinoPlan W = wino_plan(g, nprob, epi);
  out[0] = 1; out[1] = (int)W.form; out[2] = W.ok ? W.nseg : 0;
  for (int s = 0; s < out[2]; ++s) {
    out[3 + 4 * s] = W.seg[s].th; out[4 + 4 * s] = W.seg[s].row0; out[5 + 4 * s] = W.seg[s].rows; out[6 + 4 * s] = (int)(W.seg[s].grid1 * nprob);
  }
  out[11] = (int)std::min(W.wgs32, 0x7fffffffL);
  for (int s = 0; s < out[2]; ++s) out[12] |= W.seg[s].tall ? 1 << s : 0;
  return SF_OK;
}

// SF_WINO_LIST (tools/r05/wino_layers.py): the launch timed by itself, one line on stderr.  SYNCHRONISES the stream — a debugging aid only
static int wino_list_launch(ConvLaunch& W1, const WinoPlan& W, int epi, hipStream_t st) {
  const ConvProblem& q = W1.p[0];
  hipEvent_t a, b;
  SF_HIP(hipEventCreate(&a)); SF_HIP(hipEventCreate(&b));
  SF_HIP(hipEventRecord(a, st));
  SF_HIP(wino_issue(W1, W, epi, st));
  SF_HIP(hipEventRecord(b, st));
  SF_HIP(hipEventSynchronize(b));
  float ms = 0.f;
  SF_HIP(hipEventElapsedTime(&ms, a, b));
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  std::fprintf(stderr, "[sf-wino] n=%d %dx%d c=%d+%d->%d epi=%d act=%d mode=%d add=%d add_scale=%d out2=%d in_scale=%d bias_img=%d clamp=%d dil=%d up=%d var=%d us=%.1f gflop=%.3f\n",
               q.n_img, q.Hout, q.Wout, q.c0, q.c1, q.cout, epi, q.act, q.mode, q.add != nullptr, q.add_scale != nullptr, q.out2 != nullptr,
               q.in_scale != nullptr, q.bias_per_img, q.clamp_from >= 0, q.dil, q.in_up, (int)W.form, ms * 1e3,
               2.0 * wino_products(q, wino_tall_frac(W)) * wino_tiles(q) * q.cout * (q.c0 + q.c1) * 1e-9);
  return SF_OK;
}
// SF_WINO_WHY: which large 3x3 launches keep the direct form, one line each on stderr
static void wino_why(const ConvProblem* ps, int n, int epi) {
  for (int i = 0; i < n; ++i)
    if (ps[i].KH == 3 && !wino_wanted(ps[i], epi))
      std::fprintf(stderr, "[sf] direct 3x3: n=%d/%d %dx%d c=%d+%d->%d stride=%d dil=%d up=%d gather=%d gate=%d in_scale=%d se_sum=%d nsplit=%d chansum=%d acc_in=%d fuse=%d mode=%d wino=%d\n",
                   i, n, ps[i].Hout, ps[i].Wout, ps[i].c0, ps[i].c1, ps[i].cout, ps[i].stride, ps[i].dil, ps[i].in_up, ps[i].gather != nullptr,
                   ps[i].gate != nullptr, ps[i].in_scale != nullptr, ps[i].se_sum != nullptr, ps[i].nsplit, ps[i].chansum != nullptr,
                   ps[i].acc_in != nullptr, ps[i].fuse_w != nullptr, ps[i].mode, ps[i].w_wino != nullptr);
}
// Winograd F(2x2, 3x3) for the 3x3 / stride-1 layers of large launches (conv_wino.hip): 2.25x fewer MACs, exact fp32 arithmetic; also the
// 7x7 + LayerNorm layer as nine 3x3 tap groups (EPI_LNG) and the sampling layer (EPI_SAMPLE).  The profiler prices a launch at its EXECUTED
// FLOPs (key 16).  The members of a group are independent layers: those the kernel takes run on it, the others stay one group (the ASPP
// group: three dilated 3x3 branches + the 1x1 branch)
static bool wino_considers(int P, int epi) {      // run_wino looks at the layers of a group at all
  return tune().wino && P >= tune().wino_min_p && (epi == EPI_AFFINE || epi == EPI_BLEND || epi == EPI_LNG || epi == EPI_SAMPLE);
}
static int run_wino(const ConvProblem* ps, int n, int P, int epi, hipStream_t st) {
  if (!wino_considers(P, epi)) return NOT_MINE;
  bool takes[SF_MAX_GROUP];
  int n_wino = 0;
  for (int i = 0; i < n; ++i) n_wino += (takes[i] = wino_runs(ps[i], epi)) ? 1 : 0;
  if (n_wino == 0) {
    if (tune().wino_why) wino_why(ps, n, epi);
    return NOT_MINE;
  }
  SF_TRY(seg_flush());
  if (n_wino < n) {
    ConvProblem rest[SF_MAX_GROUP];
    int nr = 0;
    for (int i = 0; i < n; ++i)
      if (!takes[i]) rest[nr++] = ps[i];
    SF_TRY(run(rest, nr, epi, st));
  }
  // one profiler record per planned layer / group, whatever its number of launches
  auto issue = [&](ConvLaunch& L, const WinoPlan& W) {
    L.stamp_slot = next_stamp_slot();
    return timed([&] { return wino_issue(L, W, epi, st); }, [&] { return wino_cost(L.p, L.nprob, epi, W.form, wino_tall_frac(W)); }, st);
  };
  // layers of identical geometry (the two branches of a dual cell) share ONE launch: their tails merge
  if (!tune().wino_list && n_wino >= 2) {
    ConvLaunch WG;
    std::memset(&WG, 0, sizeof(WG));
    for (int i = 0; i < n; ++i)
      if (takes[i]) WG.p[WG.nprob++] = ps[i];
    const WinoPlan W = wino_plan(WG.p, WG.nprob, epi);
    if (W.ok) {      // (not ok — geometries differ, or too large for the group decode: one launch per problem below)
      SF_HIP(issue(WG, W));
      return SF_OK;
    }
  }
  for (int i = 0; i < n; ++i) {      // the kernel takes one problem, or a group of one geometry: launched one by one
    if (!takes[i]) continue;
    ConvLaunch W1;
    std::memset(&W1, 0, sizeof(W1));
    W1.p[0] = ps[i];
    W1.nprob = 1;
    const WinoPlan W = wino_plan(W1.p, 1, epi);
    if (!W.ok) return SF_ERR_LAUNCH;
    if (tune().wino_list && !prof_on()) {
      W1.stamp_slot = next_stamp_slot();
      SF_TRY(wino_list_launch(W1, W, epi, st));
    } else {
      SF_HIP(issue(W1, W));
    }
  }
  return SF_OK;
}

// Small-P kernel, deciding: tile width (returned), which problems take the Winograd form, K slices with their slabs and tickets from
// `scratch` (null: no split), the compact grid and the reciprocals — all into L.  K ranges are split across workgroups (sc1 slab hand-off)
// so that the launch has about SP_SPLIT_WGS workgroups of equal length: a 2500-pixel layer has only 40 tiles of 64 pixels per 64 output
// channels
constexpr int SP_SPLIT_WGS = 240, WSP_MINSUB = 1;      // ... and a slice of a Winograd-form layer is at least this many 32-channel sub-chunks (measured: 1 -> 148.2 us per step, 2 -> 150.3)
static int sp_plan(ConvLaunch& L, int epi, const SplitCtx* scratch) {
  const int n = L.nprob, bn = sp_bn(L.p, n, epi);
  bool wn_of[SF_MAX_GROUP];
  int ns_of[SF_MAX_GROUP], tiles_of[SF_MAX_GROUP], nch_of[SF_MAX_GROUP];
  double work_total = 0;
  for (int i = 0; i < n; ++i) {
    wn_of[i] = bn == 64 && sp_wino_ok(L.p[i], epi);
    tiles_of[i] = tiles(L.p[i], bn);
    // (a 32-channel sub-chunk of the Winograd form costs a 64-pixel tile what a 64-deep chunk of the direct form does: 64 MFMAs per wave)
    nch_of[i] = wn_of[i] ? sp_wino_units(L.p[i]) : chunks64(L.p[i]);
    work_total += (double)tiles_of[i] * nch_of[i];
  }
  const int wg_target = SP_SPLIT_WGS, wg_cap = 256;
  const double per_wg = work_total / wg_target;      // chunks per workgroup at the target
  int wgs = 0;
  const bool may_split = scratch && tune().split && bn == 64;
  for (int i = 0; i < n; ++i) {
    int ns = (may_split && per_wg > 0) ? (int)(nch_of[i] / per_wg + 0.5) : 1;
    const int min_per = wn_of[i] ? WSP_MINSUB : 3;      // at least 3 chunks (direct) / WSP_MINSUB sub-chunks (Winograd) per slice
    if (ns > nch_of[i] / min_per) ns = nch_of[i] / min_per;
    if (ns > 8) ns = 8;
    if (ns < 1) ns = 1;
    ns_of[i] = ns;
    wgs += tiles_of[i] * ns;
  }
  // one workgroup owns a whole CU: a launch of more than 256 of them runs a second round for the few that are left
  // (measured: the 7x7 + projection launch at 280 workgroups took 54 us for 26 us of work per workgroup)
  // ... unless the ones that are left are SHORT and come last (round 6): problems whose workgroups do less than a third of the
  // longest one's chunks — the trusting gate's 1x1 projection beside its 7x7 — are not counted against the cap when they are the last
  // problems of the group: the dispatcher hands them to the few free CUs while the long ones run
  auto long_wgs = [&]() {
    double cmax = 0;
    for (int i = 0; i < n; ++i) cmax = std::max(cmax, (double)nch_of[i] / ns_of[i]);
    int cnt = wgs;
    for (int i = n - 1; i >= 1; --i) {      // trailing problems only
      if ((double)nch_of[i] / ns_of[i] * 3.0 > cmax) break;
      cnt -= tiles_of[i] * ns_of[i];
    }
    return cnt;
  };
  while (may_split && long_wgs() > wg_cap) {
    int k = -1;
    for (int i = 0; i < n; ++i)
      if (ns_of[i] > 1 && (k < 0 || tiles_of[i] * ns_of[i] > tiles_of[k] * ns_of[k])) k = i;
    if (k < 0) break;
    wgs -= tiles_of[k];
    --ns_of[k];
  }
  size_t slab_off = 0;
  int cnt_off = 0;
  for (int i = 0; i < n && may_split; ++i) {
    ConvProblem& q = L.p[i];
    int ns = ns_of[i];
    if (ns < 2) continue;
    const int cps = (nch_of[i] + ns - 1) / ns;
    ns = (nch_of[i] + cps - 1) / cps;      // every slice non-empty
    if (ns < 2) continue;
    const size_t per = (size_t)64 * bn;
    if (slab_off + (size_t)tiles_of[i] * ns * per > scratch->slab_floats || cnt_off + tiles_of[i] > scratch->ncounters) continue;
    q.nsplit = ns;
    q.slab = scratch->slab + slab_off;
    q.counters = scratch->counters + cnt_off;
    slab_off += (size_t)tiles_of[i] * ns * per;
    cnt_off += tiles_of[i];
  }
  // compact 1-D grid (no idle workgroups: step 198 -> 195 us): problem i owns logical workgroups [wg_base[i], wg_base[i + 1]), ids in dispatch order (xcd_shift 0:
  // XCD-contiguous ids measured 156 -> 144 MB of fabric traffic per step but 195 -> 203 us, tile-major 133 MB and 218 us — the round-robin spread over the XCDs is the fast one)
  int base = 0;
  for (int i = 0; i < n; ++i) {
    L.wg_base[i] = base;
    base += tiles_of[i] * (L.p[i].nsplit > 1 ? L.p[i].nsplit : 1);
  }
  for (int i = n; i <= SF_MAX_GROUP; ++i) L.wg_base[i] = base;
  for (int i = 0; i < n; ++i) {
    ConvProblem& q = L.p[i];
    const int ns = q.nsplit > 1 ? q.nsplit : 1;
    q.sp_wino = wn_of[i] ? 1 : 0;
    if (wn_of[i]) q.sp_cps = (nch_of[i] + ns - 1) / ns;      // K slices in 32-channel sub-chunks (also when no reciprocals are made below)
    // reciprocals of the divisors of the kernel's block decode and pixel decode (conv_sp.hip: sp_mdiv; exact while dividend x
    // divisor < 2^32: a launch has < 2^16 workgroups and < 2^13 pixels)
    const long Pi = pixels(q), n_pt = (Pi + bn - 1) / bn, kcpt = q.cin_pad >> 5;
    if ((long)tiles_of[i] * ns * tiles_of[i] >= 0x100000000L || (Pi + 64) * q.Hout * q.Wout >= 0x100000000L) continue;
    q.sp_m_tw = magic(q.Wout / 2);
    // d = 1 has no reciprocal (0 = "divide"): dividing by one is what the fallback does
    q.sp_m_tiles = magic(tiles_of[i]); q.sp_m_npt = magic(n_pt); q.sp_m_hw = magic((long)q.Hout * q.Wout); q.sp_m_w = magic(q.Wout);
    q.sp_m_kcpt = magic(kcpt); q.sp_m_kw = magic(q.KW);
    q.sp_cps = (nch_of[i] + ns - 1) / ns;
    q.sp_bn = bn;
  }
  return bn;
}
static int run_sp(ConvLaunch& L, int epi, hipStream_t st) {
  const int n = L.nprob;
  if (!sp_takes(L.p, n, epi)) return NOT_MINE;
  // inside a persistent flow consecutive phases overlap in time (a slice of phase q+1 may start while a last arriver of phase q
  // still reads its slabs): slabs and tickets alternate between the two halves of the scratch by phase parity (phase q+2 starts
  // only when phase q is complete)
  // (a running count of recorded phases, NOT the index inside the flow under construction: add() may flush first and the phase then
  // opens a new flow — with the index, the phase before the flush and the one after it could land on the same half)
  SplitCtx scratch = g_split ? *g_split : SplitCtx();
  if (g_split && g_seg) {
    const int parity = g_seg->recorded & 1;
    scratch.slab_floats /= 2; scratch.ncounters /= 2;
    scratch.slab += parity * scratch.slab_floats; scratch.counters += parity * scratch.ncounters;
  }
  const int bn = sp_plan(L, epi, g_split ? &scratch : nullptr);
  L.stamp_slot = next_stamp_slot();
  bool scaled = false;
  for (int i = 0; i < n; ++i) scaled = scaled || (L.p[i].in_scale != nullptr) || (L.p[i].se_sum != nullptr);
  select_bf16x3(L);
  if (g_seg && !prof_on()) {      // inside a rollout: a phase of the persistent flow (diagnostic stamps: slot = phase index mod 64)
    const int rc = g_seg->add(L, epi, scaled, bn);
    if (rc == SF_OK) return SF_OK;
    if (rc != SF_ERR_UNSUPPORTED) return rc;
    SF_TRY(g_seg->flush());                                               // does not fit the flow kernel: an ordinary launch
  } else {
    SF_TRY(seg_flush());
  }
  SF_HIP(timed([&] { return launch_conv_sp(L, epi, scaled, bn, st); }, [&] { return direct_cost(14 * 8 + epi, L.p, n); }, st));
  return SF_OK;
}

// Tiled / LDS-DMA kernels, deciding: the row of TILES (sf_launch.h) the launch runs on; mt / ks: the direct kernel's run-time tile
struct TiledPlan { TileId tile = TILE_S16x64K4; int mt = 0, ks = 1; };
// cross-workgroup split-K on 64x64 tiles: K slices, slabs and tickets into L, or L untouched where the scratch does not hold them
constexpr int SPLIT_WGS = 1024, SPLIT_MINCH = 2;      // aim for this many workgroups per launch (round 2, sc1 hand-off: 512 -> 1024, batch-8 step 754 -> 701 us), slices of at least this many chunks
static bool tiled_split(ConvLaunch& L, const SplitCtx& scratch) {
  // workgroup budget shared in proportion to each problem's work (tiles x chunks)
  double work_total = 0;
  for (int i = 0; i < L.nprob; ++i) work_total += (double)tiles(L.p[i], 64) * chunks32(L.p[i]);
  size_t slab_off = 0;
  int cnt_off = 0;
  bool fits = true;
  for (int i = 0; i < L.nprob; ++i) {
    ConvProblem& q = L.p[i];
    const int nt = tiles(q, 64), nc = chunks32(q);
    int ns = (int)(SPLIT_WGS * (double)nc / work_total + 0.5);
    if (ns > nc / SPLIT_MINCH) ns = nc / SPLIT_MINCH;
    if (ns > 16) ns = 16;
    if (ns < 1) ns = 1;
    const int cps = (nc + ns - 1) / ns;
    ns = (nc + cps - 1) / cps;      // every slice non-empty
    q.nsplit = ns;
    q.slab = scratch.slab + slab_off;
    q.counters = scratch.counters + cnt_off;
    slab_off += (size_t)nt * ns * 4096;
    cnt_off += nt;
    if (slab_off > scratch.slab_floats || cnt_off > scratch.ncounters) fits = false;
  }
  if (!fits) for (int i = 0; i < L.nprob; ++i) { L.p[i].nsplit = 0; L.p[i].slab = nullptr; L.p[i].counters = nullptr; }
  return fits;
}
// SF_NARROW: the tile of a 64-cout-family launch whose problems all have <= 32 output channels.  The values are the variant numbers the switch
// has always taken; one that names no tile fails the launch (TILE_NONE, tiled_plan)
static TileId narrow_tile(int v) {
  switch (v) {
    case 4: return TILE_DMA64x64;
    case 6: return TILE_DMA64x128;
    case 7: return TILE_DMA64x128W4;
    case 9: return TILE_DMA32x128;
    case 10: return TILE_DMA64x256;
  }
  return TILE_NONE;
}
// LDS-DMA staging (conv_glds_kernel) where the launch qualifies
static void tiled_glds(const ConvLaunch& L, int epi, TiledPlan& T) {
  const int n = L.nprob;
  const TileId staged = T.tile;
  const bool plain_epi = epi == EPI_AFFINE || epi == EPI_BLEND || epi == EPI_SAMPLE;
  bool plain = true;      // what every form needs: no reset gate while staging, a stageable SE scale, one source tensor per chunk
  int nscaled = 0;
  long pmin = 1L << 40;
  for (int i = 0; i < n; ++i) {
    const ConvProblem& q = L.p[i];
    plain = plain && !q.gate && scale_ok(q) && one_source_per_chunk(q);
    nscaled += q.in_scale != nullptr;
    pmin = std::min(pmin, pixels(q));
  }
  // Plain large layers (no reset gate / SE scale / neighbour table / split-K): LDS-DMA staging with the barrier in the
  // middle of the MFMA stream.  Measured (profiles/r01_v_*): 128x128 tiles +2 %, 64-cout layers
  // +7 % on 64x128 tiles once there are >= 1024 of them, +3 % on 64x64 tiles below that.
  if (tune().glds && (((staged == TILE_L64x64 || staged == TILE_L128x128) && plain_epi) || (staged == TILE_LN64x128 && (epi == EPI_LNG || epi == EPI_TRUST) && (tune().glds & 4)))) {
    bool ok = plain;
    for (int i = 0; i < n; ++i) ok = ok && L.p[i].nsplit <= 1 && offsets_fit32(L.p[i], 256.0);
    if (ok && staged == TILE_L128x128 && (tune().glds & 1)) T.tile = TILE_DMA128x128;
    if (ok && staged == TILE_L64x64 && (tune().glds & 2)) {
      T.tile = pmin >= 131072 ? (tune().wide64 ? TILE_DMA64x256 : TILE_DMA64x128) : TILE_DMA64x64;
      bool narrow = true;      // every problem has at most 32 output channels: half of a 64-row tile would multiply zeros
      for (int i = 0; i < n; ++i) narrow = narrow && L.p[i].cout_pad <= 32;
      if (narrow && tune().narrow >= 0) T.tile = narrow_tile(tune().narrow);
    }
    if (ok && staged == TILE_LN64x128 && nscaled == 0) T.tile = TILE_DMA_LN64x128;
  }
  if ((tune().glds & 8) && staged == TILE_SPLIT64x64) {   // cross-workgroup split-K launches (the slab hand-off is shared); SE-scaled layers on the SCALE instantiation
    bool ok = plain && ((nscaled == 0 && epi != EPI_SAMPLE) || (nscaled == n && (epi == EPI_AFFINE || epi == EPI_SAMPLE)));
    for (int i = 0; i < n; ++i) ok = ok && !L.p[i].gather && offsets_fit32(L.p[i], 256.0);
    if (ok) T.tile = TILE_DMA_SPLIT64x64;
  }
  // small pixel counts: the same kernel on 32x32 tiles beats the direct-fragment kernel by 5-15 % per plain layer
  // (profiles/r01_v_sweep_glds_wide_tiles.txt; single-sample rollout 5.10 -> 4.64 ms with the pre-gated candidates).
  // SF_SMALL_DMA=-1 switches it off, 0 keeps the reset gate in the candidate's staging.  LayerNorm epilogues on
  // 64x32 tiles were slower than the direct kernel and stay there.
  if (tune().small_dma >= 0 && (staged == TILE_S16x64K4 || staged == TILE_DIRECT16) && plain_epi) {
    bool ok = plain;
    for (int i = 0; i < n; ++i) ok = ok && !L.p[i].gather && L.p[i].nsplit <= 1;
    if (ok) T.tile = TILE_DMA32x32;
  }
}
constexpr int DIRECT_CPW = 5, SPLIT_FROM = 100;      // direct kernel: target K chunks per wave; small P: split-K only for layers with at least this many K chunks (the 7x7)
constexpr int MID_TILES = 1300;      // mid P: split-K below this many 64x64 tiles.  Round 2: 640 -> 1300 (the 200x200 latent splits its 7x7 too: 1364 -> 1311 us)
static int tiled_plan(ConvLaunch& L, int P, int epi, const SplitCtx* scratch, TiledPlan& T) {
  const int n = L.nprob;
  T.tile = pick_tile(P, epi);
  bool gathered = false;
  int chunks_max = 0, tiles_total = 0;
  for (int i = 0; i < n; ++i) {
    gathered = gathered || (L.p[i].gather != nullptr);
    chunks_max = std::max(chunks_max, chunks32(L.p[i]));
    tiles_total += tiles(L.p[i], 64);
  }
  if (gathered) {            // sparse convolution: only the LDS-staged kernels read the neighbour table
    if (epi != EPI_AFFINE) return SF_ERR_UNSUPPORTED;
    if (T.tile == TILE_S16x64K4) T.tile = TILE_L64x64;
  }
  if (T.tile == TILE_L64x64 && (epi == EPI_AFFINE || epi == EPI_BLEND)) {
    // measured (profiles/r01_e_sweep_large_tiles.txt): 128x128 tiles with 8 waves win 7-10 % once
    // there are >= ~1000 of them and cout is a multiple of 128; 64x64 wins everywhere else
    bool big = true;
    for (int i = 0; i < n; ++i) big = big && (L.p[i].cout_pad % 128 == 0) && (pixels(L.p[i]) >= 131072);
    if (big && !(tune().b3_small_tiles && L.p[0].w3 != nullptr)) T.tile = TILE_L128x128;
  }
  // small pixel counts: direct-fragment kernel (no LDS staging), see conv_igemm.hip
  if (T.tile == TILE_S16x64K4 && tune().direct && !gathered) {
    const bool ln = (epi == EPI_LNG || epi == EPI_TRUST);
    int cp_max = 0, cp_gcd = 0;
    bool ok = true;
    for (int i = 0; i < n; ++i) {
      const ConvProblem& q = L.p[i];
      ok = ok && (q.c0 % 8 == 0) && (q.c1 % 8 == 0);
      cp_max = q.cout_pad > cp_max ? q.cout_pad : cp_max;
      int a = q.cout_pad, b = cp_gcd;
      while (b) { int t = a % b; a = b; b = t; }
      cp_gcd = a;
    }
    if (ln) T.mt = (cp_max == 16 || cp_max == 32 || cp_max == 64) ? cp_max / 16 : 0;
    else T.mt = (cp_gcd % 32 == 0) ? 2 : 1   /* measured: 32-row tiles (twice the workgroups) beat 64-row ones */;
    T.ks = (chunks_max + DIRECT_CPW - 1) / DIRECT_CPW;
    T.ks = T.ks < 1 ? 1 : (T.ks > 8 ? 8 : T.ks);
    if (ok && T.mt) T.tile = TILE_DIRECT16;
  }
  // ... or, preferred: 64x64 tiles with the K range split across workgroups (4x fewer weight
  // re-reads than 16-pixel tiles, and enough workgroups for all 256 CUs)
  // measured (profiles/r01_d_sweep_convs.txt): the slab publish + ticket + acquire costs ~8 us, so
  // it only pays for the long-K layers (7x7: 196 chunks, 68 -> 44 us)
  const bool split_small = (T.tile == TILE_S16x64K4 || T.tile == TILE_DIRECT16) && chunks_max >= SPLIT_FROM;
  // a few batched samples (P = 8k..40k pixels): the large-tile kernels would have too few tiles,
  // each walking the whole K range; split the K range instead (also keeps LayerNorm layers on 64x64).  LayerNorm-epilogue layers take the
  // split from one K chunk (the 1x1 of the trusting gate: 4-sample step 415 -> 408 us; round 1 kept short K on 64x128 tiles), the others from 8
  const bool split_mid = (T.tile == TILE_L64x64 || T.tile == TILE_LN64x128) && tiles_total < MID_TILES && chunks_max >= (T.tile == TILE_LN64x128 ? 1 : 8);
  if ((split_small || split_mid) && tune().split && scratch && tiled_split(L, *scratch)) T.tile = TILE_SPLIT64x64;
  tiled_glds(L, epi, T);
  return T.tile == TILE_NONE ? SF_ERR_LAUNCH : SF_OK;      // (an SF_NARROW that names no tile: what the launcher's hipErrorInvalidValue became)
}
static int run_tiled(ConvLaunch& L, int P, int epi, hipStream_t st) {
  SF_TRY(seg_flush());
  TiledPlan T;
  SF_TRY(tiled_plan(L, P, epi, g_split, T));
  L.stamp_slot = next_stamp_slot();
  const TileStaging staging = TILES[T.tile].staging;
  if (staging == TILE_DMA) select_bf16x3(L);
  auto launch = [&]() -> hipError_t {
    if (staging == TILE_DMA) return launch_conv_glds(L, epi, T.tile, st);
    return staging == TILE_DIRECT ? launch_conv_direct(L, epi, T.mt, T.ks, st) : launch_conv(L, epi, T.tile, st);
  };
  SF_HIP(timed(launch, [&] { return direct_cost(TILES[T.tile].key * 8 + epi, L.p, L.nprob); }, st));
  return SF_OK;
}

// sf_debug_tiled_plan (include/sfnative.h): what run() will decide for a group of the layers w[0 .. nprob) on one geometry, by run()'s own
// family predicates (wide_ln_takes, wino_considers + wino_runs, sp_takes) in run()'s order.  Host only: the pointers that decide are non-null
// placeholders, nothing is dereferenced, no HIP call
int debug_tiled_plan(const sf_conv_w* w, int epi, int n_img, int Hin, int Win, int in_up, int nprob, int flags, int32_t* out, int n_out) {
  if (!out || n_out < SF_TILED_PLAN_INTS || nprob < 1 || nprob > SF_MAX_GROUP || epi < 0 || epi >= EPI_COUNT || n_img < 1 || Hin < 1 || Win < 1 || in_up < 0 || in_up > 1) return SF_ERR_INVALID;
  float* const ph = reinterpret_cast<float*>(uintptr_t(64));
  const bool ln_epi = epi == EPI_LNG || epi == EPI_TRUST;
  ConvLaunch L;
  std::memset(&L, 0, sizeof(L));
  L.nprob = nprob;
  int P = 0;
  bool wide_ln = false;
  for (int i = 0; i < nprob; ++i) {
    ConvProblem& q = L.p[i];
    q = problem(w[i], ph, w[i].c1 > 0 ? ph : nullptr, ph, n_img, Hin, Win, in_up);
    if (flags & 1) q.gather = reinterpret_cast<const int*>(ph);
    if (flags & 2) q.gate = ph;
    if (flags & 4) q.in_scale = ph;
    if (flags & 8) q.w3 = ph;
    P = std::max(P, (int)pixels(q));
    if (ln_epi && q.cout_pad > 128) return SF_ERR_UNSUPPORTED;
    wide_ln = wide_ln || (ln_epi && q.cout_pad > 64);
  }
  for (int i = 0; i < SF_TILED_PLAN_INTS; ++i) out[i] = 0;
  TiledPlan T;
  if (wide_ln) {
    if (!wide_ln_takes(L)) return SF_ERR_UNSUPPORTED;
    T.tile = TILE_DMA_LN128x64;
  } else {
    for (int i = 0; i < nprob; ++i)
      if (wino_considers(P, epi) && wino_runs(L.p[i], epi)) out[0] = 1;
    if (!out[0] && sp_takes(L.p, nprob, epi)) out[0] = 2;
    if (out[0]) return SF_OK;
    const SplitCtx scratch{ph, SPLIT_SLAB_FLOATS, reinterpret_cast<unsigned*>(ph), SPLIT_COUNTERS};
    SF_TRY(tiled_plan(L, P, epi, (flags & 16) ? &scratch : nullptr, T));
  }
  const bool scaled = epi == EPI_SAMPLE || (flags & 4);
  out[1] = T.tile; out[2] = TILES[T.tile].staging == TILE_DMA && scaled ? TILES[T.tile].scaled_as : T.tile;
  out[3] = T.mt; out[4] = T.ks; out[5] = TILES[T.tile].key;
  for (int i = 0; i < nprob; ++i) out[6 + i] = L.p[i].nsplit;
  return SF_OK;
}

int run(const ConvProblem* ps, int n, int epi, hipStream_t st) {
  ConvLaunch L;
  std::memset(&L, 0, sizeof(L));
  if (n < 1 || n > SF_MAX_GROUP) return SF_ERR_INVALID;
  const bool ln_epi = epi == EPI_LNG || epi == EPI_TRUST;
  int P = 0;
  bool wide_ln = false, has_acc = false;
  for (int i = 0; i < n; ++i) {
    L.p[i] = ps[i];
    L.p[i].fenced = tune().fenced;
    P = std::max(P, (int)pixels(ps[i]));
    if (ln_epi && ps[i].cout_pad > 128) return SF_ERR_UNSUPPORTED;
    wide_ln = wide_ln || (ln_epi && ps[i].cout_pad > 64);
  }
  L.nprob = n;
  if (P <= 0) return SF_OK;
  for (int i = 0; i < n; ++i) {
    const ConvProblem& q = ps[i];
    // the staged kernels keep per-tap element offsets (relative to the tile's first image) in 32 bits
    const double e0 = 2.0 * q.Hin * q.Win * q.in0_cs, e1 = 2.0 * q.Hin * q.Win * q.in1_cs;
    if (!q.gather && (e0 >= 2147483648.0 || e1 >= 2147483648.0)) return SF_ERR_UNSUPPORTED;
  }
  for (int i = 0; i < n; ++i)      // planar output: the AFFINE epilogue of the LDS-staged kernels only (never silently ignored)
    if (ps[i].out_planar && (epi != EPI_AFFINE || ps[i].pl_div < 1 || ps[i].out2 || ps[i].chansum)) return SF_ERR_UNSUPPORTED;
  for (int i = 0; i < n; ++i)      // pooled output / half-size residual: the Winograd kernel only (res_block checks first; never silently ignored)
    if ((ps[i].pool2 || ps[i].add_up) && !wino_runs(ps[i], epi)) return SF_ERR_UNSUPPORTED;
  // K-partial inputs and the blend mode of the AFFINE epilogue: small-P kernel only (never silently ignored)
  for (int i = 0; i < n; ++i) has_acc = has_acc || ps[i].acc_in != nullptr || (epi == EPI_AFFINE && (ps[i].mode & 4));
  if (has_acc && (wide_ln || !sp_takes(ps, n, epi))) return SF_ERR_UNSUPPORTED;
  if (wide_ln) return run_wide_ln(L, epi, st);
  int rc = run_wino(ps, n, P, epi, st);
  if (rc == NOT_MINE) rc = run_sp(L, epi, st);
  if (rc == NOT_MINE) rc = run_tiled(L, P, epi, st);
  return rc;
}

// ---- the ASPP head's 128 x 128 LDS-DMA launches (api.hip: deeplab_head).  SF_GLDS bits 4 and 5 are LIVE, re-read at every head
// (tests/test_gpu_aspp_producer.py flips them inside one process): bit 4: the 1x1 branch is computed inside the projection launch (the
// producer form of conv_glds_kernel) where the head qualifies; bit 5, a test's setting: the 1x1 branch and the projection of a head run on
// that tile whatever their pixel count, so that both forms can be compared on shapes of a few tiles
int glds_live() { return geti("SF_GLDS", 31); }
// run() would put this layer, alone, on TILE_DMA128x128
bool plans_dma128(const ConvProblem& p, int epi) {
  const int P = (int)pixels(p);
  if (P <= 0 || (wino_considers(P, epi) && wino_runs(p, epi)) || sp_takes(&p, 1, epi)) return false;
  ConvLaunch L;
  std::memset(&L, 0, sizeof(L));
  L.p[0] = p;
  L.nprob = 1;
  TiledPlan T;
  return tiled_plan(L, P, epi, g_split, T) == SF_OK && T.tile == TILE_DMA128x128;
}
// One plain AFFINE layer on TILE_DMA128x128, planner or not.  producer: the first fuse_cout input channels of p are
// relu(fuse_scale * (fuse_w . e0) + fuse_bias) and are not read from in0 (conv_igemm.hip: the producer form).  The record's cost counts both
// GEMMs and the bytes the launch moves: x, the input channels it does read, both weight matrices, the output
int run_dma128(const ConvProblem& p, bool producer, hipStream_t st) {
  ConvLaunch L;
  std::memset(&L, 0, sizeof(L));
  L.p[0] = p;
  L.p[0].fenced = tune().fenced;
  L.nprob = 1;
  const ConvProblem& q = L.p[0];
  if (pixels(q) <= 0) return SF_OK;
  if (q.gate || q.gather || q.in_scale || q.acc_in || q.pool2 || q.add_up || q.cout_pad % 128 || !one_source_per_chunk(q) || !offsets_fit32(q, 256.0)) return SF_ERR_UNSUPPORTED;
  if (producer) {
    ConvProblem x = q;      // the producer's own reads, by the same 32-bit rule
    x.in0_cs = q.e0_cs; x.in1_cs = 0; x.cout_pad = q.fuse_cout_pad; x.ktot = q.fuse_kpad;
    const bool ok = q.e0 && q.fuse_w && q.fuse_scale && q.fuse_bias && !q.w3 && q.cout_pad == 128 && q.c1 == 0 && q.KH == 1 && q.KW == 1 && q.stride == 1 &&
                    q.pad == 0 && !q.in_up && q.fuse_cout == 128 && q.fuse_cout_pad == 128 && q.fuse_kpad >= 32 && q.fuse_kpad % 32 == 0 &&
                    q.e0_cs == q.fuse_kpad && q.cin_pad > q.fuse_cout && q.cin_pad == q.c0 && q.Hin == q.Hout && q.Win == q.Wout && offsets_fit32(x, 256.0);
    if (!ok) return SF_ERR_UNSUPPORTED;
  }
  SF_TRY(seg_flush());
  L.stamp_slot = next_stamp_slot();
  select_bf16x3(L);
  auto cost = [&] {
    Cost c = direct_cost(TILES[TILE_DMA128x128].key * 8 + EPI_AFFINE, L.p, 1);
    if (producer) {
      const double Pi = (double)pixels(q);
      c.flops += 2.0 * Pi * q.fuse_cout * q.fuse_kpad;
      c.bytes += 4.0 * (Pi * q.fuse_kpad + (double)q.fuse_cout * q.fuse_kpad - Pi * q.fuse_cout);
    }
    return c;
  };
  SF_HIP(timed([&] { return producer ? launch_conv_glds_producer(L, st) : launch_conv_glds(L, EPI_AFFINE, TILE_DMA128x128, st); }, cost, st));
  return SF_OK;
}

// RAII: zero the counters of the carved split-K scratch and arm it for the duration of one top-level call
SplitScope::SplitScope(const SplitBufs& b, hipStream_t st) : prev(g_split) {
  if (!tune().split || !b.slab || !b.counters) return;
  ctx = {b.slab, SPLIT_SLAB_FLOATS, b.counters, SPLIT_COUNTERS};
  if (zero_fill(ctx.counters, SPLIT_COUNTERS * sizeof(unsigned), st) != hipSuccess) return;
  g_split = &ctx;
}
SplitScope::~SplitScope() { g_split = prev; }

// conv-GRU cells: large pixel counts: the gates epilogue also writes (1 - r) * s and the candidate convolution reads cat[x, rs] as a plain
// layer (LDS-DMA staging); otherwise the reset gate is applied while staging
bool pregate(long P, const sf_conv_w& cand) {
  const bool dma = P >= LARGE_P ? tune().glds != 0 : (tune().small_dma >= 0 && (tune().small_dma & 1));
  return dma && (cand.c0 % 32 == 0) && (cand.c1 % 32 == 0);
}
}  // namespace sf
