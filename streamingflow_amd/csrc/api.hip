// The model's modules + C ABI (include/sfnative.h) of libsfnative.so.  gfx950 only.  Which kernel a convolution runs on: dispatch.hip.
// Every function only enqueues kernels on the caller's stream: no allocation, no sync, no
// global mutable state (graph-capture safe).
#include "dispatch.h"

#include <cstring>
#include <vector>

using namespace sf;

namespace {

constexpr int ASPP_SLABS = 64;

bool valid_w(const sf_conv_w& w) {
  return w.w && w.cout > 0 && (w.cout % 4) == 0 && (w.cout_pad % 16) == 0 && w.cout_pad >= w.cout &&
         (w.cin_pad % 32) == 0 && w.cin_pad >= w.c0 + w.c1 && (w.c0 % 4) == 0 && (w.c1 % 4) == 0 && w.kh > 0 &&
         w.kw > 0 && w.stride > 0 && w.dil > 0;
}

// ---- modules ---------------------------------------------------------------------------------

// The two convolutions of one conv-GRU branch (temporal.py:44-57); gates buffer g: [P][2C] = [u | r].  rs: optional [P][C] scratch.  Large
// pixel counts: the gates epilogue also writes (1 - r) * s there and the candidate convolution reads cat[x, rs] as a plain layer (LDS-DMA
// staging); otherwise (rs == nullptr) the gate is applied while staging.
ConvProblem gates_problem(const sf_conv_w& gw, const float* in0, const float* in1, float* g, const float* s, float* rs, int C, int n, int H, int W) {
  ConvProblem p = problem(gw, in0, in1, g, n, H, W);
  if (rs) { p.out2 = rs; p.out2_cs = C; p.e1 = s; p.e1_cs = C; p.gate_from = C; }      // the pre-gated second output
  return p;
}
ConvProblem cand_problem(const sf_conv_w& cw, const float* x, const float* s, const float* rs, float* h, const float* g, int C, int n, int H, int W) {
  ConvProblem p = problem(cw, x, rs ? rs : s, h, n, H, W);
  p.e0 = g; p.e0_cs = 2 * C; p.e1 = s; p.e1_cs = C;                                      // the blend operands
  if (!rs) { p.gate = g; p.gate_cs = 2 * C; p.gate_co = C; }
  return p;
}

// conv-GRU cell: gates -> blend
int gru_cell(const sf_gru_w& w, const float* x, const float* s, float* out, float* g, float* rs, int n, int H, int W,
             hipStream_t st, int ode_derivative = 0) {
  const int C = w.cand.cout;
  if (!(rs && pregate((long)n * H * W, w.cand))) rs = nullptr;
  SF_TRY(run1(gates_problem(w.gates, x, s, g, s, rs, C, n, H, W), EPI_AFFINE, st));
  ConvProblem b = cand_problem(w.cand, x, s, rs, out, g, C, n, H, W);
  b.mode = ode_derivative ? 1 : 0;
  return run1(b, EPI_BLEND, st);
}

// ---- workspace layouts (dispatch.h: Arena).  One struct per module: take() is the carve of the forward AND, through a measuring arena,
// the module's sf_*_ws_bytes.  It sees what the size query is given (and the flow mode), never a weight or a launch plan: where a call can
// need less than that tells (a tile width, an absent projection), the bound is carved.  P: pixels of all images.
// gates [P][2C] and the pre-gated state [P][C] of one conv-GRU cell; SpatialGRU: + the two states it alternates between
struct GruBufs { float *g, *rs; void take(Arena& A, int C, size_t P) { g = A.take(P * 2 * C); rs = A.take(P * C); } };
struct SpatialGruBufs { float *g, *sa, *sb, *rs; void take(Arena& A, int C, size_t P) { g = A.take(P * 2 * C); sa = A.take(P * C); sb = A.take(P * C); rs = A.take(P * C); } };
template <class Bufs>
struct WithSplit {      // a module's buffers behind the split-K scratch of its convolutions
  SplitBufs split;
  Bufs bufs;
  template <class... Dims> void take(Arena& A, Dims... dims) { split.take(A); bufs.take(A, dims...); }
};
// scratch of one dual cell (temporal_ode_bayes.py:92-131 / :239-275)
struct CellBufs {
  float *g1, *g2, *h1, *h2, *r2, *t1, *sk, *t2, *rs1, *rs2;
  void take(Arena& A, int C, size_t P) {
    g1 = A.take(P * 2 * C); g2 = A.take(P * 2 * C); h1 = A.take(P * C); h2 = A.take(P * C); r2 = A.take(P * C);
    t1 = A.take(P * C); sk = A.take(P * C); t2 = A.take(P * C); rs1 = A.take(P * C); rs2 = A.take(P * C);
  }
};
// Small-P kernel: a 1x1 + LayerNorm + GELU layer `q` (weights w1) that follows the LayerNorm layer ps[0] is applied to ps[0]'s
// tile before it leaves the workgroup (conv_sp.hip, ConvProblem::fuse_*); ps[0]'s own output is then not stored.  Returns
// whether the launch of ps carries q.
bool fuse_following_1x1(ConvProblem* ps, int n, const ConvProblem& q, const sf_conv_w& w1, float* out) {
  if (!sp_takes(ps, n, EPI_LNG) || !sp_takes(&q, 1, EPI_LNG)) return false;
  if (w1.kh != 1 || w1.kw != 1 || w1.c1 != 0 || w1.cin_pad > 64 || w1.cout_pad > 64 || ps[0].cout_pad > 64 || !w1.scale || !w1.bias ||
      w1.c0 != ps[0].cout || q.add)
    return false;
  ps[0].out = nullptr;
  ps[0].fuse_w = w1.w; ps[0].fuse_scale = w1.scale; ps[0].fuse_bias = w1.bias; ps[0].fuse_out = out;
  ps[0].fuse_cout = w1.cout; ps[0].fuse_cout_pad = w1.cout_pad; ps[0].fuse_kpad = w1.cin_pad;
  return true;
}

// trusting gate + mix + integrator update   (:124-131, convolutions.py:348-380)
int cell_tail(const sf_dual_w& w, const float* s, float* out, int derivative, const float* base, const float* coef,
              int coef_stride, float* out2, int acc2, const CellBufs& b, int B, int H, int W, hipStream_t st) {
  ConvProblem ps[2];
  ps[0] = problem(w.tg7, b.h1, b.r2, b.t1, B, H, W); ps[0].mode = 1;     // 7x7 + LN + GELU
  ps[1] = problem(w.tgproj, b.h1, b.r2, b.sk, B, H, W); ps[1].mode = 0;   // 1x1 projection + GELU
  ConvProblem q = problem(w.tg1, b.t1, nullptr, b.t2, B, H, W); q.mode = 1;
  // one latent on the small-P kernel: the 1x1 + LN + GELU layer is applied to the 7x7 layer's tile before it leaves the
  // workgroup (one launch and one 0.64-MB round trip fewer per cell evaluation)
  const bool fuse_1x1 = fuse_following_1x1(ps, 2, q, w.tg1, b.t2);
  // batched latents: the 7x7 runs on the Winograd kernel (nine 3x3 tap groups, conv_wino.hip GRP = 9) by itself — the 1x1 projection, which only
  // reads h1 / r2, then shares the launch of the 1x1 + LN layer behind it instead of the 7x7's
  const bool wino7 = !fuse_1x1 && wino_runs(ps[0], EPI_LNG);
  if (wino7) {
    SF_TRY(run1(ps[0], EPI_LNG, st));
    ConvProblem g2[2] = {q, ps[1]};
    SF_TRY(run(g2, 2, EPI_LNG, st));
  } else {
    SF_TRY(run(ps, 2, EPI_LNG, st));
    if (!fuse_1x1) SF_TRY(run1(q, EPI_LNG, st));
  }
  ConvProblem f = problem(w.tg3, b.t2, nullptr, out, B, H, W);
  f.e0 = b.sk; f.e1 = w.w_logit; f.e2 = b.r2; f.e3 = b.h1; f.e4 = s; f.e5 = base ? base : s;
  f.coef = coef; f.coef_stride = coef_stride; f.out2 = out2; f.mode = (derivative ? 1 : 0) | (acc2 ? 2 : 0);
  if (derivative && !coef) return SF_ERR_INVALID;
  return run1(f, EPI_TRUST, st);
}

// Branch 2 of a dual cell — gru_cell_2(s, s) and conv_decoder_2 (temporal_ode_bayes.py:112-119 / :256-263) — is a function of
// the state alone.  In a rollout the state of cell j+1 is the output of cell j, so while infer_state(state) runs (five
// launches that only the NEXT cell's branch 1 waits for) branch 2 of the next cell is computed beside it: its gate and
// candidate convolutions ride in infer_state's first two launches (`Side`), its decoder convolution in the next cell's
// candidate launch.  One latent on the small-P kernel only (every launch there leaves CUs idle); same arithmetic, same
// summation orders as the cell on its own.
struct Carry {
  float *g2, *rs2, *h2;      // gates2 output [P][2C], (1 - r2) * s [P][C], blended hidden state of cell 2 [P][C]
  float* g1s;                // state half of gates1, raw sums [P][2C] (null: not carried)
};
struct Side {                // extra problems for infer_state's launches (AFFINE): [0] with conv1 + projection, [1], [2] with conv2
  ConvProblem p[3];
  int n;                     // 2 or 3
};
bool carries_gates1_s(const sf_dual_w& w) { return w.gates1_x.w && w.gates1_s.w && tune().pipe >= 2; }

// ---- The four launch groups of the carried form, each built in ONE place: infer_state and dual_cell issue what these builders return, and
// carry_ok asks sp_takes about the same groups (with placeholder pointers).
// the two side problems of cell `w` on state `s` (= the output of the cell before it)
void side_problems(const sf_dual_w& w, const float* s, const Carry& c, int B, int H, int W, Side& sd) {
  sd.p[0] = gates_problem(w.gates2, s, nullptr, c.g2, s, c.rs2, w.C, B, H, W);
  sd.p[1] = cand_problem(w.cand2, s, s, c.rs2, c.h2, c.g2, w.C, B, H, W);
  sd.p[1].mode = 4;          // blend inside an AFFINE launch
  sd.n = 2;
  if (c.g1s && carries_gates1_s(w)) {      // gates1 = sigmoid(W_x x + [W_s s] + b): the bracket now, raw
    sd.p[2] = problem(w.gates1_s, s, nullptr, c.g1s, B, H, W);
    sd.n = 3;
  }
}
// infer_state launch 1: rb0.conv1 + rb0.proj [+ gates2 of the next cell].  Launch 2: rb0.conv2 (+ residual, channel sums) [+ cand2 of the next
// cell, + the state half of its gates1] — without its scratch pointers, which no launch decision reads: infer_state sizes its scratch by the
// tile width of this launch and fills them in afterwards.  Return the number of problems.
int infer_group1(const sf_pmodel_w& w, const float* s, float* a, float* pr, const Side* side, int B, int H, int W, ConvProblem* ps) {
  ps[0] = problem(w.rb0.conv1, s, nullptr, a, B, H, W);
  ps[1] = problem(w.rb0.proj, s, nullptr, pr, B, H, W);
  if (side) ps[2] = side->p[0];
  return side ? 3 : 2;
}
int infer_group2(const sf_pmodel_w& w, const Side* side, int B, int H, int W, ConvProblem* ps) {
  ps[0] = problem(w.rb0.conv2, nullptr, nullptr, nullptr, B, H, W);
  if (side) { ps[1] = side->p[1]; ps[2] = side->p[2]; }
  return side ? side->n : 1;
}
// the carried cell's gates launch: gates1, or its x half on top of the carried state half (acc_in) ...
ConvProblem carried_gates(const sf_dual_w& w, const float* x, const float* s, float* g1, float* rs1, const float* g1s, int B, int H, int W) {
  ConvProblem g = gates_problem(g1s ? w.gates1_x : w.gates1, x, g1s ? nullptr : s, g1, s, rs1, w.C, B, H, W);
  if (g1s) { g.acc_in = g1s; g.acc_cs = 2 * w.C; }
  return g;
}
// ... and its candidate launch: candidate of cell 1 + blend beside rnn_state2 = conv_decoder_2(h2) of the carried branch
void carried_cand(const sf_dual_w& w, const float* x, const float* s, const CellBufs& b, const float* h2, int B, int H, int W, ConvProblem* ps) {
  ps[0] = cand_problem(w.cand1, x, s, b.rs1, b.h1, b.g1, w.C, B, H, W);
  ps[0].mode = 4;
  ps[1] = problem(w.dec2, h2, nullptr, b.r2, B, H, W);
}

bool carry_ok(const sf_dual_w& w, const sf_pmodel_w& pm, int B, int H, int W) {
  const long P = (long)B * H * W;
  // One latent only.  (Measured with the blend mode / acc_in also in the large-tile AFFINE epilogues: per steady-state step 8 samples
  // 684 -> 669 us, one 200x200 latent 1200 -> 1200, 32 samples 2178 -> 2197 — and the two extra branches cost every AFFINE launch
  // of the batched forward 0.9 % (255.5 -> 257.8 ms): not worth the headline, reverted; profiles/README.md round-3 log.)
  if (!(tune().pipe && B == 1 && P < SP_MAX_P && tune().sp && pregate(P, w.cand1) && pregate(P, w.cand2))) return false;
  if (!pm.rb0.proj.w) return false;
  // The launch GROUPS the carried form issues must all be ones the small-P kernel takes (its AFFINE epilogue alone has the blend
  // mode and acc_in; run() refuses them elsewhere and the rollout would fail instead of falling back — ADVICE r3).  The groups above with
  // every buffer a non-null placeholder: sp_takes never dereferences them.
  float* const ph = reinterpret_cast<float*>(uintptr_t(64));
  const Carry c = {ph, ph, ph, carries_gates1_s(w) ? ph : nullptr};
  const CellBufs b = {ph, ph, ph, ph, ph, ph, ph, ph, ph, ph};
  Side sd = {};
  side_problems(w, ph, c, B, H, W, sd);
  ConvProblem g[3];
  if (!sp_takes(g, infer_group1(pm, ph, ph, ph, &sd, B, H, W, g), EPI_AFFINE)) return false;
  if (!sp_takes(g, infer_group2(pm, &sd, B, H, W, g), EPI_AFFINE)) return false;
  g[0] = carried_gates(w, ph, ph, ph, ph, c.g1s, B, H, W);      // the next cell
  if (!sp_takes(g, 1, EPI_AFFINE)) return false;
  carried_cand(w, ph, ph, b, ph, B, H, W, g);
  return sp_takes(g, 2, EPI_AFFINE);
}

// B images (samples) are processed as one pixel space; coef_stride = floats between the
// coefficient records of consecutive images (0: one record shared by all).  `carry`: gates2 / cand2 of this cell were
// computed beside the previous infer_state (see Carry).
int dual_cell(const sf_dual_w& w, const float* x, const float* s, float* out, int derivative, const float* base,
              const float* coef, int coef_stride, float* out2, int acc2, int B, int H, int W, const CellBufs& b, hipStream_t st,
              const Carry* carry = nullptr) {
  const int C = w.C, P = B * H * W;
  const bool pre = pregate(P, w.cand1) && pregate(P, w.cand2);
  ConvProblem ps[2];
  if (carry) {
    if (!pre) return SF_ERR_INVALID;
    SF_TRY(run1(carried_gates(w, x, s, b.g1, b.rs1, carry->g1s, B, H, W), EPI_AFFINE, st));      // gates of cell 1
    carried_cand(w, x, s, b, carry->h2, B, H, W, ps);
    SF_TRY(run(ps, 2, EPI_AFFINE, st));
    return cell_tail(w, s, out, derivative, base, coef, coef_stride, out2, acc2, b, B, H, W, st);
  }
  float *rs1 = pre ? b.rs1 : nullptr, *rs2 = pre ? b.rs2 : nullptr;
  ps[0] = gates_problem(w.gates1, x, s, b.g1, s, rs1, C, B, H, W);             // gates of both cells in one launch
  ps[1] = gates_problem(w.gates2, s, nullptr, b.g2, s, rs2, C, B, H, W);       // cell 2 sees cat[s,s]: duplicate input folded into the packed weights
  SF_TRY(run(ps, 2, EPI_AFFINE, st));
  ps[0] = cand_problem(w.cand1, x, s, rs1, b.h1, b.g1, C, B, H, W);            // candidates + blend
  ps[1] = cand_problem(w.cand2, s, s, rs2, b.h2, b.g2, C, B, H, W);
  SF_TRY(run(ps, 2, EPI_BLEND, st));
  SF_TRY(run1(problem(w.dec2, b.h2, nullptr, b.r2, B, H, W), EPI_AFFINE, st));   // rnn_state2 = conv_decoder_2(h2)
  return cell_tail(w, s, out, derivative, base, coef, coef_stride, out2, acc2, b, B, H, W, st);
}

constexpr int SE_SLABS = 64;
// scratch of infer_state.  cs1 / cs2: the SE producers' channel sums, [rows][2C] — one image: a row per pixel tile of the producing launch,
// whose kernel (16, 32 or 64 pixels a tile) the plan decides: carved for 16; several images: SE_SLABS slab sums per image
struct InferBufs {
  float *a, *pr, *y1, *b, *y2, *cs1, *cs2, *sc1, *sc2, *slabs;
  void take(Arena& A, int C, int B, size_t HW) {
    const size_t P = B * HW, C2 = 2 * (size_t)C, rows = B == 1 ? (P + 15) / 16 : (size_t)B * SE_SLABS;
    a = A.take(P * C); pr = A.take(P * C2); y1 = A.take(P * C2); b = A.take(P * C2); y2 = A.take(P * C2);
    cs1 = A.take(rows * C2); cs2 = A.take(rows * C2); sc1 = A.take(B * C2); sc2 = A.take(B * C2); slabs = A.take(SE_SLABS * C2);
  }
};

// temporal_ode_bayes.py:463-477 on B images.  SE channel means: B == 1 uses the per-16-pixel sums
// the producing conv's epilogue writes; B > 1 (16-pixel tiles straddle images) sums per-image
// slabs with one extra small launch.  Both are fixed-order.
int infer_state(const sf_pmodel_w& w, const float* s, const float* eps, float* p_out, float* q_out, int B, int H, int W,
                const InferBufs& ib, hipStream_t st, const unsigned long long* philox = nullptr, int draw = 0, const Side* side = nullptr) {
  if (!eps && !philox) return SF_ERR_INVALID;
  const int C = w.C, C2 = 2 * C, HW = H * W, P = B * HW;
  if (B < 1 || B > 64) return SF_ERR_UNSUPPORTED;
  // SE channel means.  One sample: the producing conv's epilogue writes per-tile channel sums ("rows"); a small latent sums
  // them in the consuming layer's prologue (small-P kernel) or in the gate kernel; a large one (thousands of rows) first
  // reduces the rows to SE_SLABS slab sums (two short launches instead of a pass over the whole tensor: 22 -> ~10 us per
  // gate at 200x200).  Several samples (tiles straddle images): per-image slab sums of the tensor.  All fixed-order.
  const bool tiles = (B == 1);
  const bool two_level = tiles && P >= 8192;
  // The launches that write per-tile channel sums, built before the scratch: their kernel's pixel tile (the whole group decides it: the side
  // problems ride in rb0.conv2's launch) says how many rows of sums each SE producer writes
  ConvProblem ps[3], l2[3], c4 = problem(w.rb1.conv2, nullptr, nullptr, nullptr, B, H, W);
  const int n2 = infer_group2(w, side, B, H, W, l2);
  const int tpx1 = chansum_tile_px(l2, n2, EPI_AFFINE), tpx2 = chansum_tile_px(&c4, 1, EPI_AFFINE);
  const int nt1 = tiles ? (P + tpx1 - 1) / tpx1 : SE_SLABS, nt2 = tiles ? (P + tpx2 - 1) / tpx2 : SE_SLABS;
  if (tpx1 < 16 || tpx2 < 16) return SF_ERR_UNSUPPORTED;      // InferBufs carves a row of sums per 16 pixels
  float *a = ib.a, *pr = ib.pr, *y1 = ib.y1, *b = ib.b, *y2 = ib.y2, *cs1 = ib.cs1, *cs2 = ib.cs2, *sc1 = ib.sc1, *sc2 = ib.sc2, *slabs = ib.slabs;
  if (!w.rb0.proj.w || w.rb1.proj.w) return SF_ERR_INVALID;
  auto gate = [&](const float* y, const float* rows, int nrows, const float* fc0, const float* fc2, float* scale) -> int {
    SF_TRY(seg_flush());
    if (!tiles) {
      SF_HIP(launch_chan_partial(y, const_cast<float*>(rows), B, HW, C2, SE_SLABS, st));
      SF_HIP(launch_se_fc(rows, SE_SLABS, C2, C2 / 8, HW, fc0, fc2, scale, B, st));
    } else if (two_level) {
      SF_HIP(launch_chan_partial(rows, slabs, 1, nrows, C2, SE_SLABS, st));      // the [nrows][C2] sums as a one-image "tensor"
      SF_HIP(launch_se_fc(slabs, SE_SLABS, C2, C2 / 8, HW, fc0, fc2, scale, 1, st));
    } else {
      SF_HIP(launch_se_fc(rows, nrows, C2, C2 / 8, HW, fc0, fc2, scale, B, st));
    }
    return SF_OK;
  };
  SF_TRY(run(ps, infer_group1(w, s, a, pr, side, B, H, W, ps), EPI_AFFINE, st));
  l2[0].in0 = a; l2[0].out = y1; l2[0].add = pr; l2[0].chansum = tiles ? cs1 : nullptr;
  SF_TRY(run(l2, n2, EPI_AFFINE, st));
  // SE gates.  One sample on the small-P kernel: the consuming layer computes the gate in its prologue from the
  // producer's per-tile channel sums (two launches fewer per infer_state); otherwise the gate kernel
  ConvProblem c3 = problem(w.rb1.conv1, y1, nullptr, b, B, H, W);
  c3.se_sum = cs1; c3.se_fc0 = w.se0_fc0; c3.se_fc2 = w.se0_fc2; c3.se_out = sc1; c3.se_nt = nt1; c3.se_cr = C2 / 8;
  c3.se_inv_hw = 1.f / (float)HW;
  const bool fuse_se = tiles && sp_takes(&c3, 1, EPI_AFFINE);
  if (!fuse_se) {
    c3.se_sum = nullptr;
    SF_TRY(gate(y1, cs1, nt1, w.se0_fc0, w.se0_fc2, sc1));
    c3.in_scale = sc1;
  }
  SF_TRY(run1(c3, EPI_AFFINE, st));
  c4.in0 = b; c4.out = y2; c4.add = y1; c4.add_scale = sc1; c4.chansum = tiles ? cs2 : nullptr;
  SF_TRY(run1(c4, EPI_AFFINE, st));
  ConvProblem c5 = problem(w.last, y2, nullptr, p_out, B, H, W);
  c5.e0 = eps; c5.out2 = q_out; c5.philox = philox; c5.draw = draw;
  if (fuse_se) {
    c5.se_sum = cs2; c5.se_fc0 = w.se1_fc0; c5.se_fc2 = w.se1_fc2; c5.se_out = nullptr; c5.se_nt = nt2; c5.se_cr = C2 / 8;
    c5.se_inv_hw = 1.f / (float)HW;
  }
  if (!fuse_se || !sp_takes(&c5, 1, EPI_SAMPLE)) {
    c5.se_sum = nullptr;
    SF_TRY(gate(y2, cs2, nt2, w.se1_fc0, w.se1_fc2, sc2));
    c5.in_scale = sc2;
  }
  return run1(c5, EPI_SAMPLE, st);
}

// ---- solver stages ----------------------------------------------------------------------------------------------------------
// A stage = one dual cell (ODE derivative + integrator update, or a Bayesian jump) followed by an optional infer_state.
struct Stage {              // (the defaults: an inner stage of an ODE step)
  const sf_dual_w* w = nullptr;
  const float* x = nullptr; const float* s = nullptr; float* out = nullptr;
  int derivative = 1; const float* base = nullptr; const float* coef = nullptr; float* out2 = nullptr; int acc2 = 0;
  bool infer_after = true; int draw = 0; float* p_out = nullptr;
  int op_end = -1;      // index of the op this stage completes (-1: an inner solver stage)
};
// [P][C] each; midpoint uses three, Euler none: the size query is not told the solver
struct StageBufs { float *k, *pk, *acc, *s3; void take(Arena& A, size_t PC) { k = A.take(PC); pk = A.take(PC); acc = A.take(PC); s3 = A.take(PC); } };

// One ODE step (temporal_ode_bayes.py:436-461, + build-defined RK4) of cell `w` as 1, 2 or 4 stages appended to `out`: input x (the
// imputed input, or zeros with IMPUTE off), state s -> s2, and infer_state(s2) -> p2 where need_p.  cf: the step's coefficient record
// (SF_COEF_STRIDE in sfnative.h); draws are numbered from `draw`.  Returns the number of draws (a skipped infer_state keeps its number).
int step_stages(int solver, const sf_dual_w* w, const float* x, const float* s, float* s2, float* p2, bool need_p, const float* cf, int draw,
                int op, const StageBufs& b, std::vector<Stage>& out) {
  if (solver == SF_SOLVER_EULER) {
    out.push_back({.w = w, .x = x, .s = s, .out = s2, .base = s, .coef = cf + 0, .infer_after = need_p, .draw = draw, .p_out = p2, .op_end = op});
    return 1;
  }
  if (solver == SF_SOLVER_MIDPOINT) {
    // k = s + dt/2 f(p, s); pk = infer(k) (:452 — evaluated even when IMPUTE is off: only :443's input is zeroed); s' = s + dt f(pk, k)
    out.push_back({.w = w, .x = x, .s = s, .out = b.k, .base = s, .coef = cf + 1, .draw = draw, .p_out = b.pk});
    out.push_back({.w = w, .x = b.pk, .s = b.k, .out = s2, .base = s, .coef = cf + 0, .infer_after = need_p, .draw = draw + 1, .p_out = p2, .op_end = op});
    return 2;
  }
  // RK4: cf = {dt, dt/2, dt/6, dt/3, ...}.  acc = s + dt/6 k1 + dt/3 k2 + dt/3 k3 ; s' = acc + dt/6 k4.  Stage coefficient pairs {out coef,
  // out2 coef} follow the four scalars in the record: {dt/2, dt/6}, {dt/2, dt/3}, {dt, dt/3}, {dt/6, 0}; stage inputs always come from
  // infer_state, as in midpoint; the fourth stage state reuses k
  const float* rk = cf + 4;
  out.push_back({.w = w, .x = x, .s = s, .out = b.k, .base = s, .coef = rk + 0, .out2 = b.acc, .draw = draw, .p_out = b.pk});
  out.push_back({.w = w, .x = b.pk, .s = b.k, .out = b.s3, .base = s, .coef = rk + 2, .out2 = b.acc, .acc2 = 1, .draw = draw + 1, .p_out = b.pk});
  out.push_back({.w = w, .x = b.pk, .s = b.s3, .out = b.k, .base = s, .coef = rk + 4, .out2 = b.acc, .acc2 = 1, .draw = draw + 2, .p_out = b.pk});
  out.push_back({.w = w, .x = b.pk, .s = b.k, .out = s2, .base = b.acc, .coef = rk + 6, .infer_after = need_p, .draw = draw + 3, .p_out = p2, .op_end = op});
  return 4;
}

// One stand-alone step: its stages one after the other, every cell and every infer_state on its own (no carried branch, no persistent flow).
// `zeros`: [P][C] zero tensor (IMPUTE=False); the solver stages; a cell's scratch overlays the infer_state's behind it.
struct StepLayout {
  SplitBufs split;
  float* zeros;
  StageBufs sb;
  CellBufs cell;
  InferBufs inf;
  void take(Arena& A, int C, int B, size_t HW) {
    split.take(A);
    zeros = A.take(B * HW * C);
    sb.take(A, B * HW * C);
    A.larger_of([&] { cell.take(A, C, B * HW); }, [&] { inf.take(A, C, B, HW); });
  }
};
int ode_step(const sf_dual_w& gc, const sf_pmodel_w& pm, int solver, int impute, const float* s_in, const float* p_in, const float* coef,
             int coef_stride, const float* eps, float* s_out, float* p_out, const StepLayout& L, int B, int H, int W, hipStream_t st) {
  const size_t PC = (size_t)B * H * W * gc.C;
  std::vector<Stage> stages;
  step_stages(solver, &gc, impute ? p_in : L.zeros, s_in, s_out, p_out, true, coef, 0, 0, L.sb, stages);
  for (const Stage& g : stages) {
    SF_TRY(dual_cell(*g.w, g.x, g.s, g.out, g.derivative, g.base, g.coef, coef_stride, g.out2, g.acc2, B, H, W, L.cell, st));
    if (g.infer_after) SF_TRY(infer_state(pm, g.out, eps + (size_t)g.draw * PC, g.p_out, nullptr, B, H, W, L.inf, st));
  }
  return SF_OK;
}

// ResBlock (res_models.py:74-79) on n images; t: [P][cin] scratch, pr: [P][cout] scratch (if proj)
// `pooled` (optional): MaxPool2d(2) of the block's output, [n][H/2][W/2][C]; written by the last convolution's own epilogue where the
// Winograd kernel runs it (`out` is then not written at all), by a pooling launch after it otherwise
int res_block(const sf_res_w& w, const float* x, float* out, float* t, float* pr, int n, int Hin, int Win, int in_up,
              hipStream_t st, float* pooled = nullptr) {
  ConvProblem c2 = problem(w.conv2, t, nullptr, out, n, Hin << in_up, Win << in_up);
  c2.add = w.proj.w ? pr : x;
  if (!w.proj.w && in_up) {
    // identity skip of an input that is upsampled on read: the Winograd epilogue reads the half-size tensor itself (one source pixel
    // per tile); anywhere else the caller has to materialise the upsampled input (SF_ERR_UNSUPPORTED before anything is launched)
    c2.add_up = 1;
    if (!wino_runs(c2, EPI_AFFINE)) return SF_ERR_UNSUPPORTED;
  }
  ConvProblem ps[2];
  ps[0] = problem(w.conv1, x, nullptr, t, n, Hin, Win, in_up);
  int np = 1;
  if (w.proj.w) { ps[1] = problem(w.proj, x, nullptr, pr, n, Hin, Win, in_up); np = 2; }
  SF_TRY(run(ps, np, EPI_AFFINE, st));
  if (pooled) {
    ConvProblem cp = c2;
    cp.pool2 = 1; cp.out = pooled;
    if (wino_runs(cp, EPI_AFFINE)) return run1(cp, EPI_AFFINE, st);
    SF_TRY(run1(c2, EPI_AFFINE, st));
    SF_HIP(launch_maxpool2(out, pooled, n, c2.Hout, c2.Wout, c2.cout, 0, st));
    return SF_OK;
  }
  return run1(c2, EPI_AFFINE, st);
}

}  // namespace

// =================================================================================================
extern "C" {

int sf_version(void) { return 110; }

// ABI guard (include/sfnative.h): the sizes this translation unit was compiled with
int sf_abi_version(void) { return SF_ABI_VERSION; }
size_t sf_abi_sizeof(int which) {
  switch (which) {
    case SF_STRUCT_CONV_W: return sizeof(sf_conv_w);
    case SF_STRUCT_GRU_W: return sizeof(sf_gru_w);
    case SF_STRUCT_DUAL_W: return sizeof(sf_dual_w);
    case SF_STRUCT_RES_W: return sizeof(sf_res_w);
    case SF_STRUCT_PMODEL_W: return sizeof(sf_pmodel_w);
    case SF_STRUCT_ENCODER_W: return sizeof(sf_encoder_w);
    case SF_STRUCT_DECODER_W: return sizeof(sf_decoder_w);
    case SF_STRUCT_CONVNEXT_W: return sizeof(sf_convnext_w);
    case SF_STRUCT_DEEPLAB_W: return sizeof(sf_deeplab_w);
    case SF_STRUCT_BOTTLENECK_W: return sizeof(sf_bottleneck_w);
    case SF_STRUCT_BOTTLE_W: return sizeof(sf_bottle_w);
  }
  return 0;
}
int sf_abi_check(int abi_version, const size_t* struct_sizes, int n) {
  if (abi_version != SF_ABI_VERSION || !struct_sizes || n != SF_STRUCT_COUNT) return SF_ERR_INVALID;
  for (int i = 0; i < n; ++i)
    if (struct_sizes[i] != sf_abi_sizeof(i)) return SF_ERR_INVALID;
  return SF_OK;
}

const char* sf_status_string(int s) {
  switch (s) {
    case SF_OK: return "ok";
    case SF_ERR_INVALID: return "invalid argument";
    case SF_ERR_WORKSPACE: return "workspace too small";
    case SF_ERR_LAUNCH: return "HIP launch/runtime error";
    case SF_ERR_UNSUPPORTED: return "unsupported shape";
  }
  return "unknown";
}

int sf_nchw_to_nhwc(const float* src, float* dst, int n, int C, int HW, void* stream) {
  if (!src || !dst) return SF_ERR_INVALID;
  SF_HIP(launch_transpose(src, dst, n, C, HW, (hipStream_t)stream));
  return SF_OK;
}
int sf_nhwc_to_nchw(const float* src, float* dst, int n, int C, int HW, void* stream) {
  if (!src || !dst) return SF_ERR_INVALID;
  SF_HIP(launch_transpose(src, dst, n, HW, C, (hipStream_t)stream));
  return SF_OK;
}

/* the same with the n images `src_stride` / `dst_stride` floats apart (>= C*HW): frames picked out of / written into a
 * larger [B][T][C][H][W] tensor without an intermediate copy */
int sf_nchw_to_nhwc_strided(const float* src, size_t src_stride, float* dst, size_t dst_stride, int n, int C, int HW, void* stream) {
  if (!src || !dst || src_stride < (size_t)C * HW || dst_stride < (size_t)C * HW) return SF_ERR_INVALID;
  SF_HIP(launch_transpose_strided(src, dst, n, C, HW, src_stride, dst_stride, (hipStream_t)stream));
  return SF_OK;
}
int sf_nhwc_to_nchw_strided(const float* src, size_t src_stride, float* dst, size_t dst_stride, int n, int C, int HW, void* stream) {
  if (!src || !dst || src_stride < (size_t)C * HW || dst_stride < (size_t)C * HW) return SF_ERR_INVALID;
  SF_HIP(launch_transpose_strided(src, dst, n, HW, C, src_stride, dst_stride, (hipStream_t)stream));
  return SF_OK;
}

int sf_conv2d_fwd(const sf_conv_w* w, const float* in0, const float* in1, const float* add, float* out, int n_img,
                  int Hin, int Win, int in_up, void* stream) {
  if (!w || !valid_w(*w) || !in0 || !out || (w->c1 > 0 && !in1)) return SF_ERR_INVALID;
  ConvProblem p = problem(*w, in0, in1, out, n_img, Hin, Win, in_up);
  p.add = add;
  return run1(p, EPI_AFFINE, (hipStream_t)stream);
}

// The same with channel-sliced operands (a layer reading / writing a channel range of a wider NHWC
// tensor, e.g. the stacked heads of the BEV decoder), the residual added before the activation
// (ResNet BasicBlock) and optional split-K scratch for mid-sized pixel counts.
int sf_conv2d_ex_fwd(const sf_conv_w* w, const float* in0, int in0_cs, const float* in1, int in1_cs, const float* add, int add_cs,
                     int act_after_add, float* out, int out_cs, int out_co, int n_img, int Hin, int Win, int in_up, float* ws,
                     size_t ws_bytes, void* stream) {
  if (!w || !valid_w(*w) || !in0 || !out || (w->c1 > 0 && !in1)) return SF_ERR_INVALID;
  if (in0_cs < w->c0 || (w->c1 > 0 && in1_cs < w->c1) || out_cs < out_co + w->cout || (in0_cs % 4) || (out_cs % 4) || (out_co % 4) ||
      (add && (add_cs < w->cout || (add_cs % 4))))
    return SF_ERR_INVALID;
  SplitBufs split;
  carve(split, ws, ws_bytes);      // optional scratch: what does not fit stays null, and the call runs without split-K
  SplitScope sp(split, (hipStream_t)stream);
  ConvProblem p = problem(*w, in0, in1, out, n_img, Hin, Win, in_up);
  p.in0_cs = in0_cs;
  if (w->c1 > 0) p.in1_cs = in1_cs;
  p.add = add;
  if (add) p.add_cs = add_cs;
  p.out_cs = out_cs;
  p.out_co = out_co;
  if (act_after_add) p.mode |= 2;
  return run1(p, EPI_AFFINE, (hipStream_t)stream);
}
size_t sf_conv2d_ex_ws_bytes(void) { return layout_bytes<SplitBufs>(); }

/* UpsamplingAdd tail — convolutions.py:208,215: out = bilinear_x2(in) + skip (skip may be NULL) */
int sf_upsample_bilinear2_add_fwd(const float* in, const float* skip, float* out, int n, int Hin, int Win, int C, void* stream) {
  if (!in || !out || n < 1 || Hin < 1 || Win < 1 || C < 4 || (C % 4)) return SF_ERR_INVALID;
  SF_HIP(launch_upsample_bilinear2_add(in, skip, out, n, Hin, Win, C, (hipStream_t)stream));
  return SF_OK;
}

/* sparse (gather) convolution: out[j] = act(scale * sum_t W_t . feats[nbr[j][t]] + bias) (+ add), see sfnative.h; with an optional tap
 * mask: tile_mask64[i] bit t = some row of 64 i .. 64 i + 63 has an input row under tap t */
int sf_sparse_conv_masked_fwd(const sf_conv_w* w, const float* feats, int feats_cs, int n_in, const int32_t* nbr, const uint32_t* tile_mask64, int n_out,
                              const float* add, int act_after_add, float* out, float* ws, size_t ws_bytes, void* stream) {
  if (!w || !valid_w(*w) || !feats || !nbr || !out || n_out < 0 || n_in < 1 || w->kw != 1 || w->c1 != 0 || feats_cs < w->c0 ||
      (feats_cs % 4))
    return SF_ERR_INVALID;
  if (n_out == 0) return SF_OK;
  SplitBufs split;
  carve(split, ws, ws_bytes);      // optional scratch: what does not fit stays null, and the call runs without split-K
  SplitScope sp(split, (hipStream_t)stream);
  ConvProblem p = problem(*w, feats, nullptr, out, 1, 1, n_in, 0);   // the input "image" is the n_in feature rows
  p.in0_cs = feats_cs;
  p.Hout = 1; p.Wout = n_out;
  p.gather = nbr;
  p.tap_mask = tile_mask64; p.tap_mask_n = tile_mask64 ? (n_out + 63) / 64 : 0;
  p.add = add;
  if (act_after_add) p.mode |= 2;
  return run1(p, EPI_AFFINE, (hipStream_t)stream);
}
int sf_sparse_conv_fwd(const sf_conv_w* w, const float* feats, int feats_cs, int n_in, const int32_t* nbr, int n_out,
                       const float* add, int act_after_add, float* out, float* ws, size_t ws_bytes, void* stream) {
  return sf_sparse_conv_masked_fwd(w, feats, feats_cs, n_in, nbr, nullptr, n_out, add, act_after_add, out, ws, ws_bytes, stream);
}

/* per-image channel means of an NHWC tensor (fixed-order two-level sum: reproducible) */
struct MeanBufs { float* part; void take(Arena& A, int C, int n) { part = A.take((size_t)n * 64 * C); } };      // 64 slab sums per image
size_t sf_channel_mean_ws_bytes(int C, int n) { return layout_bytes<MeanBufs>(C, n); }
int sf_channel_mean_fwd(const float* x, float* out, int n, int HW, int C, float* ws, size_t ws_bytes, void* stream) {
  if (!x || !out || n < 1 || HW < 1 || C < 4 || (C % 4) || C > 1024) return SF_ERR_INVALID;
  MeanBufs b;
  if (!carve(b, ws, ws_bytes, C, n)) return SF_ERR_WORKSPACE;
  SF_HIP(launch_chan_partial(x, b.part, n, HW, C, 64, (hipStream_t)stream));
  SF_HIP(launch_mean_from_partials(b.part, out, n, 64, C, HW, (hipStream_t)stream));
  return SF_OK;
}
/* elementwise LogSigmoid (DistributionModule(method='BERNOULLI'), streamingflow/models/distributions.py:33, :47) */
int sf_logsigmoid_fwd(const float* x, float* out, size_t n, void* stream) {
  if (!x || !out) return SF_ERR_INVALID;
  if (n == 0) return SF_OK;
  SF_HIP(launch_logsigmoid(x, out, n, (hipStream_t)stream));
  return SF_OK;
}
/* out[img][pixel][out_co .. out_co+k) = vec[img][0..k) for every pixel (k, out_cs, out_co multiples of 4) */
int sf_broadcast_channels_fwd(const float* vec, float* out, int n, int HW, int k, int out_cs, int out_co, void* stream) {
  if (!vec || !out || n < 1 || HW < 1 || k < 4 || (k % 4) || (out_cs % 4) || (out_co % 4) || out_co + k > out_cs) return SF_ERR_INVALID;
  SF_HIP(launch_broadcast_channels(vec, out, n, HW, k, out_cs, out_co, (hipStream_t)stream));
  return SF_OK;
}

// benchmarking aid: the same fused conv enqueued `reps` times back to back from C++ (no per-launch
// host-language overhead); ws may be NULL (then no cross-workgroup split-K scratch is available)
int sf_conv2d_repeat(const sf_conv_w* w, const float* in0, const float* in1, const float* add, float* out, int n_img,
                     int Hin, int Win, int in_up, int reps, float* ws, size_t ws_bytes, void* stream) {
  if (!w || !valid_w(*w) || !in0 || !out || (w->c1 > 0 && !in1)) return SF_ERR_INVALID;
  SplitBufs split;
  carve(split, ws, ws_bytes);      // optional scratch: what does not fit stays null, and the call runs without split-K
  SplitScope sp(split, (hipStream_t)stream);
  ConvProblem p = problem(*w, in0, in1, out, n_img, Hin, Win, in_up);
  p.add = add;
  for (int i = 0; i < reps; ++i) SF_TRY(run1(p, EPI_AFFINE, (hipStream_t)stream));
  return SF_OK;
}

size_t sf_gru_cell_ws_bytes(int C, int n_img, int H, int W) { return layout_bytes<GruBufs>(C, (size_t)n_img * H * W); }
static int gru_cell_entry(const sf_gru_w* w, const float* x, const float* s, float* out, int n_img, int H, int W, float* ws, size_t ws_bytes,
                          void* stream, int ode_derivative) {
  if (!w || !x || !s || !out || !valid_w(w->gates) || !valid_w(w->cand)) return SF_ERR_INVALID;
  GruBufs b;
  if (!carve(b, ws, ws_bytes, w->cand.cout, (size_t)n_img * H * W)) return SF_ERR_WORKSPACE;
  return gru_cell(*w, x, s, out, b.g, b.rs, n_img, H, W, (hipStream_t)stream, ode_derivative);
}
int sf_gru_cell_fwd(const sf_gru_w* w, const float* x, const float* s, float* out, int n_img, int H, int W, float* ws,
                    size_t ws_bytes, void* stream) {
  return gru_cell_entry(w, x, s, out, n_img, H, W, ws, ws_bytes, stream, 0);
}
// SpatialGRUODECell.forward — temporal_ode_bayes.py:35-61: dh = u * (h~ - s)
int sf_gru_ode_cell_fwd(const sf_gru_w* w, const float* x, const float* s, float* out, int n_img, int H, int W, float* ws,
                        size_t ws_bytes, void* stream) {
  return gru_cell_entry(w, x, s, out, n_img, H, W, ws, ws_bytes, stream, 1);
}

size_t sf_spatial_gru_ws_bytes(int C, int n_img, int H, int W) { return layout_bytes<SpatialGruBufs>(C, (size_t)n_img * H * W); }
int sf_spatial_gru_fwd(const sf_gru_w* w, const float* x, const float* state0, float* out, int T, int n_img, int H,
                       int W, float* ws, size_t ws_bytes, void* stream) {
  if (!w || !x || !state0 || !out || !valid_w(w->gates) || !valid_w(w->cand)) return SF_ERR_INVALID;
  const bool has_dec = w->decoder.w != nullptr;
  if (has_dec && !valid_w(w->decoder)) return SF_ERR_INVALID;
  const int C = w->cand.cout, Cx = w->gates.c0;
  const size_t P = (size_t)n_img * H * W;
  SpatialGruBufs b;
  if (!carve(b, ws, ws_bytes, C, P)) return SF_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const float* cur = state0;
  for (int t = 0; t < T; ++t) {   // temporal.py:35-39
    // without a decoder (BEVerse SpatialGRU, basic_modules.py:225-284) the states ARE the output
    float* nxt = has_dec ? ((t & 1) ? b.sb : b.sa) : out + t * P * C;
    SF_TRY(gru_cell(*w, x + t * P * Cx, cur, nxt, b.g, b.rs, n_img, H, W, st));
    if (has_dec)
      SF_TRY(run1(problem(w->decoder, nxt, nullptr, out + t * P * w->decoder.cout, n_img, H, W), EPI_AFFINE, st));
    cur = nxt;
  }
  return SF_OK;
}

size_t sf_dual_cell_ws_bytes(int C, int n_img, int H, int W) { return layout_bytes<WithSplit<CellBufs>>(C, (size_t)n_img * H * W); }
int sf_dual_cell_fwd(const sf_dual_w* w, const float* x, const float* s, float* out, int derivative, const float* base,
                     const float* coef, float* out2, int acc2, int n_img, int H, int W, float* ws, size_t ws_bytes,
                     void* stream) {
  if (!w || !x || !s || !out || w->C <= 0 || (w->C % 8) || n_img < 1) return SF_ERR_INVALID;
  if (w->C > 128) return SF_ERR_UNSUPPORTED;
  WithSplit<CellBufs> L;
  if (!carve(L, ws, ws_bytes, w->C, (size_t)n_img * H * W)) return SF_ERR_WORKSPACE;
  SplitScope sp(L.split, (hipStream_t)stream);
  return dual_cell(*w, x, s, out, derivative, base, coef, 0, out2, acc2, n_img, H, W, L.bufs, (hipStream_t)stream);
}

// trusting gate + mix of two given branch states (the tail of both dual cells; the recurrent Dual_GRU calls it per step)
int sf_trust_mix_fwd(const sf_dual_w* w, const float* r1, const float* r2, const float* s, float* out, int derivative,
                     const float* base, const float* coef, int n_img, int H, int W, float* ws, size_t ws_bytes, void* stream) {
  if (!w || !r1 || !r2 || !out || w->C <= 0 || (w->C % 8) || n_img < 1) return SF_ERR_INVALID;
  if (derivative && (!s || !coef)) return SF_ERR_INVALID;
  if (w->C > 128) return SF_ERR_UNSUPPORTED;
  WithSplit<CellBufs> L;
  if (!carve(L, ws, ws_bytes, w->C, (size_t)n_img * H * W)) return SF_ERR_WORKSPACE;
  SplitScope sp(L.split, (hipStream_t)stream);
  CellBufs& b = L.bufs;
  b.h1 = const_cast<float*>(r1);      // read only from here on
  b.r2 = const_cast<float*>(r2);
  return cell_tail(*w, s ? s : r1, out, derivative, base, coef, 0, nullptr, 0, b, n_img, H, W, (hipStream_t)stream);
}

// Bottleblock (convolutions.py:348-380) on cat[x0, x1]: out = layers(x) + (projection(x) | x)
// mid = cin / 2 channels after the 7x7 and the 1x1 layer; the projection's buffer is carved whether or not the block has one
struct BottleBufs {
  float *t1, *t2, *sk;
  void take(Arena& A, int cin, int cout, size_t P) {
    const size_t mid = cin / 2 > 0 ? cin / 2 : 1;
    t1 = A.take(P * mid); t2 = A.take(P * mid); sk = A.take(P * cout);
  }
};
size_t sf_bottleblock_ws_bytes(int cin, int cout, int n_img, int H, int W) { return layout_bytes<WithSplit<BottleBufs>>(cin, cout, (size_t)n_img * H * W); }
int sf_bottleblock_fwd(const sf_bottle_w* w, const float* x0, const float* x1, float* out, int n_img, int H, int W, float* ws,
                       size_t ws_bytes, void* stream) {
  if (!w || !x0 || !out || n_img < 1 || !valid_w(w->c7) || !valid_w(w->c1) || !valid_w(w->c3)) return SF_ERR_INVALID;
  const bool has_proj = w->proj.w != nullptr;
  if (!has_proj && (x1 || w->c7.c1 != 0 || w->c3.cout != w->c7.c0)) return SF_ERR_INVALID;      // the residual is x itself
  if (w->c7.cout_pad > 128 || w->c3.cout_pad > 128) return SF_ERR_UNSUPPORTED;                    // LayerNorm epilogue: all channels of a pixel in one wave
  const int cin = w->c7.c0 + w->c7.c1, cout = w->c3.cout;      // the size query's arguments
  if (w->c7.cout > cin / 2 || w->c1.cout > cin / 2 || (has_proj && w->proj.cout != cout)) return SF_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  WithSplit<BottleBufs> L;
  if (!carve(L, ws, ws_bytes, cin, cout, (size_t)n_img * H * W)) return SF_ERR_WORKSPACE;
  SplitScope sp(L.split, st);
  const auto [t1, t2, sk] = L.bufs;
  ConvProblem ps[2];
  ps[0] = problem(w->c7, x0, x1, t1, n_img, H, W); ps[0].mode = 1;        // 7x7 + LN + GELU
  ConvProblem q = problem(w->c1, t1, nullptr, t2, n_img, H, W); q.mode = 1;
  if (has_proj) { ps[1] = problem(w->proj, x0, x1, sk, n_img, H, W); ps[1].mode = 0; }   // 1x1 + GELU
  const bool fused = fuse_following_1x1(ps, has_proj ? 2 : 1, q, w->c1, t2);
  SF_TRY(run(ps, has_proj ? 2 : 1, EPI_LNG, st));
  if (!fused) SF_TRY(run1(q, EPI_LNG, st));
  ConvProblem f = problem(w->c3, t2, nullptr, out, n_img, H, W); f.mode = 1;
  f.add = has_proj ? sk : x0;
  f.add_cs = has_proj ? w->proj.cout : w->c7.c0;
  return run1(f, EPI_LNG, st);
}

size_t sf_infer_state_ws_bytes(int C, int n_img, int H, int W) { return layout_bytes<WithSplit<InferBufs>>(C, n_img, (size_t)H * W); }
int sf_infer_state_fwd(const sf_pmodel_w* w, const float* s, const float* eps, float* p_out, float* q_out, int n_img,
                       int H, int W, float* ws, size_t ws_bytes, void* stream) {
  if (!w || !s || !eps || !p_out || w->C <= 0 || (w->C % 8) || n_img < 1) return SF_ERR_INVALID;
  WithSplit<InferBufs> L;
  if (!carve(L, ws, ws_bytes, w->C, n_img, (size_t)H * W)) return SF_ERR_WORKSPACE;
  SplitScope sp(L.split, (hipStream_t)stream);
  return infer_state(*w, s, eps, p_out, q_out, n_img, H, W, L.bufs, (hipStream_t)stream);
}

size_t sf_ode_step_ws_bytes(int C, int n_img, int H, int W) { return layout_bytes<StepLayout>(C, n_img, (size_t)H * W); }
int sf_ode_step_fwd(const sf_dual_w* gru_c, const sf_pmodel_w* pm, int solver, int impute, const float* state_in,
                    const float* p_in, const float* coef, const float* eps, float* state_out, float* p_out, int n_img,
                    int H, int W, float* ws, size_t ws_bytes, void* stream) {
  if (!gru_c || !pm || !state_in || !p_in || !coef || !eps || !state_out || !p_out || n_img < 1) return SF_ERR_INVALID;
  if (gru_c->C > 128 || (gru_c->C % 8)) return SF_ERR_UNSUPPORTED;
  if (solver != SF_SOLVER_EULER && solver != SF_SOLVER_MIDPOINT && solver != SF_SOLVER_RK4) return SF_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  StepLayout L;
  if (!carve(L, ws, ws_bytes, gru_c->C, n_img, (size_t)H * W)) return SF_ERR_WORKSPACE;
  SplitScope sp(L.split, st);
  if (!impute) SF_HIP(zero_fill(L.zeros, al((size_t)n_img * H * W * gru_c->C) * sizeof(float), st));
  return ode_step(*gru_c, *pm, solver, impute, state_in, p_in, coef, 0, eps, state_out, p_out, L, n_img, H, W, st);
}

// ---- rollout as a list of stages -----------------------------------------------------------------------------------------
// (Measured and rejected, profiles/README.md "two-stream rollout": running gru_cell_2 / conv_decoder_2 of stage j+1 on a
// second stream beside stage j's infer_state — they only need the state — made the 18-op rollout 11 % slower: every
// small-P workgroup owns a whole CU, so the two chains take turns instead of overlapping, and the split launches lose
// the grouping of the two gate / candidate convolutions.)

// What a resumed segment takes over from / hands on to its neighbours besides the state and the imputed input: the carried branch 2
// of the ODE cell that follows the boundary (struct Carry), [g2 2PC | g1s 2PC | rs2 PC | h2 PC] in caller memory.
struct ResumeCarry {
  const float* in = nullptr;         // written by the segment before this one (first op an ODE step: consumed)
  float* out = nullptr;              // written beside the last infer_state of this segment
  const sf_dual_w* next_w = nullptr; // the cell after the boundary (gru_c)
  bool allow_flow = true;            // false: launch-per-layer form whatever SF_PERSIST / sf_set_flow_mode say
  int draw0 = 0;                     // number of the segment's first draw: eps holds the segment's own draws, Philox is keyed by the number
};
// sf_nnfo_rollout_carry_bytes of caller memory
struct CarryView : Carry { void take(Arena& A, size_t PC) { g2 = A.take(2 * PC); g1s = A.take(2 * PC); rs2 = A.take(PC); h2 = A.take(PC); } };
Carry carry_view(float* base, size_t PC) { CarryView c; carve(c, base, ~size_t(0), PC); return c; }

// The workspace of a rollout: the state / input pairs the ops alternate between, the solver stages, the carried branch 2 (written during
// one stage's infer_state, read by the next cell: outside the overlay), the persistent flow's tables under the flow mode in force, and
// every stage's cell scratch overlaid with the infer_state's behind it
struct RolloutLayout {
  SplitBufs split;
  float *zeros, *sbuf[2], *pbuf[2];
  StageBufs sb;
  Carry cb;
  FlowBufs flow;
  CellBufs cell;
  InferBufs inf;
  void take(Arena& A, int C, int B, size_t HW) {
    const size_t PC = B * HW * C;
    split.take(A);
    zeros = A.take(PC);
    sbuf[0] = A.take(PC); sbuf[1] = A.take(PC); pbuf[0] = A.take(PC); pbuf[1] = A.take(PC);
    sb.take(A, PC);
    cb.g2 = A.take(2 * PC); cb.rs2 = A.take(PC); cb.h2 = A.take(PC); cb.g1s = A.take(2 * PC);
    flow.take(A);
    A.larger_of([&] { cell.take(A, C, B * HW); }, [&] { inf.take(A, C, B, HW); });
  }
};

int run_stages(const std::vector<Stage>& stages, const sf_pmodel_w& pm, const float* eps, const unsigned long long* philox, int coef_stride,
               const int32_t* sel_nops, int n_targets, float* out_states, int B, int H, int W, const RolloutLayout& L, hipStream_t st,
               const unsigned** flow_err, const ResumeCarry& rc = ResumeCarry()) {
  const size_t PC = (size_t)B * H * W * pm.C;
  const Carry& cb = L.cb;
  Carry cnow = cb;
  // one latent: the launch groups of the stages become phases of ONE persistent flow launch (conv_sp.hip: sp_flow_kernel)
  FlowScope flow(rc.allow_flow && B == 1 && (long)B * H * W < SP_MAX_P && tune().sp, L.flow, st);      // for the duration of this function only
  SF_TRY(flow.status);
  *flow_err = flow.err();
  bool carried = false;
  // a resumed segment that starts with an ODE step: branch 2 of its first cell was computed beside the infer_state that closed the
  // segment before it (rc.in), exactly as the unsplit rollout computes it beside the infer_state of the op before
  if (rc.in && !stages.empty() && stages[0].derivative && carry_ok(*stages[0].w, pm, B, H, W)) {
    cnow = carry_view(const_cast<float*>(rc.in), PC);
    if (!carries_gates1_s(*stages[0].w)) cnow.g1s = nullptr;
    carried = true;
  }
  for (size_t j = 0; j < stages.size(); ++j) {
    const Stage& g = stages[j];
    SF_TRY(dual_cell(*g.w, g.x, g.s, g.out, g.derivative, g.base, g.coef, coef_stride, g.out2, g.acc2, B, H, W, L.cell, st, carried ? &cnow : nullptr));
    carried = false;
    if (g.op_end >= 0)
      for (int t = 0; t < n_targets; ++t)
        if (sel_nops[t] == g.op_end + 1) {
          SF_TRY(flow_copy_out(g.out, out_states + (size_t)t * PC, PC, st));
        }
    if (g.infer_after) {
      Side sd = {};
      const Stage* nx = j + 1 < stages.size() ? &stages[j + 1] : nullptr;
      // the last infer_state of a segment that hands its boundary on (rc.out): the side problems of the ODE cell that follows it
      const sf_dual_w* nw = nx ? (nx->s == g.out ? nx->w : nullptr) : (rc.out ? rc.next_w : nullptr);
      const bool pipe = nw && carry_ok(*nw, pm, B, H, W);
      if (pipe) {
        side_problems(*nw, g.out, nx ? cb : carry_view(rc.out, PC), B, H, W, sd);
        cnow = cb;
        if (sd.n < 3) cnow.g1s = nullptr;
      }
      SF_TRY(infer_state(pm, g.out, eps ? eps + (size_t)(g.draw - rc.draw0) * PC : nullptr, g.p_out, nullptr, B, H, W, L.inf, st, philox, g.draw, pipe ? &sd : nullptr));
      carried = pipe && nx;
    }
  }
  return seg_flush();
}

size_t sf_nnfo_rollout_ws_bytes(int C, int n_img, int H, int W) { return layout_bytes<RolloutLayout>(C, n_img, (size_t)H * W); }
size_t sf_nnfo_rollout_carry_bytes(int C, int n_img, int H, int W) { return layout_bytes<CarryView>((size_t)n_img * H * W * C); }
struct SegmentIO {      // what only a resumed segment is given (sfnative.h: sf_nnfo_rollout_resume_fwd)
  const float* state_in = nullptr; const float* p_in = nullptr; const float* carry_in = nullptr; int draw_base = 0;
  float* p_out = nullptr; float* carry_out = nullptr;
};
// One segment of the rollout.  state_in / p_in (NULL: zeros) are read, never written; draws are numbered from draw_base; p_out != NULL
// keeps the infer_state of the last op.  The one-shot entry points are this with an empty SegmentIO.
static int rollout_core(const sf_dual_w* gru_c, const sf_dual_w* gru_obs, const sf_pmodel_w* pm, int solver, int impute,
                        const int32_t* ops, int n_ops, const float* hx_obs, const float* eps, const unsigned long long* philox,
                        const float* coef, int coef_per_image, const int32_t* sel_nops, int n_targets, float* out_states,
                        float* final_state, int n_img, int H, int W, float* ws, size_t ws_bytes, void* stream, const SegmentIO& io = SegmentIO()) {
  const auto [state_in, p_in, carry_in, draw_base, p_out, carry_out] = io;
  if (!gru_c || !gru_obs || !pm || (!ops && n_ops > 0) || (!eps && !philox) || n_img < 1 || n_ops < 0 || n_targets < 0 || draw_base < 0) return SF_ERR_INVALID;
  if (n_targets > 0 && (!sel_nops || !out_states)) return SF_ERR_INVALID;
  if ((carry_in && (!state_in || !p_in)) || (carry_out && (!p_out || n_ops == 0))) return SF_ERR_INVALID;      // (no op: no infer_state to compute the carry beside)
  if (gru_c->C > 128 || (gru_c->C % 8)) return SF_ERR_UNSUPPORTED;
  if (solver != SF_SOLVER_EULER && solver != SF_SOLVER_MIDPOINT && solver != SF_SOLVER_RK4) return SF_ERR_INVALID;
  const int C = gru_c->C, B = n_img;
  const size_t PC = (size_t)B * H * W * C;
  const bool resumed = state_in || p_in || p_out;
  RolloutLayout L;
  if (!carve(L, ws, ws_bytes, C, B, (size_t)H * W)) return SF_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  SplitScope sp(L.split, st);
  SF_HIP(zero_fill(L.zeros, al(PC) * sizeof(float), st));
  if (!state_in) SF_HIP(zero_fill(L.sbuf[0], al(PC) * sizeof(float), st));   // state = zeros  (temporal_ode_bayes.py:507)
  if (!p_in) SF_HIP(zero_fill(L.pbuf[0], al(PC) * sizeof(float), st));       // input: overwritten by the first jump (:565,574)
  // the carried state / input are read where they lie (the first op writes L.sbuf[1] / L.pbuf[1]); nothing below writes through s_cur / p_cur
  const float* s_cur = state_in ? state_in : L.sbuf[0];
  const float* p_cur = p_in ? p_in : L.pbuf[0];
  int si = 0, pi = 0, draw = draw_base;
  const int cstride = coef_per_image ? SF_COEF_STRIDE : 0;
  const size_t step_stride = (size_t)SF_COEF_STRIDE * (coef_per_image ? B : 1);
  std::vector<Stage> stages;
  for (int i = 0; i < n_ops; ++i) {
    const int kind = ops[2 * i], arg = ops[2 * i + 1];
    // the imputed input this op leaves behind is only read by a following ODE step (:446-455); a jump ignores it
    // (:327-344) and then overwrites it (:574), and nothing reads it after the last op: those infer_state passes
    // are skipped (their noise draw keeps its index) — unless the caller takes it over as p_out
    const bool next_is_step = (i + 1 < n_ops) && ops[2 * (i + 1)] == SF_OP_STEP;
    const bool last = i + 1 == n_ops;
    const bool need_p = (impute && next_is_step) || (last && p_out);
    const float* s = s_cur; float* s2 = L.sbuf[si ^ 1];
    const float* p = p_cur; float* p2 = (last && p_out) ? p_out : L.pbuf[pi ^ 1];
    if (kind == SF_OP_JUMP) {   // :562-574
      // (the jump's imputed input replaces the current one in place; p_in itself is never written)
      float* pj = (last && p_out) ? p_out : L.pbuf[pi];
      if (!hx_obs) return SF_ERR_INVALID;      // (NULL is fine for a segment without jumps)
      stages.push_back({.w = gru_obs, .x = hx_obs + (size_t)arg * PC, .s = s, .out = s2, .derivative = 0, .infer_after = need_p, .draw = draw, .p_out = pj, .op_end = i});
      draw += 1;
      si ^= 1;
      s_cur = s2;
      if (need_p) p_cur = pj;
    } else if (kind == SF_OP_STEP) {
      if (!coef) return SF_ERR_INVALID;
      draw += step_stages(solver, gru_c, impute ? p : L.zeros, s, s2, p2, need_p, coef + (size_t)arg * step_stride, draw, i, L.sb, stages);
      si ^= 1;
      pi ^= 1;
      s_cur = s2;
      p_cur = p2;
    } else {
      return SF_ERR_INVALID;
    }
  }
  const unsigned* flow_err = nullptr;
  ResumeCarry rc;
  // The boundary of an IMPUTE rollout lies between an infer_state and the ODE cell that reads its sample: the unsplit rollout
  // computes branch 2 of that cell beside the infer_state (struct Carry), and the launch grouping decides the split-K summation
  // order — so a segment that hands p_out on computes the same side problems into carry_out, and the next one consumes them.
  // Without IMPUTE no cell follows an infer_state it depends on (a step reads zeros): nothing is carried.
  rc.in = impute ? carry_in : nullptr;
  rc.out = impute ? carry_out : nullptr;
  rc.next_w = gru_c;
  rc.draw0 = draw_base;
  rc.allow_flow = !resumed;      // a resumed segment always runs in the launch-per-layer form (sfnative.h)
  SF_TRY(run_stages(stages, *pm, eps, philox, cstride, sel_nops, n_targets, out_states, B, H, W, L, st, &flow_err, rc));
  if (final_state && final_state != s_cur) SF_HIP(copy_floats(s_cur, final_state, PC, st));
  if (p_out && n_ops == 0 && p_out != p_cur) SF_HIP(copy_floats(p_cur, p_out, PC, st));
  return flow_close(flow_err, out_states, (size_t)n_targets * PC, final_state, final_state ? PC : 0, st);
}
int sf_nnfo_rollout_fwd(const sf_dual_w* gru_c, const sf_dual_w* gru_obs, const sf_pmodel_w* pm, int solver, int impute,
                        const int32_t* ops, int n_ops, const float* hx_obs, const float* eps, const float* coef,
                        int coef_per_image, const int32_t* sel_nops, int n_targets, float* out_states,
                        float* final_state, int n_img, int H, int W, float* ws, size_t ws_bytes, void* stream) {
  if (!eps || !ops || !hx_obs || !sel_nops || !out_states) return SF_ERR_INVALID;
  return rollout_core(gru_c, gru_obs, pm, solver, impute, ops, n_ops, hx_obs, eps, nullptr, coef, coef_per_image, sel_nops, n_targets,
                      out_states, final_state, n_img, H, W, ws, ws_bytes, stream);
}
// resumable form: see sfnative.h.  eps holds the segment's own draws (draw k of the segment reads eps[k]); draw_base keys the Philox form
int sf_nnfo_rollout_resume_fwd(const sf_dual_w* gru_c, const sf_dual_w* gru_obs, const sf_pmodel_w* pm, int solver, int impute,
                               const int32_t* ops, int n_ops, const float* hx_obs, const float* eps, const float* coef,
                               int coef_per_image, const int32_t* sel_nops, int n_targets, float* out_states, float* final_state,
                               const float* state_in, const float* p_in, const float* carry_in, int draw_base, float* p_out,
                               float* carry_out, int n_img, int H, int W, float* ws, size_t ws_bytes, void* stream) {
  if (!eps) return SF_ERR_INVALID;
  return rollout_core(gru_c, gru_obs, pm, solver, impute, ops, n_ops, hx_obs, eps, nullptr, coef, coef_per_image, sel_nops, n_targets,
                      out_states, final_state, n_img, H, W, ws, ws_bytes, stream, {state_in, p_in, carry_in, draw_base, p_out, carry_out});
}
int sf_nnfo_rollout_resume_philox_fwd(const sf_dual_w* gru_c, const sf_dual_w* gru_obs, const sf_pmodel_w* pm, int solver, int impute,
                                      const int32_t* ops, int n_ops, const float* hx_obs, const uint64_t* philox_state, const float* coef,
                                      int coef_per_image, const int32_t* sel_nops, int n_targets, float* out_states, float* final_state,
                                      const float* state_in, const float* p_in, const float* carry_in, int draw_base, float* p_out,
                                      float* carry_out, int n_img, int H, int W, float* ws, size_t ws_bytes, void* stream) {
  if (!philox_state) return SF_ERR_INVALID;
  return rollout_core(gru_c, gru_obs, pm, solver, impute, ops, n_ops, hx_obs, nullptr, reinterpret_cast<const unsigned long long*>(philox_state),
                      coef, coef_per_image, sel_nops, n_targets, out_states, final_state, n_img, H, W, ws, ws_bytes, stream,
                      {state_in, p_in, carry_in, draw_base, p_out, carry_out});
}
// the same with the Gaussian noise of infer_state generated in the sampling epilogue (Philox4x32-10, csrc/sf_math.h)
int sf_nnfo_rollout_philox_fwd(const sf_dual_w* gru_c, const sf_dual_w* gru_obs, const sf_pmodel_w* pm, int solver, int impute,
                               const int32_t* ops, int n_ops, const float* hx_obs, const uint64_t* philox_state, const float* coef,
                               int coef_per_image, const int32_t* sel_nops, int n_targets, float* out_states, float* final_state,
                               int n_img, int H, int W, float* ws, size_t ws_bytes, void* stream) {
  if (!philox_state || !ops || !hx_obs || !sel_nops || !out_states) return SF_ERR_INVALID;
  return rollout_core(gru_c, gru_obs, pm, solver, impute, ops, n_ops, hx_obs, nullptr, reinterpret_cast<const unsigned long long*>(philox_state),
                      coef, coef_per_image, sel_nops, n_targets, out_states, final_state, n_img, H, W, ws, ws_bytes, stream);
}
int sf_infer_state_philox_fwd(const sf_pmodel_w* w, const float* s, const uint64_t* philox_state, int draw, float* p_out, float* q_out,
                              int n_img, int H, int W, float* ws, size_t ws_bytes, void* stream) {
  if (!w || !s || !philox_state || !p_out || w->C <= 0 || (w->C % 8) || n_img < 1 || draw < 0) return SF_ERR_INVALID;
  WithSplit<InferBufs> L;
  if (!carve(L, ws, ws_bytes, w->C, n_img, (size_t)H * W)) return SF_ERR_WORKSPACE;
  SplitScope sp(L.split, (hipStream_t)stream);
  return infer_state(*w, s, nullptr, p_out, q_out, n_img, H, W, L.bufs, (hipStream_t)stream, reinterpret_cast<const unsigned long long*>(philox_state), draw);
}

// ---- SmallEncoder / SmallDecoder ------------------------------------------------------------------
// level 0 at H x W: conv1's output, the projection, the block's output (max(C, F) channels each); level 1 at H/2 x W/2: the pooled
// input (F), t (F), pr and o (2F); level 2 at H/4 x W/4: the pooled input (2F), t, pr and three outputs (4F)
struct EncoderBufs {
  float *t0, *pr0, *o0, *q1, *t1, *pr1, *o1, *q2, *t2, *pr2, *o2, *o3, *o4;
  void take(Arena& A, int C, int F, int n, int H, int W) {
    const size_t P0 = (size_t)n * H * W, P1 = (size_t)n * (H / 2) * (W / 2), P2 = (size_t)n * (H / 2 / 2) * (W / 2 / 2);
    const int Cm = C > F ? C : F;
    t0 = A.take(P0 * Cm); pr0 = A.take(P0 * Cm); o0 = A.take(P0 * Cm);
    q1 = A.take(P1 * F); t1 = A.take(P1 * F); pr1 = A.take(P1 * 2 * F); o1 = A.take(P1 * 2 * F);
    q2 = A.take(P2 * 2 * F); t2 = A.take(P2 * 4 * F); pr2 = A.take(P2 * 4 * F);
    o2 = A.take(P2 * 4 * F); o3 = A.take(P2 * 4 * F); o4 = A.take(P2 * 4 * F);
  }
};
size_t sf_small_encoder_ws_bytes(int C, int F, int n, int H, int W) { return layout_bytes<EncoderBufs>(C, F, n, H, W); }
int sf_small_encoder_fwd(const sf_encoder_w* w, const float* x, float* out, int n, int H, int W, float* ws,
                         size_t ws_bytes, void* stream) {
  if (!w || !x || !out) return SF_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const int H1 = H / 2, W1 = W / 2, H2 = H1 / 2, W2 = W1 / 2;
  EncoderBufs b;
  if (!carve(b, ws, ws_bytes, w->C, w->F, n, H, W)) return SF_ERR_WORKSPACE;
  SF_TRY(res_block(w->blocks[0], x, b.o0, b.t0, b.pr0, n, H, W, 0, st, b.q1));        // res_models.py:101-105: block, MaxPool2d(2)
  SF_TRY(res_block(w->blocks[1], b.q1, b.o1, b.t1, b.pr1, n, H1, W1, 0, st, b.q2));
  SF_TRY(res_block(w->blocks[2], b.q2, b.o2, b.t2, b.pr2, n, H2, W2, 0, st));
  SF_TRY(res_block(w->blocks[3], b.o2, b.o3, b.t2, b.pr2, n, H2, W2, 0, st));
  SF_TRY(res_block(w->blocks[4], b.o3, b.o4, b.t2, b.pr2, n, H2, W2, 0, st));
  return run1(problem(w->last, b.o4, nullptr, out, n, H2, W2), EPI_AFFINE, st);   // :106 conv+BN+tanh
}

struct DecoderBufs {      // four tensors at h x w (4F channels), three at 2h x 2w (2F), four at 4h x 4w (max(F, C))
  float *a0, *a1, *a2, *a3, *b0, *b1, *b2, *c0, *c1, *c2, *c3;
  void take(Arena& A, int C, int F, size_t P) {
    const int Cm = F > C ? F : C;
    a0 = A.take(P * 4 * F); a1 = A.take(P * 4 * F); a2 = A.take(P * 4 * F); a3 = A.take(P * 4 * F);
    b0 = A.take(4 * P * 2 * F); b1 = A.take(4 * P * 2 * F); b2 = A.take(4 * P * 2 * F);
    c0 = A.take(16 * P * Cm); c1 = A.take(16 * P * Cm); c2 = A.take(16 * P * Cm); c3 = A.take(16 * P * Cm);
  }
};
size_t sf_small_decoder_ws_bytes(int C, int F, int n, int h, int w) { return layout_bytes<DecoderBufs>(C, F, (size_t)n * h * w); }
int sf_small_decoder_fwd(const sf_decoder_w* w, const float* z, float* out, int n, int h, int wd, float* ws,
                         size_t ws_bytes, void* stream) {
  if (!w || !z || !out) return SF_ERR_INVALID;
  const int F = w->F;
  hipStream_t st = (hipStream_t)stream;
  DecoderBufs b;
  if (!carve(b, ws, ws_bytes, w->C, F, (size_t)n * h * wd)) return SF_ERR_WORKSPACE;
  const auto [a0, a1, a2, a3, b0, b1, b2, c0, c1, c2, c3] = b;
  SF_TRY(run1(problem(w->first, z, nullptr, a0, n, h, wd), EPI_AFFINE, st));           // res_models.py:136
  SF_TRY(res_block(w->blocks[0], a0, a1, a2, a3, n, h, wd, 0, st));                     // 4F -> 2F
  SF_TRY(res_block(w->blocks[1], a1, a0, a2, a3, n, h, wd, 0, st));                     // 2F -> 2F
  SF_TRY(res_block(w->blocks[2], a0, a1, a2, a3, n, h, wd, 0, st));                     // 2F -> 2F
  // upsample(x2) is applied on read by block 3 (conv_1 and projection), :142-143
  SF_TRY(res_block(w->blocks[3], a1, b0, b1, b2, n, h, wd, 1, st));                     // 2F -> F @2h
  // block 4 (F -> F @4h) reads block 3's output upsampled: on read where its second convolution runs on the Winograd kernel (the
  // identity skip then comes from the half-size tensor too), from a materialised copy otherwise
  int rc = res_block(w->blocks[4], b0, c1, c2, c3, n, 2 * h, 2 * wd, 1, st);
  if (rc == SF_ERR_UNSUPPORTED) {
    SF_HIP(launch_upsample2(b0, c0, n, 2 * h, 2 * wd, F, st));
    rc = res_block(w->blocks[4], c0, c1, c2, c3, n, 4 * h, 4 * wd, 0, st);
  }
  SF_TRY(rc);
  SF_TRY(run1(problem(w->last0, c1, nullptr, c2, n, 4 * h, 4 * wd), EPI_AFFINE, st));
  return run1(problem(w->last1, c2, nullptr, out, n, 4 * h, 4 * wd), EPI_AFFINE, st);
}

// ---- Bottleneck / distribution heads (secondary, BEVerse-compatible classes) ------------------------
// the two hidden tensors (Cin / 2 channels), the pooled input and the projection: the last three at the input's size also where the
// block downsamples (the size query is not told)
struct BottleneckBufs {
  float *t1, *t2, *xp, *pr;
  void take(Arena& A, int Cin, int Cout, size_t P) { t1 = A.take(P * (Cin / 2)); t2 = A.take(P * (Cin / 2)); xp = A.take(P * Cin); pr = A.take(P * Cout); }
};
size_t sf_bottleneck_ws_bytes(int Cin, int Cout, int n, int H, int W) { return layout_bytes<BottleneckBufs>(Cin, Cout, (size_t)n * H * W); }
// Bottleneck.forward (streamingflow/layers/convolutions.py:65-172, beverse basic_modules.py:68-178):
// 1x1 -> BN,ReLU -> 3x3 (stride 2 if downsample) -> BN,ReLU -> 1x1 -> BN,ReLU, + skip (identity, or
// [zero-pad + 2x2 max-pool] + 1x1 + BN).  out: [n][Ho][Wo][Cout], Ho = ceil(H/2) when downsampling.
int sf_bottleneck_fwd(const sf_bottleneck_w* w, const float* x, float* out, int n, int H, int W, float* ws,
                      size_t ws_bytes, void* stream) {
  if (!w || !x || !out || !valid_w(w->down) || !valid_w(w->conv) || !valid_w(w->up)) return SF_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const int Cin = w->down.c0, Cm = w->down.cout, Cout = w->up.cout;
  const int Ho = w->downsample ? (H + 1) / 2 : H, Wo = w->downsample ? (W + 1) / 2 : W;
  if (Cm > Cin / 2 || w->conv.cout > Cin / 2 || (w->proj.w && w->proj.cout != Cout)) return SF_ERR_INVALID;
  BottleneckBufs b;
  if (!carve(b, ws, ws_bytes, Cin, Cout, (size_t)n * H * W)) return SF_ERR_WORKSPACE;
  const auto [t1, t2, xp, pr] = b;
  SF_TRY(run1(problem(w->down, x, nullptr, t1, n, H, W), EPI_AFFINE, st));
  ConvProblem c = problem(w->conv, t1, nullptr, t2, n, H, W);
  if (c.Hout != Ho || c.Wout != Wo) return SF_ERR_INVALID;
  SF_TRY(run1(c, EPI_AFFINE, st));
  ConvProblem u = problem(w->up, t2, nullptr, out, n, Ho, Wo);
  if (w->proj.w) {
    const float* src = x;
    if (w->downsample) {
      SF_HIP(launch_maxpool2(x, xp, n, H, W, Cin, 1, st));
      src = xp;
    }
    SF_TRY(run1(problem(w->proj, src, nullptr, pr, n, Ho, Wo), EPI_AFFINE, st));
    u.add = pr;
  } else {
    if (w->downsample || Cin != Cout) return SF_ERR_INVALID;
    u.add = x;
  }
  return run1(u, EPI_AFFINE, st);
}

// 1x1 head of the (Spatial)DistributionModule (beverse motion_modules.py:34-46, 74-88): optional
// global average pool, 1x1 conv with bias, log-sigma half clamped to [lo, hi] when clamp != 0.
// the pooled form's slab sums and mean: carved also without global_pool (the size query is not told)
struct DistHeadBufs { float *part, *mean; void take(Arena& A, int C, int n) { part = A.take((size_t)n * 64 * C); mean = A.take((size_t)n * C); } };
size_t sf_dist_head_ws_bytes(int C, int n) { return layout_bytes<DistHeadBufs>(C, n); }
int sf_dist_head_fwd(const sf_conv_w* w, const float* enc, float* out, int n, int H, int W, int global_pool, int clamp,
                     float lo, float hi, float* ws, size_t ws_bytes, void* stream) {
  if (!w || !enc || !out || !valid_w(*w)) return SF_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const int C = w->c0;
  const float* src = enc;
  int Hh = H, Wh = W;
  DistHeadBufs b;
  if (!carve(b, ws, ws_bytes, C, n)) return SF_ERR_WORKSPACE;
  if (global_pool) {
    SF_HIP(launch_chan_partial(enc, b.part, n, H * W, C, 64, st));
    SF_HIP(launch_mean_from_partials(b.part, b.mean, n, 64, C, H * W, st));
    src = b.mean; Hh = 1; Wh = 1;
  }
  ConvProblem p = problem(*w, src, nullptr, out, n, Hh, Wh);
  if (clamp) { p.clamp_from = w->cout / 2; p.clamp_lo = lo; p.clamp_hi = hi; }
  return run1(p, EPI_AFFINE, st);
}

// ---- head blocks ----------------------------------------------------------------------------------
// the depthwise + LayerNorm output and the hidden tensor
struct ConvNextBufs { float *t, *u; void take(Arena& A, int C, size_t P) { t = A.take(P * C); u = A.take(P * 4 * C); } };
size_t sf_convnext_block_ws_bytes(int C, int n, int H, int W) { return layout_bytes<ConvNextBufs>(C, (size_t)n * H * W); }
int sf_convnext_block_fwd(const sf_convnext_w* w, const float* x, float* out, int n, int H, int W, float* ws,
                          size_t ws_bytes, void* stream) {
  if (!w || !x || !out) return SF_ERR_INVALID;
  const int C = w->C;
  hipStream_t st = (hipStream_t)stream;
  const size_t P = (size_t)n * H * W;
  ConvNextBufs bufs;
  if (!carve(bufs, ws, ws_bytes, C, P)) return SF_ERR_WORKSPACE;
  float *t = bufs.t, *u = bufs.u;
  if (launch_dwconv7_ln(x, t, w->dw_w, w->dw_b, w->ln_w, w->ln_b, n, H, W, C, 1e-6f, st) != hipSuccess)
    return SF_ERR_UNSUPPORTED;
  // 64 -> 256 -> 64 (every ConvNeXt block of the reference's configs): the two pointwise layers in one launch, the hidden tensor
  // never written (convnext_mlp.hip).  Exact fp32 only: the bf16x3 mode keeps its own K loop on the two-launch path
  const sf_conv_w &a = w->pw1, &b = w->pw2;
  const bool one_by_one = a.kh == 1 && a.kw == 1 && b.kh == 1 && b.kw == 1 && a.stride == 1 && b.stride == 1 && a.pad == 0 && b.pad == 0;
  if (one_by_one && C == 64 && a.c0 == 64 && a.c1 == 0 && a.cin_pad == 64 && a.cout == 256 && a.cout_pad == 256 && a.act == ACT_GELU &&
      b.c0 == 256 && b.c1 == 0 && b.cin_pad == 256 && b.cout == 64 && b.cout_pad == 64 && b.act == ACT_NONE && a.w && b.w &&
      !(a.w_bf16x3 && b.w_bf16x3)) {
    SF_TRY(seg_flush());
    auto cost = [&] {      // t and x once, out once, both weight matrices once
      return Cost{20 * 8 + EPI_AFFINE, 2.0 * (double)P * (64.0 * 256.0 + 256.0 * 64.0), 4.0 * ((double)P * 64.0 * 3.0 + 2.0 * 64.0 * 256.0)};
    };
    SF_HIP(timed([&] { return launch_convnext_mlp(t, x, out, a.w, a.scale, a.bias, b.w, b.scale, b.bias, (long)P, st); }, cost, st));
    return SF_OK;
  }
  SF_TRY(run1(problem(w->pw1, t, nullptr, u, n, H, W), EPI_AFFINE, st));
  ConvProblem p2 = problem(w->pw2, u, nullptr, out, n, H, W);
  p2.add = x;
  return run1(p2, EPI_AFFINE, st);
}

struct DeepLabBufs {      // the four branches side by side, projection and 3x3 output, the pooling branch's slab sums and per-image bias
  float *cat, *y, *z, *part, *bimg;
  void take(Arena& A, int C, int hid, int n, size_t P) {
    cat = A.take(P * 4 * hid); y = A.take(P * hid); z = A.take(P * hid);
    part = A.take((size_t)n * ASPP_SLABS * C); bimg = A.take((size_t)n * hid);
  }
};
size_t sf_deeplab_head_ws_bytes(int C, int hid, int n, int H, int W) { return layout_bytes<DeepLabBufs>(C, hid, n, (size_t)n * H * W); }
static int deeplab_head(const sf_deeplab_w* w, const float* x, float* out, int n, int H, int W, int planar_group, size_t stride_major,
                        size_t stride_minor, float* ws, size_t ws_bytes, void* stream) {
  if (!w || !x || !out) return SF_ERR_INVALID;
  const int C = w->C, hid = w->hid;
  hipStream_t st = (hipStream_t)stream;
  const size_t P = (size_t)n * H * W;
  DeepLabBufs b;
  if (!carve(b, ws, ws_bytes, C, hid, n, P)) return SF_ERR_WORKSPACE;
  const auto [cat, y, z, part, bimg] = b;
  SF_HIP(launch_aspp_pool(x, part, bimg, n, H * W, C, hid, w->pool_w, w->pool_scale, w->pool_bias, w->proj_pool_w,
                          w->project.scale, w->project.bias, ASPP_SLABS, st));
  ConvProblem ps[4];
  for (int i = 0; i < 4; ++i) {   // convolutions.py:265-269
    ps[i] = problem(w->branch[i], x, nullptr, cat, n, H, W);
    ps[i].out_cs = 4 * hid; ps[i].out_co = i * hid;
  }
  ConvProblem pj = problem(w->project, cat, nullptr, y, n, H, W);
  pj.bias = bimg; pj.bias_per_img = 1;
  // The 1x1 branch's slice of `cat` is read by the projection alone: where the projection runs on the 128 x 128 LDS-DMA tile in exact fp32
  // with one cout tile, its workgroups compute that slice for their own pixels (conv_igemm.hip: the producer form) and neither the branch's
  // launch nor the slice's trip through memory happens (slice 0 of `cat` stays unwritten and unread).  Same chunk and k order in both GEMMs:
  // bitwise the two launches' result.  SF_GLDS bit 4 (live) = 0 restores the two launches; bit 5 is a test's: the branch and the projection on
  // that tile at any pixel count, so that both forms meet on a few tiles
  const int live = glds_live();
  const sf_conv_w& b0 = w->branch[0];
  const bool forced = (live & 32) && hid % 128 == 0 && b0.kh == 1 && b0.kw == 1 && b0.stride == 1 && b0.pad == 0;
  const bool on_tile = forced || plans_dma128(pj, EPI_AFFINE);
  const bool fused = (live & 16) && on_tile && hid == 128 && pj.cout_pad == 128 && pj.c0 == 4 * hid && pj.cin_pad == 4 * hid && !pj.w3 && pj.w &&
                     C % 32 == 0 && b0.c0 == C && b0.c1 == 0 && b0.cin_pad == C && b0.cout == hid && b0.cout_pad == hid && b0.kh == 1 && b0.kw == 1 &&
                     b0.stride == 1 && b0.pad == 0 && b0.act == ACT_RELU && b0.w && b0.scale && b0.bias && !b0.w_bf16x3;
  if (fused) {
    SF_TRY(run(ps + 1, 3, EPI_AFFINE, st));
    pj.e0 = x; pj.e0_cs = C;
    pj.fuse_w = b0.w; pj.fuse_scale = b0.scale; pj.fuse_bias = b0.bias;
    pj.fuse_cout = hid; pj.fuse_cout_pad = b0.cout_pad; pj.fuse_kpad = b0.cin_pad;
    SF_TRY(run_dma128(pj, true, st));
  } else if (forced) {
    SF_TRY(run_dma128(ps[0], false, st));
    SF_TRY(run(ps + 1, 3, EPI_AFFINE, st));
    SF_TRY(run_dma128(pj, false, st));
  } else {
    SF_TRY(run(ps, 4, EPI_AFFINE, st));
    SF_TRY(run1(pj, EPI_AFFINE, st));
  }
  SF_TRY(run1(problem(w->conv3, y, nullptr, z, n, H, W), EPI_AFFINE, st));
  ConvProblem pc = problem(w->cls, z, nullptr, out, n, H, W);
  if (planar_group > 0) { pc.out_planar = 1; pc.pl_div = planar_group; pc.pl_sa = stride_major; pc.pl_sb = stride_minor; }
  return run1(pc, EPI_AFFINE, st);
}
int sf_deeplab_head_fwd(const sf_deeplab_w* w, const float* x, float* out, int n, int H, int W, float* ws,
                        size_t ws_bytes, void* stream) {
  return deeplab_head(w, x, out, n, H, W, 0, 0, 0, ws, ws_bytes, stream);
}
// the same with the classifier writing the boundary layout itself: image i as [cout][H][W] planes at
// out + (i / group) * stride_major + (i % group) * stride_minor floats (frames (t, b) of a [T][B] run into a [B][T][C][H][W] tensor:
// group = B, stride_major = C*H*W, stride_minor = T*C*H*W) — no transpose launches after the head (future_prediction_ode.py:62-64)
int sf_deeplab_head_planar_fwd(const sf_deeplab_w* w, const float* x, float* out, int n, int H, int W, int group, size_t stride_major,
                               size_t stride_minor, float* ws, size_t ws_bytes, void* stream) {
  if (group < 1 || !w || stride_major < (size_t)w->cls.cout * H * W || stride_minor < (size_t)w->cls.cout * H * W) return SF_ERR_INVALID;
  return deeplab_head(w, x, out, n, H, W, group, stride_major, stride_minor, ws, ws_bytes, stream);
}

// ---- graphs / events ------------------------------------------------------------------------------
int sf_graph_begin(void* stream) {
  SF_HIP(hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeThreadLocal));
  return SF_OK;
}
int sf_graph_end(void* stream, void** exec_out) {
  if (!exec_out) return SF_ERR_INVALID;
  hipGraph_t g = nullptr;
  SF_HIP(hipStreamEndCapture((hipStream_t)stream, &g));
  hipGraphExec_t e = nullptr;
  hipError_t r = hipGraphInstantiate(&e, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (r != hipSuccess) return SF_ERR_LAUNCH;
  *exec_out = (void*)e;
  return SF_OK;
}
int sf_graph_launch(void* exec, void* stream) {
  SF_HIP(hipGraphLaunch((hipGraphExec_t)exec, (hipStream_t)stream));
  return SF_OK;
}
int sf_graph_destroy(void* exec) {
  SF_HIP(hipGraphExecDestroy((hipGraphExec_t)exec));
  return SF_OK;
}

/* Diagnostic builds (-DSF_STAMP) only: `buf` = 64 slots x 4096 workgroups x 8 uint64 device buffer (NULL switches the
 * stamps off); conv launches then record in-kernel s_memrealtime stamps into consecutive slots.  SF_ERR_UNSUPPORTED
 * in the product build. */
int sf_set_flow_mode(int on) { return set_flow_mode(on); }
// number of timed-out dependency waits of the calling thread's most recent persistent-flow rollout (0 = healthy; > 0: its outputs were
// overwritten with NaN).  Synchronises `stream`.  SF_ERR_INVALID: this thread has not run one.
int sf_flow_errors(void* stream) { return flow_errors((hipStream_t)stream); }

int sf_debug_stamps(void* buf) { return debug_stamps(buf); }

/* diagnostic: workgroups per CU of the large LDS-DMA tiles (0: 128x128 fp32, 1: 128x128 bf16x3, 2: 64x128 fp32, 3: 64x128 bf16x3) */
int sf_debug_occupancy(int which) { return glds_occupancy(which); }
/* diagnostic, host only: the Winograd plan of a launch (dispatch.hip: debug_wino_plan) */
int sf_debug_wino_plan(const sf_conv_w* w, int epi, int n_img, int Hin, int Win, int in_up, int nprob, int flags, int32_t* out, int n_out) {
  if (!w || !valid_w(*w)) return SF_ERR_INVALID;
  return debug_wino_plan(*w, epi, n_img, Hin, Win, in_up, nprob, flags, out, n_out);
}
/* diagnostic, host only: the plan of the tiled kernels for a launch group (dispatch.hip: debug_tiled_plan) */
int sf_debug_tiled_plan(const sf_conv_w* w, int epi, int n_img, int Hin, int Win, int in_up, int nprob, int flags, int32_t* out, int n_out) {
  if (!w || nprob < 1 || nprob > SF_MAX_GROUP) return SF_ERR_INVALID;
  for (int i = 0; i < nprob; ++i)
    if (!valid_w(w[i])) return SF_ERR_INVALID;
  return debug_tiled_plan(w, epi, n_img, Hin, Win, in_up, nprob, flags, out, n_out);
}

int sf_prof_enable(int on) {
  prof_enable(on != 0);
  return SF_OK;
}
// Aggregates (and clears) the recorded launches by kernel key (dispatch.hip: prof_collect).  Synchronises.
int sf_prof_collect(int32_t* calls, double* ms, double* flops, double* bytes) {
  if (!calls || !ms || !flops || !bytes) return SF_ERR_INVALID;
  return prof_collect(calls, ms, flops, bytes);
}

int sf_event_create(void** ev) {
  hipEvent_t e;
  SF_HIP(hipEventCreate(&e));
  *ev = (void*)e;
  return SF_OK;
}
int sf_event_record(void* ev, void* stream) { SF_HIP(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream)); return SF_OK; }
int sf_event_elapsed_ms(void* a, void* b, float* ms) {
  SF_HIP(hipEventSynchronize((hipEvent_t)b));
  SF_HIP(hipEventElapsedTime(ms, (hipEvent_t)a, (hipEvent_t)b));
  return SF_OK;
}
int sf_event_destroy(void* ev) { SF_HIP(hipEventDestroy((hipEvent_t)ev)); return SF_OK; }

}  // extern "C"
