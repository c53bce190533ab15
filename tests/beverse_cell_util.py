"""TEST INFRASTRUCTURE — the BEVerse conv-GRU cells (streamingflow_amd/beverse/basic_modules.py: ``GRUCell``, ``SpatialGRU`` without
decoder) at every kernel family their dispatch reaches: the case table, the builders and the float64 reference.

A case: name, kind (cell | spatial_gru), Cx = input_size, C = hidden_size, n images of h x w, T frames (spatial_gru), gru_bias_init,
family = the regime of FAMILIES the case exists for, given = whether a SpatialGRU gets a state (else ``state=None``), seed, gain.
The module is filled with ``hashfill.fill_state_dict(..., seed, gain)`` (running variances U(.5, 1.5): positive), the inputs are
``hashfill.normal``.  ``reference(case)`` is the same module cast to float64 and run through ``gru_cell_torch`` / ``spatial_gru_torch``
on the CPU; ``reference32(case)`` the same in float32.  Nothing here needs a GPU.

The tolerance is measured, not chosen: ``python tests/beverse_cell_util.py`` prints, per case, e32 = max |reference32 - reference|
— what float32 accumulation of the same cell costs in the reference's own arithmetic.  Direct-form families pass within
TOL_DIRECT = 8 x max(e32) (another summation order over up to 9 (Cx + C) products, then the epilogue's sigmoid and blend), Winograd
families get the project's Winograd-against-direct bar of 2e-5 on top (TOL_WINO); neither may exceed 1e-4, the bar test_gru_cell_gpu
holds for one cell.

Measured e32 (torch CPU, 8 threads, float32 against float64):
  sp_3img 1.286e-06, sp_odd_side 1.132e-06, sp_wino 1.014e-06, sp_wino_head 1.351e-06, direct_48_32 8.450e-07, direct_24_16 1.333e-06,
  staged16_12_8 4.941e-07, dma32 1.182e-06, direct_mid 1.516e-06, dma64 1.340e-06, staged64_48_32 1.121e-06, staged64_80_64 1.462e-06,
  wino_rows_over_4 1.269e-06, wino_3img 1.932e-06, wino_refused_w30 1.469e-06, gru_16_32_none 1.177e-06, gru_16_32_state 1.042e-06,
  gru_32_32_none 1.073e-06, gru_32_32_state 1.295e-06, gru_large_none 1.172e-06, gru_large_state 1.429e-06
max e32 = 1.932e-06  ->  TOL_DIRECT = 1.546e-05, TOL_WINO = 3.546e-05 (the E32 dict below is the same table; the plan test holds the two
equal).  On the MI355X the cells land at 2.9e-07 .. 6.3e-06 from the float64 reference, the Winograd forms at 1.0e-06 .. 3.2e-06.

WRONG names the deliberately wrong float64 cells of the sensitivity check (tests/test_beverse_cell_plan.py): each must move a case's
output by at least 100 x its tolerance, or the case's inputs could not tell a right kernel from a wrong one."""
import functools
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from workloads import hashfill  # noqa: E402

SP_MAX_P, LARGE_P, WINO_MIN_P = 4096, 8192, 14000      # csrc/dispatch.h: SP_MAX_P, LARGE_P, the default of SF_WINO_MIN_P

# family -> (what runs, the tile-table rows (csrc/sf_launch.h: TileId) of the gates and the candidate launch or None for the small-P /
# Winograd kernels, whether a Winograd form runs)
FAMILIES = {
    "sp_pregated": ("small-P kernel, direct form, gates write (1 - r) * s as a second output", None, False),
    "sp_wino": ("small-P kernel, Winograd form, pre-gated state", None, True),
    "direct_gate": ("direct-fragment kernel, reset gate applied while staging, P < 4096", ("TILE_DIRECT16", "TILE_DIRECT16"), False),
    "staged16_gate": ("staged 16x64 tile, reset gate applied while staging", ("TILE_S16x64K4", "TILE_S16x64K4"), False),
    "dma32": ("LDS-DMA 32x32 tiles, pre-gated state", ("TILE_DMA32x32", "TILE_DMA32x32"), False),
    "direct_gate_mid": ("direct-fragment kernel, reset gate applied while staging, 4096 <= P < 8192", ("TILE_DIRECT16", "TILE_DIRECT16"), False),
    "dma64": ("LDS-DMA 64x64 tiles, pre-gated state", ("TILE_DMA64x64", "TILE_DMA64x64"), False),
    "dma64_narrow": ("LDS-DMA tiles, pre-gated state, a candidate of 32 output channels on the narrow 32x128 tile", ("TILE_DMA64x64", "TILE_DMA32x128"), False),
    "staged64_gate": ("staged 64x64 tile, reset gate applied while staging", ("TILE_L64x64", "TILE_L64x64"), False),
    "wino": ("batched Winograd kernel: AFFINE + second output, then BLEND", None, True),
    "wino_refused": ("Winograd size, geometry refused (W < 32): LDS-DMA 64x64 tiles, pre-gated state", ("TILE_DMA64x64", "TILE_DMA64x64"), False),
}


def _case(name, kind, Cx, C, n, h, w, family, T=1, bias=0.0, given=True, seed=2, gain=1.0):
    return dict(name=name, kind=kind, Cx=Cx, C=C, n=n, h=h, w=w, T=T, gru_bias_init=bias, family=family, given=given, seed=seed, gain=gain)


CASES = [
    _case("sp_3img", "cell", 96, 64, 3, 13, 21, "sp_pregated", bias=0.3),
    _case("sp_odd_side", "cell", 96, 64, 1, 31, 34, "sp_pregated"),
    _case("sp_wino", "cell", 96, 64, 1, 30, 34, "sp_wino", bias=-0.2),
    _case("sp_wino_head", "cell", 288, 256, 1, 16, 18, "sp_wino"),
    _case("direct_48_32", "cell", 48, 32, 2, 11, 9, "direct_gate"),
    _case("direct_24_16", "cell", 24, 16, 1, 9, 7, "direct_gate", bias=0.3),
    _case("staged16_12_8", "cell", 12, 8, 1, 9, 7, "staged16_gate", bias=-0.2),
    _case("dma32", "cell", 96, 64, 1, 70, 66, "dma32"),
    _case("direct_mid", "cell", 48, 32, 1, 70, 66, "direct_gate_mid", bias=0.3),
    _case("dma64", "cell", 96, 64, 2, 66, 64, "dma64", bias=-0.2),
    _case("staged64_48_32", "cell", 48, 32, 2, 66, 64, "staged64_gate"),
    _case("staged64_80_64", "cell", 80, 64, 2, 66, 64, "staged64_gate", bias=0.3),      # % 16 but not % 32: no Winograd either
    _case("wino_rows_over_4", "cell", 96, 64, 1, 100, 142, "wino"),                   # 50 tile rows: two over a multiple of four
    _case("wino_3img", "cell", 96, 64, 3, 70, 68, "wino", bias=0.3),
    _case("wino_refused_w30", "cell", 96, 64, 8, 64, 30, "wino_refused"),
    _case("gru_16_32_none", "spatial_gru", 16, 32, 2, 13, 21, "direct_gate", T=3, given=False),
    _case("gru_16_32_state", "spatial_gru", 16, 32, 2, 13, 21, "direct_gate", T=3, bias=0.3),
    _case("gru_32_32_none", "spatial_gru", 32, 32, 1, 30, 34, "sp_wino", T=3, given=False, bias=-0.2),
    _case("gru_32_32_state", "spatial_gru", 32, 32, 1, 30, 34, "sp_wino", T=3),
    _case("gru_large_none", "spatial_gru", 32, 32, 1, 92, 90, "dma64_narrow", T=2, given=False),
    _case("gru_large_state", "spatial_gru", 32, 32, 1, 92, 90, "dma64_narrow", T=2, bias=0.3),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# ---- the measured tolerance (see the module docstring; `python tests/beverse_cell_util.py` prints this table) ----------------------
E32 = {
    "sp_3img": 1.286e-06,
    "sp_odd_side": 1.132e-06,
    "sp_wino": 1.014e-06,
    "sp_wino_head": 1.351e-06,
    "direct_48_32": 8.450e-07,
    "direct_24_16": 1.333e-06,
    "staged16_12_8": 4.941e-07,
    "dma32": 1.182e-06,
    "direct_mid": 1.516e-06,
    "dma64": 1.340e-06,
    "staged64_48_32": 1.121e-06,
    "staged64_80_64": 1.462e-06,
    "wino_rows_over_4": 1.269e-06,
    "wino_3img": 1.932e-06,
    "wino_refused_w30": 1.469e-06,
    "gru_16_32_none": 1.177e-06,
    "gru_16_32_state": 1.042e-06,
    "gru_32_32_none": 1.073e-06,
    "gru_32_32_state": 1.295e-06,
    "gru_large_none": 1.172e-06,
    "gru_large_state": 1.429e-06,
}
E32_MAX = max(E32.values()) if E32 else float("nan")
TOL_DIRECT = 8 * E32_MAX
TOL_WINO = TOL_DIRECT + 2e-5
TOL_CAP = 1e-4


def tolerance(case):
    return TOL_WINO if FAMILIES[case["family"]][2] else TOL_DIRECT


# ---- what the dispatch decides for a case's two launches (host arithmetic, no GPU) -----------------------------------------------------
EPI_AFFINE, EPI_BLEND = 0, 1


def pixels(case):
    return case["n"] * case["h"] * case["w"]


def pregated(case):
    """dispatch.hip: pregate under the shipped switches — the gates launch writes (1 - r) * s as a second output and the candidate reads
    cat[x, that] as a plain layer; otherwise the candidate launch applies the reset gate while staging."""
    return case["Cx"] % 32 == 0 and case["C"] % 32 == 0


def sp_wino_shape(case, cout):
    """the shape rules of the small-P kernel's Winograd form for a layer of `cout` outputs (dispatch.hip: sp_wino_ok)"""
    return (case["n"] == 1 and case["h"] % 2 == 0 and case["w"] % 2 == 0 and case["h"] >= 4 and case["w"] >= 4 and case["Cx"] % 32 == 0 and
            case["C"] % 32 == 0 and ((cout + 15) // 16 * 16) % 64 == 0)


def planned(case):
    """dict(gates, cand = util.tiled_plan of the launch with the flags gru_cell sets; wino_gates, wino_cand = util.wino_plan of it;
    names = the profiler's kernel names the cell must run on, or None where the Winograd kernel's form decides them)"""
    from streamingflow_amd import _lib
    from util import tiled_plan, wino_plan
    Cx, C, n, h, w = (case[k] for k in ("Cx", "C", "n", "h", "w"))
    pre = pregated(case)
    lay = lambda cout: [dict(c0=Cx, c1=C, cout=cout, k=3, wino=True)]      # (packed with Winograd weights, as the shipped default packs them)
    p = dict(gates=tiled_plan(lay(2 * C), n, h, w, epi=EPI_AFFINE, flags=0),      # (a second output does not enter the tiled / small-P plan)
             cand=tiled_plan(lay(C), n, h, w, epi=EPI_BLEND, flags=0 if pre else 2),
             wino_gates=wino_plan(Cx, C, 2 * C, n, h, w, epi=EPI_AFFINE, flags=4 if pre else 0),
             wino_cand=wino_plan(Cx, C, C, n, h, w, epi=EPI_BLEND))
    fam = (p["gates"]["family"], p["cand"]["family"])
    key = lambda q: 14 if q["family"] == 2 else q["key"]      # (_lib.KEY_NAMES: 14 is the small-P kernel)
    p["names"] = None if 1 in fam else {_lib.KERNEL_NAMES[key(p["gates"]) * 8 + EPI_AFFINE], _lib.KERNEL_NAMES[key(p["cand"]) * 8 + EPI_BLEND]}
    return p


def kernel_prefix(case):
    """the family prefix of the profiler's kernel names for the case"""
    fam = case["family"]
    return "conv_sp<" if fam.startswith("sp_") else "conv_wino<" if fam == "wino" else "conv_glds<" if fam.startswith(("dma", "wino_refused")) else "conv_igemm<"


# ---- builders ------------------------------------------------------------------------------------------------------------------------
def build(case, dtype=torch.float32):
    """The product module of the case on the CPU, hashed parameters (as tools/gen_resfuture_golden.py: build), eval mode."""
    from streamingflow_amd.beverse import basic_modules as B
    cls = B.GRUCell if case["kind"] == "cell" else B.SpatialGRU
    net = cls(case["Cx"], case["C"], gru_bias_init=case["gru_bias_init"])
    net.load_state_dict(hashfill.fill_state_dict(net.state_dict(), seed=case["seed"], gain=case["gain"]))
    return net.eval().to(dtype)


def inputs(case, dtype=torch.float32):
    """cell: (x (n, Cx, h, w), state (n, C, h, w)); spatial_gru: (x (n, T, Cx, h, w), state (n, C, h, w) or None).  CPU."""
    n, h, w, T = case["n"], case["h"], case["w"], case["T"]
    tag = "bvc_%s_" % case["name"]
    s = hashfill.normal(tag + "s", (n, case["C"], h, w), case["seed"] + 41).to(dtype) if case["given"] else None
    if case["kind"] == "cell":
        return hashfill.normal(tag + "x", (n, case["Cx"], h, w), case["seed"] + 40).to(dtype), s
    return hashfill.normal(tag + "x", (n, T, case["Cx"], h, w), case["seed"] + 40).to(dtype), s


def _forward_torch(case, dtype):
    from streamingflow_amd.beverse import basic_modules as B
    net = build(case, dtype)
    x, s = inputs(case, dtype)
    with torch.no_grad():
        return B.gru_cell_torch(net, x, s) if case["kind"] == "cell" else B.spatial_gru_torch(net, x, s)


@functools.lru_cache(maxsize=None)
def _reference(name):
    return _forward_torch(BY_NAME[name], torch.float64)


def reference(case):
    """float64, CPU: cell (n, C, h, w); spatial_gru (n, T, C, h, w).  Built once per case; do not modify."""
    return _reference(case["name"])


@functools.lru_cache(maxsize=None)
def _reference32(name):
    return _forward_torch(BY_NAME[name], torch.float32)


def reference32(case):
    return _reference32(case["name"])


# ---- the cell once more, step by step, with its gates exposed and with deliberate mistakes ---------------------------------------------
WRONG = ("r_not_one_minus_r", "update_reset_swapped", "bias_dropped", "x_state_exchanged")


def _cell(net, x, s, wrong, pre=None):
    """One float64 step on the parameters of `net`: (new state, update gate, reset gate, gate pre-activations without gru_bias_init).
    wrong: None or one of WRONG.  pre: the pre-activations of an earlier call on the same (x, s)."""
    from streamingflow_amd.beverse.basic_modules import conv_block_torch
    if pre is None:
        xs = torch.cat([x, s], dim=1)
        pre = (F.conv2d(xs, net.conv_update.weight, net.conv_update.bias, padding=1),
               F.conv2d(xs, net.conv_reset.weight, net.conv_reset.bias, padding=1))
    zu, zr = (pre[1], pre[0]) if wrong == "update_reset_swapped" else pre
    g = 0.0 if wrong == "bias_dropped" else net.gru_bias_init
    u, r = torch.sigmoid(zu + g), torch.sigmoid(zr + g)
    gated = (r if wrong == "r_not_one_minus_r" else 1.0 - r) * s
    cat = torch.cat([gated, x] if wrong == "x_state_exchanged" else [x, gated], dim=1)
    return (1.0 - u) * s + u * conv_block_torch(net.conv_state_tilde, cat), u, r, pre


@functools.lru_cache(maxsize=None)
def _trace(name):
    """The right cell through _cell: (output as reference(), update gates, reset gates, first step's pre-activations)."""
    case = BY_NAME[name]
    net = build(case, torch.float64)
    x, s = inputs(case, torch.float64)
    with torch.no_grad():
        if case["kind"] == "cell":
            y, u, r, pre = _cell(net, x, s, None)
            return y, u, r, pre
        s = torch.zeros((case["n"], case["C"], case["h"], case["w"]), dtype=torch.float64) if s is None else s
        outs, us, rs, pre0 = [], [], [], None
        for t in range(case["T"]):
            s, u, r, pre = _cell(net, x[:, t], s, None)
            pre0 = pre if pre0 is None else pre0
            outs.append(s); us.append(u); rs.append(r)
        return torch.stack(outs, 1), torch.stack(us, 1), torch.stack(rs, 1), pre0


def gates(case):
    """(update gates, reset gates) of the float64 reference, every step."""
    return _trace(case["name"])[1:3]


def traced_reference(case):
    """reference(case) as _cell computes it (the plan test holds the two equal: the wrong variants differ from the reference by their mistake alone)"""
    return _trace(case["name"])[0]


def wrong_reference(case, wrong):
    """float64 output of the case with the mistake `wrong` in every step."""
    assert wrong in WRONG
    net = build(case, torch.float64)
    x, s = inputs(case, torch.float64)
    pre0 = _trace(case["name"])[3]      # the first step sees the right inputs: its gate convolutions are the reference's
    with torch.no_grad():
        if case["kind"] == "cell":
            return _cell(net, x, s, wrong, pre0)[0]
        s = torch.zeros((case["n"], case["C"], case["h"], case["w"]), dtype=torch.float64) if s is None else s
        outs = []
        for t in range(case["T"]):
            s = _cell(net, x[:, t], s, wrong, pre0 if t == 0 else None)[0]
            outs.append(s)
        return torch.stack(outs, 1)


# ---- whole rollouts at the kernel families of the benchmarked size (tests/test_gpu_beverse_cells.py) ------------------------------------
# prefix: the kernel family the rollout's first cell — GRUCell(C + L, C), the asymmetric one — must be seen on
ROLLOUTS = [
    dict(name="v2_wino", cls="ResFuturePredictionV2", C=64, L=32, kw=dict(n_future=2), n=1, h=100, w=142, seed=2, gain=1.0, prefix="conv_wino<"),
    dict(name="res_direct_mid", cls="ResFuturePrediction", C=32, L=16, kw=dict(n_future=2), n=1, h=70, w=66, seed=2, gain=1.0, prefix="conv_igemm<direct16px"),
    dict(name="v1_each_sp", cls="ResFuturePredictionV1", C=64, L=32, kw=dict(n_future=2, n_gru_blocks=2, prob_each_future=True), n=1, h=30, w=34,
         seed=2, gain=1.0, prefix="conv_sp<"),
]


def build_rollout(r):
    """the module on the CPU, float32, hashed parameters (as tools/gen_resfuture_golden.py: build), eval mode"""
    from streamingflow_amd.beverse import motion_modules as M
    net = getattr(M, r["cls"])(r["C"], r["L"], **r["kw"])
    net.load_state_dict(hashfill.fill_state_dict(net.state_dict(), seed=r["seed"], gain=r["gain"]))
    return net.eval()


def rollout_inputs(r):
    """(sample (n, L [x n_future], h, w), hidden state (n, C, h, w)), CPU"""
    k = r["kw"]["n_future"] if r["kw"].get("prob_each_future") else 1
    tag = "bvr_%s_" % r["name"]
    return (hashfill.normal(tag + "s", (r["n"], r["L"] * k, r["h"], r["w"]), r["seed"] + 50),
            hashfill.normal(tag + "h", (r["n"], r["C"], r["h"], r["w"]), r["seed"] + 51))


@functools.lru_cache(maxsize=None)
def _rollout_reference(name):
    r = next(q for q in ROLLOUTS if q["name"] == name)
    with torch.no_grad():
        return build_rollout(r)._forward_torch(*rollout_inputs(r))


def rollout_reference(r):
    """the module's own _forward_torch on the CPU in float32, the arithmetic the reference class runs.  Built once; do not modify."""
    return _rollout_reference(r["name"])


def first_flow(r):
    """(max |flow| in pixels, samples beyond the left / right / top / bottom image edge) of the rollout's first step, CPU path"""
    from streamingflow_amd.beverse.basic_modules import conv_block_torch
    net = build_rollout(r)
    sample, hidden = rollout_inputs(r)
    blk, head = (net.flow_pred[0], net.flow_pred[1]) if r["cls"].endswith("V1") else net._flow_modules(0)
    with torch.no_grad():
        flow = F.conv2d(conv_block_torch(blk, torch.cat((sample[:, :r["L"]], hidden), dim=1)), head.weight, head.bias)
    h, w = r["h"], r["w"]
    ix = flow[:, 0] + torch.arange(w, dtype=torch.float32).view(1, 1, w)
    iy = flow[:, 1] + torch.arange(h, dtype=torch.float32).view(1, h, 1)
    return float(flow.abs().max()), dict(left=int((ix < 0).sum()), right=int((ix > w - 1).sum()), top=int((iy < 0).sum()), bottom=int((iy > h - 1).sum()))


def perturbation_movement(r, eps=1e-5):
    """max |rollout(inputs + d) - rollout(inputs)| on the CPU path for hashed d uniform in (-eps, eps) on both inputs"""
    sample, hidden = rollout_inputs(r)
    tag = "bvr_%s_d" % r["name"]
    ds, dh = hashfill.uniform(tag + "s", tuple(sample.shape), -eps, eps, 7), hashfill.uniform(tag + "h", tuple(hidden.shape), -eps, eps, 8)
    with torch.no_grad():
        moved = build_rollout(r)._forward_torch(sample + ds, hidden + dh)
    return float((moved.double() - rollout_reference(r).double()).abs().max())


def measure():
    """name -> e32, printed as the table of the module docstring and the E32 dict"""
    res = {}
    for c in CASES:
        res[c["name"]] = float((reference32(c).double() - reference(c)).abs().max())
        print('    "%s": %.3e,' % (c["name"], res[c["name"]]), flush=True)
    emax = max(res.values())
    print("max e32 = %.3e -> TOL_DIRECT = %.3e, TOL_WINO = %.3e (cap %.0e)" % (emax, 8 * emax, 8 * emax + 2e-5, TOL_CAP))
    return res


if __name__ == "__main__":
    measure()
