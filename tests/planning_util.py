"""Shared by test_planning.py (CPU, plain-torch path) and test_gpu_planning.py (device path): the fixture scenes of
tools/gen_planning_golden.py rebuilt from their seeds, the product's Planning with the hashed weights the reference ran with, and the
comparisons against tests/golden/planning.npz.

Cost tolerances.  cost_fo sums five terms of which the headway area over a drivable probability and the grown-footprint sum reorder
at most 192 terms of one sign, so |delta| <= 224 * 2^-23 * max(1, |value|) (192 + 32 half-ulp roundings).  cost_fc has no area sum:
comfort and progress are chains of correctly rounded IEEE operations (subtract, divide by 0.5, sqrt, square, add) in the reference's own
order, so only a different association of the last few additions can show: 4 * 2^-23 * max(1, |value|).  The safety, rule and divider
terms alone (fixtures <tag>.term.*) are an exact integer, or one square root, times one float each: 1 ulp of the stored value.  A larger
gap means the arithmetic is not the reference's."""
import functools
import os
import sys

import numpy as np
import torch

from util import ROOT, gold

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_planning_golden as GEN  # noqa: E402

COST_TOL = 224 * 2.0 ** -23
FC_TOL = 4 * 2.0 ** -23
TAGS = sorted(GEN.SCENES)


@functools.lru_cache(maxsize=None)
def scene(tag):
    return GEN.scene(tag)


@functools.lru_cache(maxsize=None)
def golden():
    return gold("planning.npz")


def on(sc, device):
    return {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in sc.items()}


@functools.lru_cache(maxsize=None)
def model(tag, device="cpu"):
    from streamingflow_amd.models.planning import Planning
    sc = scene(tag)
    net = Planning(sc["cfg"], sc["C"], 6, sc["S"]).eval()
    net.load_state_dict(GEN.weights(net.state_dict()), strict=True)
    return net.to(device)


def maps(sc):
    hd = sc["hd_map"]
    return (hd[:, 0:1], hd[:, 1:2]) if hd.shape[1] == 2 else (hd[:, 0:2], hd[:, 2:4])


def cost_gap(got, want, tol=COST_TOL):
    """max of |got - want| / (tol * max(1, |want|)): <= 1 is within the bound."""
    got, want = got.detach().cpu().double().numpy(), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((np.abs(got - want) / (tol * np.maximum(1.0, np.abs(want)))).max())


def check_terms(tag, net, sc, cur):
    """The plain-torch term classes alone against the reference's: the terms over boolean maps and the divider term, to 1 ulp."""
    G, cf = golden(), net.cost_function
    lane, drv = maps(sc)
    occ, lane, drv = cf._maps(sc["cost_volume"], sc["semantic_pred"], lane, drv)
    tr = cur[..., :2] * torch.tensor([-1, 1], device=cur.device)
    got = {"safety": cf.safetycost(tr, occ), "rule": cf.rulecost(tr, drv), "divider": cf.lrdividercost(tr, lane)}
    for k, v in got.items():
        want = G[f"{tag}.term.{k}"]
        off = np.abs(torch.clamp(v, 0, 100).cpu().numpy().astype(np.float64) - want.astype(np.float64))
        assert bool((off <= np.spacing(np.abs(want)).astype(np.float64)).all()), (k, float(off.max()))


def check_scene(tag, device):
    """costs, select, forward of one scene on `device` against the fixtures."""
    G, sc, net = golden(), on(scene(tag), device), model(tag, device)
    lane, drv = maps(sc)
    cur = net._command_trajs(sc["trajs"], sc["commands"])
    fc, fo = net.cost_function(sc["cost_volume"], cur[:, :, :, :2], sc["semantic_pred"], lane, drv, sc["target_points"])
    assert fc.dtype == fo.dtype == torch.float32 and fc.device.type == fo.device.type == torch.device(device).type
    gaps = cost_gap(fc, G[f"{tag}.cost_fc"], FC_TOL), cost_gap(fo, G[f"{tag}.cost_fo"])
    print(f"{tag}: cost_fc gap {gaps[0]:.3f}, cost_fo gap {gaps[1]:.3f} (in units of their bounds)")
    assert max(gaps) <= 1.0, gaps
    if torch.device(device).type == "cpu":
        check_terms(tag, net, sc, cur)
    sel = net.select(cur, sc["cost_volume"], sc["semantic_pred"], lane, drv, sc["target_points"])
    assert np.array_equal(sel.cpu().numpy(), G[f"{tag}.selected"])          # values, bit for bit: tied thirds hold equal trajectories
    loss, out = net(sc["cam_front"], sc["trajs"], sc["gt_trajs"], sc["cost_volume"], sc["semantic_pred"], sc["hd_map"], sc["commands"], sc["target_points"])
    assert loss == 0 and tuple(out.shape) == tuple(sel.shape) and out.dtype == torch.float32
    err, tol = float(np.abs(out.cpu().double().numpy() - G[f"{tag}.out"]).max()), float(G["refine.tol"])
    print(f"{tag}: refined trajectory max abs error {err:.3e} (refine.tol {tol:.3e})")
    assert err <= tol, (err, tol)
    assert bool((out[..., 2] == 0).all())


def metric_of(tag, device, updates=1):
    from streamingflow_amd.metrics import PlanningMetric
    sc = scene(tag)
    pred, gt, seg = (t.to(device) for t in GEN.metric_inputs(sc))
    m = PlanningMetric(sc["cfg"], n_future=pred.shape[1]).to(device)
    for _ in range(updates):
        m.update(pred, gt, seg)
    return m, len(pred)


def check_metric(tag, device):
    G = golden()
    m, n = metric_of(tag, device)
    got = m.compute()
    assert int(m.total) == int(G[f"{tag}.metric.total"]) == n
    for k in ("obj_col", "obj_box_col"):
        assert np.array_equal(got[k].cpu().numpy(), G[f"{tag}.metric.{k}"]), k
    want = G[f"{tag}.metric.L2"].astype(np.float64)
    assert float(np.abs(got["L2"].cpu().double().numpy() - want).max()) <= 2.0 ** -21 * float(np.abs(want).max())      # n <= 10 sqrt terms, summed in order
