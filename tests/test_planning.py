"""CPU: the planner's plain-torch path (streamingflow_amd.cost, .models.planning, .metrics.PlanningMetric) against the REFERENCE's
Cost_Function / Planning / PlanningMetric (tests/golden/planning.npz, tools/gen_planning_golden.py).  The generator refused scenes in
which a discretised cell moves under 1 +- 2e-7 / 1 +- 1e-5 scaling of the trajectories, a clamp hides a term or two distinct
trajectories come within 1000 cost tolerances, so selected trajectories and metric counters are demanded exactly.  The tolerances are
derived in planning_util.py and in the generator (refine.tol)."""
import json
import os
from types import SimpleNamespace as NS

import pytest
import torch

import planning_util as PU
from util import GOLD


def _keys():
    with open(os.path.join(GOLD, "planning_state_dict_keys.json")) as f:
        return json.load(f)


def _shipped():
    from streamingflow_amd.models.planning import Planning
    return Planning(PU.GEN.make_cfg(200, 4, 600, 256), 64, 6, 256)


def test_state_dict_keys_and_shapes_are_the_references():
    want = _keys()
    got = {k: list(v.shape) for k, v in _shipped().state_dict().items()}
    assert got == want
    assert len(want) == 119 and "cost_function.safetycost.dx" in want and "cost_function.safetycost.w" in want


def test_reference_shaped_state_dict_loads_strictly():
    net = _shipped()
    sd = {k: torch.full(shape, 0.25) if "num_batches_tracked" not in k else torch.tensor(3) for k, shape in _keys().items()}
    net.load_state_dict(sd, strict=True)
    assert float(net.GRU.weight_hh.detach()[5, 7]) == 0.25 and float(net.cost_function.rulecost.bx.detach()[1]) == 0.25


def test_footprint_tables_at_the_shipped_ego_size():
    cf = _shipped().cost_function
    assert cf.safetycost.rc0.shape == (32, 2) and cf.safetycost.rc_lambda.shape == (192, 2)
    assert cf.safetycost.rc0.min(0)[0].tolist() == [97, 98] and cf.safetycost.rc0.max(0)[0].tolist() == [104, 101]
    assert not any(k.endswith(("rc0", "rc_lambda", "_rc_i32")) for k in cf.state_dict())


def test_corner_on_a_lattice_line_raises():
    from streamingflow_amd.cost import Cost_Function
    cfg = PU.GEN.make_cfg(200, 4, 600, 256)
    Cost_Function(cfg)                          # the shipped rectangle: corners at 96.416, 104.584 and 97.65, 101.35
    cfg.EGO = NS(WIDTH=1.5, HEIGHT=4.084)       # (0.75 + 49.75) / 0.5 = 101 exactly
    with pytest.raises(ValueError):
        Cost_Function(cfg)


def test_non_square_grid_is_refused():
    net, sc = PU.model("n9"), PU.scene("n9")
    lane, drv = PU.maps(sc)
    with pytest.raises(NotImplementedError):
        net.cost_function(sc["cost_volume"][..., :40], sc["trajs"][..., :2], sc["semantic_pred"][..., :40], lane[..., :40], drv[..., :40], sc["target_points"])


@pytest.mark.parametrize("tag", PU.TAGS)
def test_costs_select_and_forward_match_the_reference(tag):
    PU.check_scene(tag, "cpu")


@pytest.mark.parametrize("tag", PU.TAGS)
def test_planning_metric_matches_the_reference(tag):
    PU.check_metric(tag, "cpu")


def test_metric_accumulates_and_resets():
    one, n = PU.metric_of("n66", "cpu", updates=1)
    two, _ = PU.metric_of("n66", "cpu", updates=2)
    assert int(two.total) == 2 * n
    for k in ("obj_col", "obj_box_col"):
        assert torch.equal(getattr(two, k), 2 * getattr(one, k))
    assert all(torch.equal(two.compute()[k], one.compute()[k]) for k in ("obj_col", "obj_box_col"))
    two.reset()
    assert int(two.total) == 0 and not any(bool(getattr(two, k).any()) for k in ("obj_col", "obj_box_col", "L2"))


def test_sync_reduces_total_with_the_sums(monkeypatch):
    """Every rank divides by the number of samples of ALL ranks: sync() hands `total` to the reduction too (two equal ranks here)."""
    from streamingflow_amd import dist
    m, n = PU.metric_of("n66", "cpu")
    before = {k: v.clone() for k, v in m.compute().items()}
    seen = []

    def two_ranks(t, force_collective=False):
        seen.append(t)
        return t.mul_(2)

    monkeypatch.setattr(dist, "reduce_counters", two_ranks)
    m.sync()
    assert any(t is m.total for t in seen) and len(seen) == 4 and int(m.total) == 2 * n
    assert all(torch.equal(m.compute()[k], before[k]) for k in before)


def test_forward_in_training_mode_raises():
    from streamingflow_amd.models.planning import Planning
    sc = PU.scene("n9")
    net = Planning(sc["cfg"], sc["C"], 6, sc["S"]).train()
    with pytest.raises(RuntimeError):
        net(sc["cam_front"], sc["trajs"], sc["gt_trajs"], sc["cost_volume"], sc["semantic_pred"], sc["hd_map"], sc["commands"], sc["target_points"])
    with pytest.raises(NotImplementedError):
        net.loss()


def test_top_level_model_without_planning_is_unchanged():
    """With planning off — PLANNING.ENABLED False or no PLANNING key at all — the model has the modules and state_dict it had; switching
    it on adds exactly the planner and the decoder's cost-volume head."""
    from streamingflow_amd.models.streamingflow import default_cfg, streamingflow
    off = default_cfg()
    off.MODEL.MODALITY.USE_LIDAR = False
    none = default_cfg()
    none.MODEL.MODALITY.USE_LIDAR = False
    none.PLANNING = None
    on = default_cfg()
    on.MODEL.MODALITY.USE_LIDAR = False
    on.PLANNING.ENABLED = True
    keys = {name: set(streamingflow(c).state_dict()) for name, c in (("off", off), ("none", none), ("on", on))}
    assert keys["off"] == keys["none"] and not any(k.startswith("planning.") for k in keys["off"])
    extra = keys["on"] - keys["off"]
    assert keys["off"] < keys["on"] and all(k.startswith(("planning.", "decoder.")) for k in extra)
    assert {"planning." + k for k in _keys()} <= extra
    assert not hasattr(streamingflow(off), "planning")
