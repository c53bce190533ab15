"""CPU: the BEVerse ResFuturePrediction family (streamingflow_amd.beverse: ResFuturePrediction, ResFuturePredictionV2,
ResFuturePredictionV1, GRUCell, warp_with_flow) on its plain-torch path against fixtures generated from the reference classes
(tests/golden/resfuture.npz, resfuture_state_dict_keys.json; tools/gen_resfuture_golden.py).  The torch path states the same
wiring as the device path in torch's own ops, so CPU against CPU the bound is test_beverse.py's 1e-5."""
import json
import os
import sys

import pytest
import torch

from util import GOLD, ROOT, gold, hashfill, maxabs

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_resfuture_golden as GEN  # noqa: E402

CASES = [(t, v) for t in GEN.SHAPES for v in GEN.VARIANTS]


def _modules():
    from streamingflow_amd.beverse import basic_modules as B, motion_modules as M
    return B, M


def test_state_dict_keys_match_reference():
    _, M = _modules()
    with open(os.path.join(GOLD, "resfuture_state_dict_keys.json")) as f:
        want = json.load(f)
    assert set(want) == set(GEN.VARIANTS)
    for variant in GEN.VARIANTS:
        net = GEN.build(M, "s", variant)
        assert list(net.state_dict().keys()) == want[variant], variant
    # V2 without state refinement lists ONE flow head and ONE ConvBlock n_future times: 72 keys over 44 distinct tensors
    sd = GEN.build(M, "s", "v2_shared").state_dict()
    assert len(sd) == 72 and len({v.data_ptr() for v in sd.values()}) == 44
    net = GEN.build(M, "s", "v2_shared")
    assert all(m is net.flow_preds[0] for m in net.flow_preds) and all(m is net.spatial_convs[0] for m in net.spatial_convs)
    net = GEN.build(M, "s", "v2_refine")
    assert net.flow_preds[1] is not net.flow_preds[0]


def test_exported_names():
    import streamingflow_amd.beverse as bv
    for name in ("GRUCell", "warp_with_flow", "ResFuturePrediction", "ResFuturePredictionV2", "ResFuturePredictionV1"):
        assert hasattr(bv, name), name


@pytest.mark.parametrize("tag,variant", CASES)
def test_torch_path_matches_reference_fixture(tag, variant):
    _, M = _modules()
    g = gold("resfuture.npz")
    net = GEN.build(M, tag, variant)
    sample, hidden = GEN.inputs(tag, variant)
    s0, h0 = sample.clone(), hidden.clone()
    out = net(sample, hidden)
    C, L, h, w, B = GEN.SHAPES[tag]
    T = GEN.N_FUTURE + (1 if variant.startswith("v1") else 0)
    assert tuple(out.shape) == (B, T, C, h, w)
    assert torch.equal(sample, s0) and torch.equal(hidden, h0)
    err = maxabs(out[:, :, GEN.channels(tag)], g[f"{tag}/{variant}/out"])
    print(tag, variant, "max |torch path - reference|", err)
    assert err <= 1e-5


@pytest.mark.parametrize("tag,variant", [c for c in CASES if GEN.has_flow(c[1])])
def test_cpu_warp_with_flow(tag, variant):
    _, M = _modules()
    g = gold("resfuture.npz")
    _, hidden = GEN.inputs(tag, variant)
    flow = torch.from_numpy(g[f"{tag}/{variant}/flow0"])
    before = flow.clone()
    out = M.warp_with_flow(hidden, flow)
    assert torch.equal(flow, before)      # unlike the reference, the caller's flow is left alone
    assert maxabs(out[:, GEN.channels(tag)], g[f"{tag}/{variant}/warp0"]) <= 1e-5


def test_gru_cell_torch_path():
    B, _ = _modules()
    g = gold("resfuture.npz")
    cell = GEN.build_gru_cell(B)
    x, s = GEN.gru_cell_inputs()
    assert maxabs(cell(x, s), g["gru_cell/out"]) <= 1e-5
    assert list(cell.state_dict().keys()) == list(B.SpatialGRU(48, 32).state_dict().keys())


def test_v1_without_flow_warp_is_refused():
    _, M = _modules()
    with pytest.raises(NotImplementedError):
        M.ResFuturePredictionV1(16, 8, 3, flow_warp=False)


@pytest.mark.parametrize("variant", ["res_flow", "v2_refine", "v1"])
def test_train_mode_raises(variant):
    B, M = _modules()
    net = GEN.build(M, "s", variant)
    sample, hidden = GEN.inputs("s", variant)
    net.train()
    with pytest.raises(RuntimeError, match="inference-only"):
        net(sample, hidden)
    cell = GEN.build_gru_cell(B).train()
    with pytest.raises(RuntimeError, match="inference-only"):
        cell(*GEN.gru_cell_inputs())


@pytest.mark.parametrize("C,L", [(18, 8), (16, 6)])
def test_unsupported_channel_counts_raise(C, L):
    B, M = _modules()
    for cls in (M.ResFuturePrediction, M.ResFuturePredictionV2, M.ResFuturePredictionV1):
        with pytest.raises(NotImplementedError):
            cls(C, L, 3)
    with pytest.raises(NotImplementedError):
        B.GRUCell(C + L, C)


def test_detach_state_has_no_effect():
    _, M = _modules()
    sample, hidden = GEN.inputs("s", "res_flow")
    outs = []
    for detach in (True, False):
        net = M.ResFuturePrediction(16, 8, GEN.N_FUTURE, detach_state=detach)
        net.load_state_dict(hashfill.fill_state_dict(net.state_dict(), seed=2, gain=1.0))
        outs.append(net.eval()(sample, hidden))
    assert torch.equal(outs[0], outs[1])
