"""CPU: the camera ``Encoder``'s host side (streamingflow_amd/models/encoder.py) against the fixture generated from the reference's own
class (tests/golden/encoder_neck.npz, encoder_neck_state_dict_keys.json; tools/gen_encoder_neck_golden.py): state_dict keys and a
strict load, the twin-head packing, the dead-branch rule, the EfficientNet walk.  The device side is test_gpu_encoder_neck.py."""
import json
import os

import pytest
import torch

import encoder_neck_util as U
from encoder_neck_util import GEN
from streamingflow_amd.models import encoder as E      # fails on a tree without the feature: the module is new
from util import GOLD


def test_state_dict_keys_match_reference_and_load_strict():
    with open(os.path.join(GOLD, "encoder_neck_state_dict_keys.json")) as f:
        want = json.load(f)
    assert set(want) == {"b0", "b4"}
    for version, D in (("b4", 48), ("b0", 20)):
        net = E.Encoder(GEN.cfg(version), D)
        assert list(net.state_dict().keys()) == want[version], version
        assert not any(k.startswith("backbone.") for k in want[version])
        filled = GEN.hashed_state(net.state_dict())
        net.load_state_dict(filled, strict=True)
        assert all(torch.equal(v, filled[k]) for k, v in net.state_dict().items())
    assert E.Encoder(GEN.cfg("b4"), 48).c_hi == 160 and E.Encoder(GEN.cfg("b7"), 48).c_lo == 80


def test_variants_outside_the_shipped_configs_raise():
    cfg = GEN.cfg("b4")
    cfg.NAME = "efficientnet-b3"
    with pytest.raises(NotImplementedError):
        E.Encoder(cfg, 48)
    cfg = GEN.cfg("b4")
    cfg.USE_DEPTH_DISTRIBUTION = False
    with pytest.raises(NotImplementedError):
        E.Encoder(cfg, 48)
    with pytest.raises(RuntimeError, match="backbone"):
        U.build("b4", 48)(torch.zeros(1, 3, 64, 96))


def test_dead_rates():
    rates = (12, 24, 36)
    assert E.dead_rates(rates, 14, 30) == (36,)            # 24 is dead along y only: two live taps
    assert E.dead_rates(rates, 5, 9) == (12, 24, 36)
    assert E.dead_rates(rates, 38, 40) == ()
    assert E.dead_rates(rates, 12, 12) == (12, 24, 36) and E.dead_rates(rates, 13, 12) == (24, 36) and E.dead_rates(rates, 12, 13) == (24, 36)


def test_dead_rate_means_centre_tap_only():
    """the rule against torch: on an image a rate is dead on, the dilated 3x3 equals the 1x1 of its centre tap (the other taps add
    exact zeros; 1e-13 leaves room for a different summation order over the input channels)"""
    torch.manual_seed(0)
    w = torch.randn(4, 3, 3, 3, dtype=torch.float64)
    for (H, W), rate, same in (((14, 30), 36, True), ((14, 30), 24, False), ((5, 9), 12, True), ((12, 13), 12, False)):
        x = torch.randn(1, 3, H, W, dtype=torch.float64)
        full = torch.nn.functional.conv2d(x, w, padding=rate, dilation=rate)
        centre = torch.nn.functional.conv2d(x, w[:, :, 1:2, 1:2])
        gap = float((full - centre).abs().max())
        assert (gap <= 1e-13) if same else (gap > 1e-2), ((H, W), rate, gap)
        assert (rate in E.dead_rates((rate,), H, W)) == same


@pytest.mark.parametrize("collapsed", [(), (36,), (12, 24, 36)], ids=str)
def test_twin_head_packing(collapsed):
    net = U.build("b4_14x30")
    f, d = net.feature_layer_1, net.depth_layer_1
    t = E.twin_head_tensors(f, d, collapsed)
    hid, C = 64, 160
    assert t["hid"] == 2 * hid and t["C"] == C
    for i in range(4):
        wf, wd = f[0].convs[i][0].weight, d[0].convs[i][0].weight
        dil = f[0].convs[i][0].dilation[0]
        if dil in collapsed:
            wf, wd, dil = wf[:, :, 1:2, 1:2], wd[:, :, 1:2, 1:2], 1
        assert t["branch_dil"][i] == dil and tuple(t["branch_w"][i].shape) == (2 * hid, C) + tuple(wf.shape[2:])
        assert torch.equal(t["branch_w"][i][:hid], wf) and torch.equal(t["branch_w"][i][hid:], wd)
    assert torch.equal(t["pool_w"][:hid], f[0].convs[4][1].weight[:, :, 0, 0]) and torch.equal(t["pool_w"][hid:], d[0].convs[4][1].weight[:, :, 0, 0])
    pf, pd = f[0].project[0].weight, d[0].project[0].weight
    pw = t["project_w"]
    assert tuple(pw.shape) == (2 * hid, 8 * hid, 1, 1)
    for i in range(4):      # branch i of the twin cat is [feature | depth]
        blk = pw[:, 2 * hid * i:2 * hid * (i + 1)]
        assert torch.equal(blk[:hid, :hid], pf[:, hid * i:hid * (i + 1)]) and torch.equal(blk[hid:, hid:], pd[:, hid * i:hid * (i + 1)])
        assert not blk[:hid, hid:].any() and not blk[hid:, :hid].any()
    for key, a, b in (("proj_pool_w", pf[:, 4 * hid:, 0, 0], pd[:, 4 * hid:, 0, 0]), ("conv3_w", f[1].weight, d[1].weight),
                      ("cls_w", f[4].weight, d[4].weight)):
        w = t[key]
        ra, ca = a.shape[:2]
        assert tuple(w.shape[:2]) == (ra + b.shape[0], ca + b.shape[1])
        assert torch.equal(w[:ra, :ca], a) and torch.equal(w[ra:, ca:], b)
        assert not w[:ra, ca:].any() and not w[ra:, :ca].any()
    assert torch.equal(t["cls_b"], torch.cat([f[4].bias, d[4].bias]))


def test_twin_head_computes_both_heads():
    """the twin tensors run as ONE head in plain float64 torch give [feature head | depth head] of the reference formulation"""
    name = "b4_5x9"
    net = U.build(name)
    hi, _ = GEN.endpoints(name)
    sd = {k: v.double() for k, v in net.state_dict().items()}
    want = torch.cat([GEN._head_f64(sd, "feature_layer_1.", hi.double()), GEN._head_f64(sd, "depth_layer_1.", hi.double())], 1)
    t = E.twin_head_tensors(net.feature_layer_1, net.depth_layer_1, E.dead_rates((12, 24, 36), 5, 9))
    F = torch.nn.functional
    f, d = net.feature_layer_1, net.depth_layer_1

    def bn2(a, b, x):
        g = lambda n: torch.cat([getattr(a, n), getattr(b, n)]).double()
        return F.relu(F.batch_norm(x, g("running_mean"), g("running_var"), g("weight"), g("bias"), False, 0.0, a.eps))

    x = hi.double()
    cat = [bn2(f[0].convs[i][1], d[0].convs[i][1], F.conv2d(x, t["branch_w"][i].double(), dilation=t["branch_dil"][i],
                                                           padding=t["branch_dil"][i] * (t["branch_w"][i].shape[2] // 2))) for i in range(4)]
    g = bn2(f[0].convs[4][2], d[0].convs[4][2], F.conv2d(x.mean((2, 3), keepdim=True), t["pool_w"].double()[:, :, None, None]))
    pre = F.conv2d(torch.cat(cat, 1), t["project_w"].double()) + F.conv2d(g, t["proj_pool_w"].double()[:, :, None, None])
    y = bn2(f[0].project[1], d[0].project[1], pre)
    y = bn2(f[2], d[2], F.conv2d(y, t["conv3_w"].double(), padding=1))
    got = F.conv2d(y, t["cls_w"].double(), t["cls_b"].double())
    assert float((got - want).detach().abs().max()) <= 1e-12


def test_efficientnet_endpoints_walk():
    fx = U.fixture()
    trunk = GEN.trunk_for_walk(GEN.TRUNK_VERSION)
    walk = E.EfficientNetEndpoints(trunk, GEN.TRUNK_VERSION, 8).eval()
    with torch.no_grad():
        hi, lo = walk(GEN.trunk_images())
    assert torch.equal(hi, torch.from_numpy(fx["trunk/hi"])) and torch.equal(lo, torch.from_numpy(fx["trunk/lo"]))
    brk = E.BREAK_INDEX[GEN.TRUNK_VERSION]
    rates = [b.seen_rate for b in trunk._blocks]
    assert rates[brk + 1:] == [None, None]                 # the blocks behind the break are not walked
    assert rates[:brk + 1] == list(fx["trunk/rates"])      # drop-connect scaled by idx / (blocks the reference keeps)
    with pytest.raises(NotImplementedError):
        E.EfficientNetEndpoints(trunk, "b3", 8)
    enc = U.build("b4", 48, backbone=walk)
    assert [k for k in enc.state_dict() if not k.startswith("backbone.")] == list(U.build("b4", 48).state_dict())
