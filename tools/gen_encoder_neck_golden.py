"""TEST INFRASTRUCTURE — tests/golden/encoder_neck.npz and encoder_neck_state_dict_keys.json: the REFERENCE's own ``Encoder``
(streamingflow/models/encoder.py, imported as it is through oracle.refimport.install(), CPU) on hashed weights, BatchNorm statistics
and endpoints.  The third-party ``efficientnet_pytorch`` is absent: a stub module in ``sys.modules`` hands the reference a small
stand-in trunk (``StandInTrunk`` below: a stem and strided conv blocks with the version's endpoint channel counts and the private
attribute names the reference deletes or walks), and ``np.int`` (removed from numpy, used at encoder.py:32) is shimmed.

Usage: python tools/gen_encoder_neck_golden.py        (where the reference is installed)

Weights and inputs are NOT stored: the tests rebuild them with ``hashed_state`` / ``endpoints`` (same hash, same names).  Stored:
  <case>/err32         float64 [3]: max |float32 reference - float64 reference| of (feature, depth logits, softmax(depth)) over EVERY
                       channel and pixel — the tolerances of tests/test_gpu_encoder_neck.py are 8 x these
  <case>/feat_ch, <case>/feat      the float64 reference's feature output [n, k, 2H, 2W] at the channels feat_ch (every pixel)
  <case>/depth_ch, <case>/depth    the same for the depth logits
                       Every channel and pixel would be 3 MB (b4 14x30) and 12 MB (b0 38x40) in float64; a committed file stays under
                       1 MB.  ``neck_f64`` below restates the neck in plain float64 torch; this script refuses to write unless it
                       agrees with the reference class on every channel and pixel to 1e-12, and the tests hold it against the stored
                       channels again before they compare the device result with it on every channel and pixel.
  trunk/hi, trunk/lo   float32: the endpoints the reference's walk selected on the stand-in trunk (b4, images ``trunk_images()``)
  trunk/rates          the drop-connect rate the reference handed each walked block
The file is not written unless every output is O(1) (max |y| in [0.5, 50]) and no ReLU layer of any case is all-dead.
"""
import json
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from workloads import hashfill  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "encoder_neck.npz")
KEYS = os.path.join(ROOT, "tests", "golden", "encoder_neck_state_dict_keys.json")
SEED, GAIN = 7, 1.6
C_OUT = 64
REDUCTION = {"b0": [0, 16, 24, 40, 112, 320], "b4": [0, 24, 32, 56, 160, 448], "b7": [0, 32, 48, 80, 224, 640]}
BREAK = {"b0": 10, "b4": 21, "b7": 37}
# name -> version, images, H, W of the /16 endpoint, D, stored channels per output
CASES = {
    "b4_14x30": dict(version="b4", n=2, H=14, W=30, D=48, keep=2),
    "b4_5x9": dict(version="b4", n=1, H=5, W=9, D=48, keep=None),       # in full
    "b0_38x40": dict(version="b0", n=3, H=38, W=40, D=20, keep=1),
}
TRUNK_VERSION, TRUNK_D = "b4", 48


def cfg(version):
    return NS(NAME="efficientnet-" + version, OUT_CHANNELS=C_OUT, USE_DEPTH_DISTRIBUTION=True, DOWNSAMPLE=8)


def stored_channels(total, keep):
    return list(range(total)) if keep is None else [(1 + i * (total // keep)) % total for i in range(keep)]


def endpoints(name):
    """(reduction_hi [n, c_hi, H, W], reduction_lo [n, c_lo, 2H, 2W]) of a case, float32 CPU."""
    c = CASES[name]
    rc = REDUCTION[c["version"]]
    return (hashfill.normal("neck_hi_" + name, (c["n"], rc[4], c["H"], c["W"]), 51),
            hashfill.normal("neck_lo_" + name, (c["n"], rc[3], 2 * c["H"], 2 * c["W"]), 52))


def hashed_state(sd, prefix=""):
    """Hashed tensors for a state dict whose keys the reference would spell ``prefix + key``."""
    filled = hashfill.fill_state_dict({prefix + k: v for k, v in sd.items()}, seed=SEED, gain=GAIN)
    return {k[len(prefix):]: v for k, v in filled.items()}


# ---- the stand-in trunk ------------------------------------------------------------------------------------------------
class _Block(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        k = 3 if stride == 2 else 1
        self.conv = nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=False)
        self.bn = nn.BatchNorm2d(cout)
        self.seen_rate = None

    def forward(self, x, drop_connect_rate=None):
        self.seen_rate = drop_connect_rate      # identity at inference, as efficientnet_pytorch's drop_connect; recorded for the test
        return F.silu(self.bn(self.conv(x)))


class StandInTrunk(nn.Module):
    """Stem (/2) and blocks reaching /4, /8, /16 at the version's endpoint channel counts by the version's break index, then two
    blocks (/32) behind it — the ones the reference deletes; plus the head attributes it deletes."""

    def __init__(self, version):
        super().__init__()
        rc, brk = REDUCTION[version], BREAK[version]
        self._conv_stem = nn.Conv2d(3, rc[1], 3, stride=2, padding=1, bias=False)
        self._bn0 = nn.BatchNorm2d(rc[1])
        self._swish = nn.SiLU()
        plan, c = [], rc[1]
        for idx in range(brk + 3):
            drop = {1: rc[2], 3: rc[3], 5: rc[4], brk + 1: rc[5]}.get(idx)
            plan.append((c, drop or c, 2 if drop else 1))
            c = drop or c
        self._blocks = nn.ModuleList([_Block(*p) for p in plan])
        self._global_params = NS(drop_connect_rate=0.2)
        self._conv_head, self._bn1 = nn.Conv2d(c, 8, 1), nn.BatchNorm2d(8)
        self._avg_pooling, self._dropout, self._fc = nn.AdaptiveAvgPool2d(1), nn.Dropout(0.2), nn.Linear(8, 4)


def trunk_for_walk(version):
    """The stand-in trunk as the reference leaves it (hashed weights under the reference's ``backbone.`` keys, eval mode), every
    block still in place: the adapter has to stop by itself."""
    t = StandInTrunk(version)
    t.load_state_dict(hashed_state(t.state_dict(), "backbone."))
    return t.eval()


def trunk_images():
    return hashfill.uniform("neck_images", (2, 3, 64, 96), -1.0, 1.0, 53)


# ---- the neck restated in float64 ----------------------------------------------------------------------------------------
def _bn(sd, k, x):
    return F.batch_norm(x, sd[k + ".running_mean"], sd[k + ".running_var"], sd[k + ".weight"], sd[k + ".bias"], False, 0.0, 1e-5)


def _head_f64(sd, p, x):
    cbr = lambda k, x, **kw: F.relu(_bn(sd, p + k[1], F.conv2d(x, sd[p + k[0] + ".weight"], **kw)))
    res = [cbr(("0.convs.0.0", "0.convs.0.1"), x)]
    for i, r in enumerate((12, 24, 36), 1):
        res.append(cbr(("0.convs.%d.0" % i, "0.convs.%d.1" % i), x, padding=r, dilation=r))
    g = cbr(("0.convs.4.1", "0.convs.4.2"), x.mean((2, 3), keepdim=True))
    res.append(g.expand(-1, -1, x.shape[2], x.shape[3]))      # bilinear upsampling of a 1x1 map is a constant
    y = cbr(("0.project.0", "0.project.1"), torch.cat(res, 1))
    y = cbr(("1", "2"), y, padding=1)
    return F.conv2d(y, sd[p + "4.weight"], sd[p + "4.bias"])


def _join_f64(sd, p, x_up, x):
    x_up = F.interpolate(x_up, scale_factor=2, mode="bilinear", align_corners=False)
    y = torch.cat([x, x_up], 1)
    y = F.relu(_bn(sd, p + "conv.1", F.conv2d(y, sd[p + "conv.0.weight"], padding=1)))
    return F.relu(_bn(sd, p + "conv.4", F.conv2d(y, sd[p + "conv.3.weight"], padding=1)))


def neck_f64(sd, hi, lo, dtype=torch.float64):
    """(feature, depth logits, softmax(depth)) in float64 from a neck state dict: the reference's formulation (encoder.py:107-112,
    layers/convolutions.py:183-280) in plain torch.nn.functional calls, eval-mode BatchNorm.  (``dtype`` = float32 on a GPU is the
    stock-PyTorch form tools/neckbench.py times.)"""
    sd = {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point()}
    hi, lo = hi.to(dtype), lo.to(dtype)
    with torch.no_grad():
        feat = _join_f64(sd, "feature_layer_2.", _head_f64(sd, "feature_layer_1.", hi), lo)
        depth = _join_f64(sd, "depth_layer_2.", _head_f64(sd, "depth_layer_1.", hi), lo)
    return feat, depth, depth.softmax(1)


# ---- generation ------------------------------------------------------------------------------------------------------------
def reference_encoder(version, D):
    """The reference's Encoder class over the stand-in trunk, hashed state, eval mode."""
    import types
    from oracle import refimport
    refimport.install()
    if not hasattr(np, "int"):
        np.int = int      # encoder.py:32
    stub = types.ModuleType("efficientnet_pytorch")

    class EfficientNet:
        @staticmethod
        def from_pretrained(name):
            return StandInTrunk(name.split("-")[1])

    stub.EfficientNet = EfficientNet
    sys.modules["efficientnet_pytorch"] = stub
    sys.modules.pop("streamingflow.models.encoder", None)      # another oracle helper may have stubbed it
    import importlib
    enc = importlib.import_module("streamingflow.models.encoder").Encoder(cfg(version), D)
    enc.load_state_dict(hashed_state(enc.state_dict()))
    return enc.eval()


def _run_neck(enc, hi, lo):
    feat = enc.feature_layer_2(enc.feature_layer_1(hi), lo)
    depth = enc.depth_layer_2(enc.depth_layer_1(hi), lo)
    return feat, depth, depth.softmax(dim=1)


def main():
    res, keys = {}, {}
    with torch.no_grad():
        for name, c in CASES.items():
            enc = reference_encoder(c["version"], c["D"])
            neck_sd = {k: v for k, v in enc.state_dict().items() if not k.startswith("backbone.")}
            keys[c["version"]] = list(neck_sd.keys())
            live = {}
            hooks = [m.register_forward_hook(lambda m, i, o, n=n: live.__setitem__(n, float((o > 0).float().mean())))
                     for n, m in enc.named_modules() if isinstance(m, nn.ReLU) and not n.startswith("backbone.")]
            hi, lo = endpoints(name)
            out32 = _run_neck(enc, hi, lo)
            for h in hooks:
                h.remove()
            dead = [n for n, frac in live.items() if frac == 0.0]
            if dead or len(live) < 16:
                sys.exit(f"{name}: ReLU layers with no live output {dead} ({len(live)} seen): nothing written")
            out64 = _run_neck(enc.double(), hi.double(), lo.double())
            mine = neck_f64(neck_sd, hi, lo)
            gap = max(float((a - b).abs().max()) for a, b in zip(mine, out64))
            if gap > 1e-12:
                sys.exit(f"{name}: neck_f64 differs from the reference class by {gap}: nothing written")
            peak = [float(o.abs().max()) for o in out64[:2]]
            if not all(0.5 <= p <= 50.0 for p in peak):
                sys.exit(f"{name}: outputs are not O(1): max |y| {peak}: nothing written")
            err = [float((a.double() - b).abs().max()) for a, b in zip(out32, out64)]
            res[name + "/err32"] = np.asarray(err, dtype=np.float64)
            for tag, o in (("feat", out64[0]), ("depth", out64[1])):
                idx = stored_channels(o.shape[1], c["keep"])
                res[f"{name}/{tag}_ch"] = np.asarray(idx, dtype=np.int64)
                res[f"{name}/{tag}"] = o[:, idx].contiguous().numpy()
            print(f"{name}: feature {tuple(out64[0].shape)} max|y| {peak[0]:.3f}, depth {tuple(out64[1].shape)} max|y| {peak[1]:.3f}, "
                  f"float32 reference error {err}, least live ReLU {min(live.values()):.3f}, neck_f64 gap {gap:.1e}")
        # the walk: the reference's get_features_depth on the stand-in trunk; the endpoints it selected are what its heads were given
        enc = reference_encoder(TRUNK_VERSION, TRUNK_D)
        seen = {}
        h1 = enc.feature_layer_1.register_forward_hook(lambda m, i, o: seen.__setitem__("hi", i[0]))
        h2 = enc.feature_layer_2.register_forward_hook(lambda m, i, o: seen.__setitem__("lo", i[1]))
        feat, depth = enc(trunk_images())
        h1.remove(), h2.remove()
        res["trunk/hi"], res["trunk/lo"] = seen["hi"].contiguous().numpy(), seen["lo"].contiguous().numpy()
        res["trunk/rates"] = np.asarray([b.seen_rate for b in enc.backbone._blocks], dtype=np.float64)
        print(f"trunk: {len(enc.backbone._blocks)} blocks walked, endpoints {tuple(seen['hi'].shape)} / {tuple(seen['lo'].shape)} -> "
              f"{tuple(feat.shape)} / {tuple(depth.shape)}")
    np.savez_compressed(OUT, **res)
    with open(KEYS, "w") as f:
        json.dump(keys, f, indent=0)
    print(OUT, os.path.getsize(OUT), "bytes;", KEYS, os.path.getsize(KEYS), "bytes")


if __name__ == "__main__":
    main()
