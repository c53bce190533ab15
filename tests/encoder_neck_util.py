"""Shared by test_encoder_neck.py (CPU) and test_gpu_encoder_neck.py: the camera neck's cases, hashed weights and endpoints, the
float64 reference and the tolerances.  Everything is regenerated from names and seeds (tools/gen_encoder_neck_golden.py); the
fixture tests/golden/encoder_neck.npz holds what only the reference's own class can say: its float64 outputs at a few channels (the
anchor of ``GEN.neck_f64``, the plain-torch float64 restatement every channel and pixel is compared with) and the float32
reference's own error, which sets the bounds."""
import functools
import os
import sys

import torch

from util import ROOT, gold

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_encoder_neck_golden as GEN  # noqa: E402

CASES = list(GEN.CASES)
WINO_ALLOWANCE = 2e-5      # added where a launch of the chain lands on a Winograd form


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(gold("encoder_neck.npz"))


def build(name_or_version, D=None, backbone=None):
    """This package's Encoder with the hashed state of the case (or of a version with D depth bins), eval mode, CPU."""
    from streamingflow_amd.models.encoder import Encoder
    c = GEN.CASES.get(name_or_version)
    version, D = (c["version"], c["D"]) if c else (name_or_version, D)
    net = Encoder(GEN.cfg(version), D, backbone=backbone)
    neck = {k: v for k, v in net.state_dict().items() if not k.startswith("backbone.")}
    net.load_state_dict(GEN.hashed_state(neck), strict=backbone is None)
    return net.eval()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(feature [n, C, 2H, 2W], depth logits [n, D, 2H, 2W], softmax(depth)) in float64, every channel and pixel: ``GEN.neck_f64`` on
    the case's state and endpoints, held against the reference class's stored channels first.  Computed once per process; callers do
    not modify it."""
    fx = fixture()
    out = GEN.neck_f64(build(name).state_dict(), *GEN.endpoints(name))
    for tag, o in (("feat", out[0]), ("depth", out[1])):
        idx = torch.from_numpy(fx[f"{name}/{tag}_ch"])
        gap = float((o[:, idx] - torch.from_numpy(fx[f"{name}/{tag}"])).abs().max())
        assert gap <= 1e-12, (name, tag, gap)
    return out


def tolerance(name, wino=True):
    """(feature, depth logits, depth probabilities): 8 x the float32 reference's own max error against float64 (measured on the
    reference by the generator, every channel and pixel), + 2e-5 where the chain may run a Winograd launch.  A softmax moves by at
    most the movement of its logits, so the probabilities take the allowance as the logits do."""
    e = fixture()[name + "/err32"]
    return tuple(8.0 * float(v) + (WINO_ALLOWANCE if wino else 0.0) for v in e)
