"""Shared helpers of the parity tests: the product module and the oracle state_dict are filled
with the same hashed weights (oracle.cases / workloads.hashfill), nothing is read from disk."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import cases, refimport  # noqa: E402
from workloads import hashfill  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def make_cfg(C, impute=True, solver="euler", variable=True):
    return refimport.make_cfg(C, impute=impute, solver=solver, variable=variable)


def build_pair(C, solver="euler", impute=True, variable=True, delta_t=0.05, device="cuda"):
    """(product FuturePredictionODE on `device`, oracle state_dict on CPU) with identical weights."""
    import streamingflow_amd as sfa
    net = sfa.FuturePredictionODE(in_channels=C, latent_dim=C, n_future=4, cfg=make_cfg(C, impute, solver, variable),
                                  mixture=True, n_gru_blocks=2, n_res_layers=1, delta_t=delta_t).eval()
    sd = cases.fpode_state_dict(net.state_dict())
    net.load_state_dict(sd)
    if device != "cpu":
        net = net.to(device)
    return net, sd


def wino_plan(c0, c1, cout, n, H, W, dil=1, in_up=0, k=3, epi=0, nprob=1, flags=0):
    """What the conv dispatch decides for a launch of `nprob` identical k x k / stride-1 / pad = dil (k - 1) / 2 layers on n images of H x W
    (sf_debug_wino_plan: host arithmetic under the switches in force, no GPU; the weight pointers are placeholders nobody reads).  flags:
    1 SE input scale, 2 residual, 4 second output.  dict(takes, form 2 plain / 3 dilated / 4 concatenated, segs = [(tile rows per block,
    first tile row, tile rows, workgroups)] — empty where a group runs one by one —, wgs32 = workgroups of the whole launch on 32-tile blocks)"""
    import ctypes
    from streamingflow_amd import _lib
    cin = c0 + c1
    w = _lib.ConvW(w=64, cout=cout, cout_pad=(cout + 15) // 16 * 16, c0=c0, c1=c1, cin_pad=(cin + 31) // 32 * 32, kh=k, kw=k, dil=dil, stride=1,
                   pad=dil * (k - 1) // 2, act=0, w_wino=64)
    out = (ctypes.c_int32 * _lib.SF_WINO_PLAN_INTS)()
    _lib.check(_lib.lib().sf_debug_wino_plan(ctypes.byref(w), epi, n, H, W, in_up, nprob, flags, out, len(out)), "sf_debug_wino_plan")
    return dict(takes=bool(out[0]), form=out[1], segs=[tuple(out[3 + 4 * s:7 + 4 * s]) for s in range(out[2])], wgs32=out[11])


def tiled_plan(layers, n, H, W, epi=0, flags=0, in_up=0):
    """What the conv dispatch decides for ONE launch group of `layers` (dicts: c0, c1, cout, k, and optionally dil, stride, wino = the layer
    was packed with Winograd weights) on n images of H x W (sf_debug_tiled_plan: host arithmetic under the switches in force, no GPU; the
    weight pointers are placeholders nobody reads).  flags: 1 neighbour table, 2 reset gate while staging, 4 SE input scale, 8 split-bf16
    weights, 16 split-K scratch.  dict(family 0 tiled / 1 Winograd / 2 small-P, row planned, row run, mt, ks, key, nsplit per layer)"""
    import ctypes
    from streamingflow_amd import _lib
    ws = (_lib.ConvW * len(layers))()
    for w, l in zip(ws, layers):
        k, dil, cin = l["k"], l.get("dil", 1), l["c0"] + l["c1"]
        w.w, w.cout, w.cout_pad, w.c0, w.c1, w.cin_pad = 64, l["cout"], (l["cout"] + 15) // 16 * 16, l["c0"], l["c1"], (cin + 31) // 32 * 32
        w.kh, w.kw, w.dil, w.stride, w.pad, w.act, w.w_wino = k, k, dil, l.get("stride", 1), dil * (k - 1) // 2, 0, 64 if l.get("wino") else None
    out = (ctypes.c_int32 * _lib.SF_TILED_PLAN_INTS)()
    _lib.check(_lib.lib().sf_debug_tiled_plan(ws, epi, n, H, W, in_up, len(layers), flags, out, len(out)), "sf_debug_tiled_plan")
    return dict(family=out[0], row=out[1], runs=out[2], mt=out[3], ks=out[4], key=out[5], nsplit=list(out[6:6 + len(layers)]))


def gold(name):
    return np.load(os.path.join(GOLD, name))


def maxabs(a, b):
    a = a.detach().cpu() if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))
    b = b.detach().cpu() if isinstance(b, torch.Tensor) else torch.from_numpy(np.asarray(b))
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a.double() - b.double()).abs().max())


def oracle_rollout(sd, sc, hx_nhwc, eps_nhwc, solver="euler", impute=True, prefix="gru_ode"):
    """The oracle's GRU-ODE with Bayesian jumps at the LATENT level: a schedule (streamingflow_amd.schedule.Schedule — itself pinned to 44
    reference-captured schedules) applied with the oracle's own jump / step / infer_state restatements (oracle/ref_torch.py: dual_cell,
    ode_step, infer_state = temporal_ode_bayes.py:562-574 / :436-461 / :463-477) to encoded observations hx [n_obs, h, w, C]; eps
    [n_draws, h, w, C] is consumed in call order, as the reference's global generator would be.  Returns (selected states
    [n_T, h, w, C], final state [h, w, C]) in the product's NHWC layout.  Test infrastructure."""
    from oracle import ref_torch as R
    from streamingflow_amd._lib import OP_JUMP, OP_STEP
    hx = hx_nhwc.detach().cpu().permute(0, 3, 1, 2).contiguous()
    eps = eps_nhwc.detach().cpu().permute(0, 3, 1, 2).contiguous()
    draw = [0]

    def eps_fn(shape, dtype, device):
        e = eps[draw[0]][None]
        draw[0] += 1
        assert tuple(e.shape) == tuple(shape), (e.shape, shape)
        return e

    state = torch.zeros_like(hx[:1])
    inp = torch.zeros_like(hx[:1])
    after = [state]      # state after k ops
    with torch.no_grad():
        for kind, idx in sc.ops:
            if kind == OP_JUMP:
                state = R.dual_cell(sd, prefix + ".gru_obs.gru_d", hx[idx:idx + 1], state, False)
                inp = R.infer_state(sd, prefix, state, eps_fn)[0]
            else:
                assert kind == OP_STEP
                state, inp = R.ode_step(sd, prefix, state, inp, sc.dts[idx], solver, impute, eps_fn)
            after.append(state)
    sel = torch.cat([after[n] for n in sc.sel_nops], 0).permute(0, 2, 3, 1).contiguous()
    return sel, state[0].permute(1, 2, 0).contiguous()
