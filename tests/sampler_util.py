"""Shared by test_sampler.py (CPU, plain-torch path) and test_gpu_sampler.py (device path): the scenes of tools/gen_sampler_golden.py
and the comparison of a sampler result against the REFERENCE's rows in tests/golden/sampler.npz.

The comparison rule.  In fp64 the product's rows differ from the reference's by at most 80 m x 1e-12 (alpha <= 80 times the Fresnel bar)
plus reordered fp64 roundings, far below half an fp32 ulp; after both sides are rounded to fp32 they can differ by one ulp where they
straddle a rounding boundary: |out - fp32(ref)| <= 2^-23 max(1, |ref|) per element.  Neighbouring sort keys come within 1e-9 m of each
other, so rows are not compared position by position with the reference's sorted result but through the product's own order, with U
the reference's unsorted rows:
  (a) out equals fp32(U[order]) within the tolerance;
  (b) keys[order] is non-decreasing up to 1e-9 m (ten times the Fresnel bar at alpha = 80; swapping truly distinct keys violates it);
  (c) order is a permutation;
  (d) inside the run of exactly-zero keys (the lines) order is ascending: the stable sort."""
import functools
import os
import sys

import numpy as np
import torch

from util import ROOT, gold

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_sampler_golden as GEN  # noqa: E402

TAGS = GEN.TAGS
ROW_TOL = 2.0 ** -23
KEY_TOL = 1e-9
FRESNEL_TOL = 1e-12


@functools.lru_cache(maxsize=None)
def golden():
    return gold("sampler.npz")


def scene_args(tag, device, full_grid=False):
    """(v0, kappa, t0, n0 [1, ...], stamps, t_key, uniforms [1, 5, M], counts) of a scene as fp64 tensors on `device`; the stamps are the
    kept ones, or with full_grid every stamp of the fine grid."""
    from streamingflow_amd import sampler as S
    sc = GEN.scene(tag)
    f = lambda a, shape: torch.from_numpy(np.asarray(a, dtype=np.float64).reshape(shape).copy()).to(device)
    tt = sc["tt"] if full_grid else sc["tt"][::sc["fine"]]
    return (f(sc["v0"], (1,)), f(sc["kappa"], (1,)), f(sc["T0"], (1, 2)), f(sc["N0"], (1, 2)), f(tt, (-1,)), float(sc["tt"][-1]),
            f(golden()[f"{tag}.uniforms"], (1, 5, sc["M"])), S.counts(sc["M"], sc["possibility"]))


def check_rows(tag, out, order, what=""):
    """(a) - (d) for out [M, n_t, 3] and order [M] of one scene; prints and returns the largest row error in units of the tolerance."""
    G = golden()
    out = out.detach().cpu().to(torch.float32).numpy().astype(np.float64)
    order = order.detach().cpu().numpy().astype(np.int64)
    U, keys = G[f"{tag}.unsorted"], G[f"{tag}.keys"]
    M = len(keys)
    assert out.shape == U.shape and order.shape == (M,), (out.shape, U.shape, order.shape)
    assert np.array_equal(np.sort(order), np.arange(M)), "order is not a permutation"                         # (c)
    ref = U[order].astype(np.float64)
    gap = float((np.abs(out - ref) / (ROW_TOL * np.maximum(1.0, np.abs(ref)))).max())
    k = keys[order]
    back = float((k[:-1] - k[1:]).max()) if M > 1 else 0.0
    print(f"{tag}{what}: largest row error {gap:.3f} x 2^-23 max(1, |ref|); largest backward step of the sorted keys {max(back, 0.0):.3e} m")
    assert gap <= 1.0, gap                                                                                   # (a)
    assert back <= KEY_TOL, back                                                                             # (b)
    lines = order[k == 0.0]
    assert np.all(np.diff(lines) > 0), "rows with equal keys left their order"                                # (d)
    return gap


def run_scene(tag, device, full_grid=False):
    """The sampler's core on a scene: (rows [M, n, 3], order [M])."""
    from streamingflow_amd import sampler as S
    *args, cnt = scene_args(tag, device, full_grid)
    out, order = S._run(*args, cnt, True)
    return out[0], order[0]
