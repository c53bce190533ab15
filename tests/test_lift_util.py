"""CPU: the numpy oracles of tests/lift_util.py (what test_gpu_lift_kernels.py holds the lift-splat kernels to) against the pinned oracle
oracle/lift_splat.py, bit for bit, and the conditions on the synthetic inputs that make the GPU tests mean something — all from CPU
arithmetic alone, so they hold before any kernel runs."""
import numpy as np
import pytest
import torch

from util import cases, hashfill
from oracle import lift_splat as LS
import lift_util as LU


def _pool_case_csr(tag):
    geo, x, start, res, dim = cases.lift_pool_inputs(tag)
    B, N, D, fH, fW, C = x.shape
    lo = start - res / 2.0
    n = B * N * D * fH * fW
    idx, kept = LU.quantise_oracle(geo.view(-1, 3), lo, res, dim)
    b = np.arange(n) // (n // B)
    n_cells = B * int(dim[0]) * int(dim[1]) * int(dim[2])
    order, cs = LU.csr_oracle(LU.cell_ids(idx, kept, b, dim.tolist()), n_cells)
    return geo, x, start, res, dim, idx, kept, b, order, cs, n_cells


@pytest.mark.parametrize("tag", ["z4_b2", "z1_b1"])
def test_pool_oracle_materialised_equals_sf_bev_pool(tag):
    geo, x, start, res, dim, idx, kept, b, order, cs, n_cells = _pool_case_csr(tag)
    B, C = x.shape[0], x.shape[-1]
    X, Y, Z = (int(v) for v in dim)
    want, want_kept = LS.sf_bev_pool(geo, x, start, res, dim, stable=True)
    assert 0 < kept.sum() < kept.shape[0]
    assert np.array_equal(np.concatenate([idx[kept], b[kept, None]], 1), want_kept.numpy())
    out, s64, sab, length = LU.pool_oracle(order, cs, n_cells, C, x=x.reshape(-1, C))
    assert LU.same_bits(out.reshape(B, Z, X, Y, C).transpose(0, 4, 1, 2, 3), want.numpy())
    assert length.sum() == kept.sum() and length.max() >= 2
    assert (np.abs(out - s64) <= (length[:, None] + 2) * LU.U * sab).all()
    n = kept.shape[0]
    LU.csr_invariants(order, cs, n, n_cells, int(kept.sum()))
    assert np.array_equal(LU.cells_from_csr(order, cs, n), LU.cell_ids(idx, kept, b, dim.tolist()))
    assert set(order[cs[-1]:].tolist()) == set(np.nonzero(~kept)[0].tolist())


def test_pool_oracle_fused_equals_materialised():
    bn, C, D, fH, fW = 3, 20, 11, 5, 7
    fHW = fH * fW
    feat = hashfill.normal("lu_feat", (bn, C, fH, fW), 61)
    logits = hashfill.normal("lu_logits", (bn, D, fH, fW), 62, std=2.0)
    x = LS.depth_outer(feat, logits).reshape(-1, C)                       # [bn*D*fHW, C], the reference's own product
    prob = logits.softmax(dim=1).reshape(-1)
    rays = feat.permute(0, 2, 3, 1).reshape(bn * fHW, C)
    n = bn * D * fHW
    n_cells = 9
    cell = np.floor(hashfill.uniform("lu_cell", (n,), -2.0, n_cells, 63).numpy().astype(np.float64)).astype(np.int64).clip(-1, n_cells - 1)
    order, cs = LU.csr_oracle(cell, n_cells)
    prev = hashfill.normal("lu_prev", (n_cells, C), 64)
    for pv, disc in ((None, 1.0), (prev, 0.5), (prev, 0.9)):
        a = LU.pool_oracle(order, cs, n_cells, C, x=x, prev=pv, discount=disc)
        f = LU.pool_oracle(order, cs, n_cells, C, depth=prob, feat=rays, D=D, fHW=fHW, prev=pv, discount=disc)
        assert LU.same_bits(a[0], f[0]) and np.array_equal(a[3], f[3]) and a[3].max() > 64
        # the fused form's float64 sum is that of the exact products: within one rounding per term of the materialised one
        assert (np.abs(a[1] - f[1]) <= LU.U * f[2]).all()
        assert (np.abs(f[0] - f[1]) <= (f[3][:, None] + 2) * LU.U * f[2]).all()


@pytest.mark.parametrize("discount", [0.5, 0.7])
def test_pool_oracle_blend_equals_projection_to_birds_eye_view(discount):
    """0.7: prev * discount is inexact, so a blend rounded once (a fused multiply-add) would differ from the reference's two torch ops"""
    tag = "tiny"
    feat, depth, geo, ego, (start, res, dim), _ = cases.lift_inputs(tag)
    b, s, n, C, fH, fW = feat.shape
    X, Y = int(dim[0]), int(dim[1])
    x = LS.depth_outer(feat.reshape(b * s * n, C, fH, fW), depth.reshape(b * s * n, -1, fH, fW))
    x = x.reshape(b, s, n, *x.shape[1:])
    want = LS.projection_to_birds_eye_view(x, geo, ego, start, res, dim, discount, stable=True)          # [b, s, C, X, Y]
    mat = LS.pose_vec2mat(ego)
    lo = start - res / 2.0
    for bi in range(b):
        g = LS.warp_geometry(geo[bi], mat[bi, :, :3, :3], mat[bi, :, :3, 3])
        prev = None
        for t in range(s):
            idx, kept = LU.quantise_oracle(g[t].reshape(-1, 3), lo, res, dim)
            order, cs = LU.csr_oracle(LU.cell_ids(idx, kept, 0, dim.tolist()), X * Y)
            prev = LU.pool_oracle(order, cs, X * Y, C, x=x[bi, t].reshape(-1, C), prev=prev, discount=discount)[0]
            assert LU.same_bits(prev.reshape(X, Y, C).transpose(2, 0, 1), want[bi, t].numpy())


def test_quantise_oracle_equals_reference_expression():
    geo, x, start, res, dim = cases.lift_pool_inputs("z4_b2")
    idx, kept = LU.quantise_oracle(geo.view(-1, 3), start - res / 2.0, res, dim)
    q = LS.quantise(geo, start, res).view(-1, 3)
    ok = ((q >= 0) & (q < dim)).all(1)
    assert np.array_equal(kept, ok.numpy()) and np.array_equal(idx[kept], q[ok].numpy())
    for grid in (LU.EDGE_GRID, LU.DYADIC_GRID):                            # and at the cell edges, finite points
        pts = LU.edge_points(grid)
        pts = torch.from_numpy(pts[np.isfinite(pts).all(1) & (np.abs(pts) < 1e29).all(1)])
        lo, rs, dm = torch.tensor(grid["lo"]), torch.tensor(grid["res"]), torch.tensor(grid["dim"])
        q = ((pts - lo) / rs).long()                                      # streamingflow.py:353, torch fp32 on the CPU
        ok = ((q >= 0) & (q < dm)).all(1)
        idx, kept = LU.quantise_oracle(pts, grid["lo"], grid["res"], grid["dim"])
        assert np.array_equal(kept, ok.numpy()) and np.array_equal(idx[kept], q[ok].numpy())
        assert (idx[~kept] == -1).all()


def test_quantise_oracle_drops_what_has_no_cell():
    big = np.float32(2.0 ** 31)
    g = np.array([[np.nan, 0, 0], [np.inf, 0, 0], [-np.inf, 0, 0], [1e30, 0, 0], [-1e30, 0, 0], [big, 0, 0], [-0.0, 0, 0], [-0.5, 0, 0],
                  [-1.0, 0, 0], [4.0, 0, 0], [3.999, 0, 0]], np.float32)
    idx, kept = LU.quantise_oracle(g, [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [4, 1, 1])
    assert kept.tolist() == [False] * 6 + [True, True, False, False, True]
    assert idx[kept].tolist() == [[0, 0, 0], [0, 0, 0], [3, 0, 0]]


@pytest.mark.parametrize("grid,dyadic", [(LU.EDGE_GRID, False), (LU.DYADIC_GRID, True)], ids=["edge", "dyadic"])
def test_edge_point_sets_hold_their_conditions(grid, dyadic):
    pts = LU.edge_points(grid)
    assert pts.shape[0] % grid["n_batch"] == 0
    found = LU.edge_conditions(grid, pts, dyadic)
    print(found)
    idx, kept = LU.quantise_oracle(pts, grid["lo"], grid["res"], grid["dim"])
    half = pts.shape[0] // 2
    for part in (kept[:half], kept[half:]):                               # both batch elements hold kept and dropped points
        assert 0.2 < part.mean() < 0.9


def test_csr_oracle_by_hand():
    cell = np.array([2, -1, 0, 2, 5, -1, 0, 2])
    order, cs = LU.csr_oracle(cell, 6)
    assert order[:6].tolist() == [2, 6, 0, 3, 7, 4] and sorted(order[6:].tolist()) == [1, 5]
    assert cs.tolist() == [0, 2, 2, 5, 5, 5, 6]
    assert LU.cells_from_csr(order, cs, 8).tolist() == cell.tolist()
    LU.csr_invariants(order, cs, 8, 6, 6)
    bad = order.copy()
    bad[[2, 3]] = bad[[3, 2]]                                             # descending inside cell 2
    with pytest.raises(AssertionError):
        LU.csr_invariants(bad, cs, 8, 6, 6)


def test_rig_matches_the_module_host_side_and_the_reference_chain():
    """rig() composes its affines on its own; LiftSplat.rig_affines (torch, runs on the CPU as well) and the reference chain get_geometry ->
    warp_geometry in float64 must give the same positions."""
    from streamingflow_amd.models.lift_splat import LiftSplat
    c = LU.RIG_SMALL
    r = LU.rig_case(c)
    A, us, vs, ds = LU.rig(c["s"], c["n"], c["d_bound"], c["final_dim"], c["down"], c["seed"])
    assert np.array_equal(A, r["A"]) and A.shape == (c["s"] * c["n"], 12) and A.dtype == np.float32
    m = LiftSplat(c["xb"], c["yb"], c["zb"], c["d_bound"], c["final_dim"], c["down"])
    fr = m.frustum.data
    assert np.array_equal(us, fr[0, 0, :, 0].numpy()) and np.array_equal(vs, fr[0, :, 0, 1].numpy()) and np.array_equal(ds, fr[:, 0, 0, 2].numpy())
    assert (r["D"], r["fH"], r["fW"]) == (13, 5, 7) == tuple(fr.shape[:3])
    assert np.abs(m.rig_affines(r["intr"], r["extr"], r["ego"]).view(-1, 12).numpy().astype(np.float64) - A).max() <= 1e-6
    lo, res = torch.tensor(m._grid[1]), torch.tensor(m._grid[2])
    assert np.array_equal(lo.numpy(), r["lo"]) and np.array_equal(res.numpy(), r["res"]) and m._grid[0] == r["dim"]
    s, n = c["s"], c["n"]
    g = LS.get_geometry(fr.double(), r["intr"].double().view(s, n, 3, 3), r["extr"].double().view(s, n, 4, 4))
    mat = LS.pose_vec2mat(r["ego"].double())
    fin = LS.warp_geometry(g, mat[0, :, :3, :3], mat[0, :, :3, 3]).reshape(-1, 3)
    q = ((fin - lo.double()) / res.double()).numpy()
    assert np.abs(q - r["q"]).max() <= 1e-4                                # the affines are rounded to fp32 once: ~60 m * 2^-24 / res


@pytest.mark.parametrize("name", ["RIG_SMALL", "RIG_CROWDED"])
def test_rig_cases_hold_their_conditions(name):
    r = LU.rig_case(getattr(LU, name))
    found = LU.rig_conditions(r)
    print(name, found)
    if name == "RIG_CROWDED":
        assert r["n_points"] == 48384 and r["dim"] == (16, 16, 1) and r["D"] == 48
        assert found["fullest_cell"] >= 129 and found["cells_17_64"] >= 1
    else:
        assert len({r["s"], r["n"], r["D"], r["fH"], r["fW"]}) == 5 and r["dim"] == (24, 20, 1)
    # a clear point's reachable cells are all its own cell; an ambiguous point has more than one
    reach = LU.reachable_cells(r["q"], r["frame"], r["dim"], r["margin"])
    assert (reach[r["clear"]] == r["cell64"][r["clear"], None]).all()
