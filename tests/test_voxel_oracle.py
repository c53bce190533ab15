"""CPU: the voxelisation oracle (oracle/voxelize.py) against fixtures produced by the reference's own
C++ CPU kernel + Voxelization module (tests/golden/voxelize.npz; `python -m oracle.gen_golden --only voxel`),
against its literal sequential formulation, and — when oracle/_ref holds the compiled reference — live."""
import numpy as np
import pytest
import torch

from util import cases, gold
from oracle import voxelize as VZ
import voxel_util as VU


@pytest.mark.parametrize("tag", list(cases.VOXEL_CASES))
def test_oracle_matches_reference_fixture(tag):
    G = gold("voxelize.npz")
    n, F, vs, rng, mp, mv = cases.VOXEL_CASES[tag]
    pts = cases.voxel_points(tag).numpy()
    v, c, k = VZ.hard_voxelize(pts, vs, rng, mp, mv)
    assert np.array_equal(v, G["voxels_" + tag]) and np.array_equal(c, G["coors_" + tag]) and np.array_equal(k, G["num_" + tag])
    v2, c2, k2 = VZ.hard_voxelize_loops(pts, vs, rng, mp, mv)
    assert np.array_equal(v, v2) and np.array_equal(c, c2) and np.array_equal(k, k2)


def test_oracle_matches_compiled_reference_live():
    """the reference kernel's outputs on 4000 random points as stored (tests/golden/voxelize_live.npz, `gen_golden --only
    voxel_live`), and live as well where oracle/_ref holds the compiled kernel"""
    from oracle import build_ref
    G = gold("voxelize_live.npz")
    vs, rng, mp, mv = cases.VOXEL_LIVE        # 12^3 cells
    v, c, k = VZ.hard_voxelize(G["points"], vs, rng, mp, mv)
    assert np.array_equal(G["voxels"], v) and np.array_equal(G["coors"], c) and np.array_equal(G["num"], k)
    ext = build_ref.load_voxel_layer()
    if ext is None:
        return
    pts = torch.from_numpy(G["points"])
    voxels = pts.new_zeros((mv, mp, 5))
    coors = pts.new_zeros((mv, 3), dtype=torch.int)
    num = pts.new_zeros((mv,), dtype=torch.int)
    m = ext.hard_voxelize(pts, voxels, coors, num, vs, rng, mp, mv, 3, True)
    v, c, k = VZ.hard_voxelize(pts.numpy(), vs, rng, mp, mv)
    assert m == v.shape[0]
    assert np.array_equal(voxels[:m].numpy(), v) and np.array_equal(coors[:m].numpy(), c) and np.array_equal(num[:m].numpy(), k)


def test_shipped_grid_properties():
    """1600 x 1600 x 40 grid (the reference's CPU kernel is not memory-safe there): restatement only."""
    vs, rng, mp, mv = cases.VOXEL_SHIPPED
    assert VZ.grid_size(vs, rng) == [1600, 1600, 40]      # the sparse encoder pads z to 41
    g = torch.Generator().manual_seed(2)
    pts = torch.cat([torch.randn((20000, 3), generator=g) * torch.tensor([12.0, 12.0, 1.5]), torch.rand((20000, 2), generator=g)], 1)
    pts = torch.cat([pts, pts[:5000] + 1e-4], 0).numpy()                    # near-duplicates share voxels
    v, c, k = VZ.hard_voxelize(pts, vs, rng, mp, mv)
    _, ok = VZ.point_coors(pts, vs, rng)
    assert int(k.sum()) <= int(ok.sum()) and (k >= 1).all() and (k <= mp).all()
    assert len({tuple(r) for r in c.tolist()}) == c.shape[0]               # one voxel per coordinate
    first = v[:, 0, :]                                                      # first point of every voxel, in appearance order
    idx = [int(np.nonzero((pts == f).all(1))[0][0]) for f in first[:200]]
    assert idx == sorted(idx)
    feats, coords, sizes = VZ.sf_voxelize([torch.from_numpy(pts), torch.from_numpy(pts[:1000])], vs, rng, mp, mv)
    assert feats.shape[0] == coords.shape[0] == sizes.shape[0] and set(coords[:, 0].tolist()) == {0, 1}


@pytest.mark.parametrize("tag", list(cases.VOXEL_CASES))
def test_dynamic_voxelize_oracle_matches_reference_fixture(tag):
    """the max_points == -1 branch (voxelize.py:46-49): per-point coordinates from the reference module on its own C++ kernel"""
    G = gold("voxelize.npz")
    n, F, vs, rng, mp, mv = cases.VOXEL_CASES[tag]
    c = VZ.dynamic_voxelize(cases.voxel_points(tag).numpy(), vs, rng)
    assert c.dtype == np.int32 and np.array_equal(c, G["dyn_coors_" + tag])
    assert ((c == -1).all(1) | (c >= 0).all(1)).all()          # a point is inside on every axis or marked on every axis


def test_dynamic_voxelize_oracle_matches_compiled_reference_live():
    """as above for the dynamic call: stored per-point coordinates, and live where the compiled kernel is here"""
    from oracle import build_ref
    G = gold("voxelize_live.npz")
    vs, rng = cases.VOXEL_LIVE[:2]
    assert np.array_equal(G["dyn_coors"], VZ.dynamic_voxelize(G["points"], vs, rng))
    ext = build_ref.load_voxel_layer()
    if ext is None:
        return
    pts = torch.from_numpy(G["points"])
    coors = pts.new_zeros((pts.shape[0], 3), dtype=torch.int)
    ext.dynamic_voxelize(pts, coors, vs, rng, 3)
    assert np.array_equal(coors.numpy(), VZ.dynamic_voxelize(pts.numpy(), vs, rng))


# ---- the edge clouds of voxel_util.py: the oracle must be right there before the device is held to it -------------------------------
def _oracle(cid):
    pts, vs, rng, mp, mv = VU.case(cid)
    with np.errstate(invalid="ignore"):                     # NaN / inf coordinates -> int64 in point_coors
        return (pts, vs, rng, mp, mv), VZ.hard_voxelize(pts, vs, rng, mp, mv), VZ.dynamic_voxelize(pts, vs, rng)


def test_grid_rounds_half_away_from_zero():
    """C round() of the reference (voxelization_cpu.cpp:123, :159): a ratio ending in .5 rounds up, whole ratios are unchanged"""
    assert VZ.grid_size([2, 1, 1], [-2.5, -2, -2, 2.5, 2, 2]) == [3, 4, 4]
    for cid in ("half_cubic", "half_flat"):
        _, vs, rng, _, _ = VU.case(cid)
        assert VZ.grid_size(vs, rng) == [3, 3, 3], cid
    assert VZ.grid_size([1, 1, 1], [0, 0, 0, 3.5, 4.5, 0.5]) == [4, 5, 1]          # half to even would give 4, 4, 0
    assert VZ.grid_size([1, 1, 1], [0, 0, 0, 2048, 2048, 1023]) == [2048, 2048, 1023]
    assert VZ.grid_size([0.75, 0.75, 0.75], [-4.5, -4.5, -4.5, 4.5, 4.5, 4.5]) == [12, 12, 12]


@pytest.mark.parametrize("cid", VU.CASE_IDS)
def test_edge_case_vectorised_oracle_matches_loops(cid):
    """hard_voxelize (sort, run heads, ranks) against the literal sequential formulation, and dynamic_voxelize against point_coors"""
    (pts, vs, rng, mp, mv), (v, c, k), dyn = _oracle(cid)
    assert pts.dtype == np.float32 and pts.shape[0] <= 3000
    with np.errstate(invalid="ignore"):
        v2, c2, k2 = VZ.hard_voxelize_loops(pts, vs, rng, mp, mv)
        pc, ok = VZ.point_coors(pts, vs, rng)
    assert np.array_equal(v.view(np.uint32), v2.view(np.uint32)) and np.array_equal(c, c2) and np.array_equal(k, k2)
    assert dyn.dtype == np.int32 and np.array_equal(dyn, pc)
    assert ((dyn == -1).all(1) == ~ok).all() and (dyn[ok] >= 0).all()
    g = VZ.grid_size(vs, rng)
    assert (dyn < np.asarray(g)).all() and v.shape[0] == min(VU.occupied(pts, vs, rng), mv)


def test_edge_cases_cover_what_they_are_for():
    """each cloud still reaches the edge it is named after"""
    inside = {}
    for cid in VU.CASE_IDS:
        (pts, vs, rng, mp, mv), (v, c, k), dyn = _oracle(cid)
        inside[cid] = (dyn[:, 0] >= 0)
    n_edge = len(VU.HALF_EDGES)
    for a in range(3):                                      # hand-placed coordinates of half_cubic, on every axis
        assert inside["half_cubic"][a * n_edge:(a + 1) * n_edge].tolist() == VU.HALF_EDGES_INSIDE
    dyn = _oracle("half_cubic")[2]
    assert dyn[:3, 0].tolist() == [2, 2, 2] and dyn[n_edge:n_edge + 3, 1].tolist() == [2, 2, 2]
    for cid in ("pow2_64", "pow2_256", "pow2_4096", "one_cell", "two_cells"):
        frac = inside[cid].mean()
        assert 0.4 <= frac <= 0.6, (cid, frac)
        g = VZ.grid_size(*VU.case(cid)[1:3])
        assert (g[0] * g[1] * g[2]) & (g[0] * g[1] * g[2] - 1) == 0
    (pts, vs, rng, mp, mv), (v, c, k), dyn = _oracle("high_keys")
    g = VZ.grid_size(vs, rng)
    assert g == [2048, 2048, 1023] and g[0] * g[1] * g[2] == 4290772992 < 2 ** 32 - 1
    key = (dyn[:, 2].astype(np.int64) * g[1] + dyn[:, 1]) * g[0] + dyn[:, 0]
    assert (key[inside["high_keys"]] >= 2 ** 31).sum() >= 200 and key.max() == 4290772991 and (~inside["high_keys"]).sum() == 15
    assert v.shape[0] == mv < VU.occupied(pts, vs, rng)
    (pts, vs, rng, mp, mv), _, dyn = _oracle("descending:2xV")
    key = ((dyn[:, 2].astype(np.int64) * 4 + dyn[:, 1]) * 4 + dyn[:, 0])[inside["descending:2xV"]]
    assert (np.diff(key) <= 0).all() and mv == VU.occupied(pts, vs, rng) == 64
    assert VU.occupied(*VU.case("crowd_one")[:3]) == 1 and VU.occupied(*VU.case("crowd_two")[:3]) == 2
    assert not inside["all_outside"].any()
    (pts, vs, rng, mp, mv), (v, c, k), dyn = _oracle("nonfinite")
    bad = ~np.isfinite(pts[:, :3]).all(1)
    assert bad.sum() == 9 and not inside["nonfinite"][bad].any()                   # a non-finite coordinate is outside, on any axis
    assert inside["nonfinite"][9:13].all() and np.signbit(pts[9, 0]) and dyn[9].tolist() == [0, 2, 2]
    assert (v.view(np.uint32) == VU.NAN_PAYLOAD).sum() == 1 and np.isinf(v).sum() == 2


@pytest.mark.parametrize("cid", VU.REFERENCE_IDS)
def test_edge_case_oracle_matches_compiled_reference(cid):
    """the oracle against the compiled reference kernel on the cubic, finite edge clouds: as stored (tests/golden/voxelize_edges.npz,
    `gen_golden --only voxel_edges`) and live where oracle/_ref holds the kernel.  half_cubic pins the grid rounding: with half-to-even
    the oracle forms 2^3 cells there and drops what the reference keeps in cell 2."""
    from oracle import build_ref, gen_golden
    G = gold("voxelize_edges.npz")
    (pts, vs, rng, mp, mv), (v, c, k), dyn = _oracle(cid)
    key = cid.replace(":", "_")
    assert np.array_equal(G["voxels_" + key], v) and np.array_equal(G["coors_" + key], c) and np.array_equal(G["num_" + key], k)
    assert np.array_equal(G["dyn_coors_" + key], dyn)
    ext = build_ref.load_voxel_layer()
    if ext is None:
        return
    rv, rc, rk, rd = gen_golden.run_voxel_reference(ext, pts, vs, rng, mp, mv)
    assert np.array_equal(rv, v) and np.array_equal(rc, c) and np.array_equal(rk, k) and np.array_equal(rd, dyn)
