"""GPU: csrc/voxelize.hip at the places where its design — key, stable radix sort, run heads, scan, binary search — can go wrong and
the fixtures of test_gpu_voxel.py never reach: half-way grid ratios, power-of-two and one-cell grids (the sentinel's sort bit), keys
above 2^31, runs that cross 256-thread blocks, caps under descending arrival order, non-finite coordinates, and what the C entry
points alone promise (voxel_num, zeroed tails, mean-only mode, empty clouds, refusals that write nothing).  The clouds are those of
voxel_util.py; the expectation is oracle/voxelize.py, pinned on the CPU to its sequential form on every cloud and to the compiled
reference kernel where that can run (test_voxel_oracle.py).  Integer and copy work: everything is compared exactly.  The line numbers
in the docstrings are those of streamingflow_amd/csrc/voxelize.hip."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import voxelize as VZ
import voxel_util as VU

pytestmark = pytest.mark.gpu

CANARY_I = 0x5A5A5A5A
CANARY_F = -7.25


def _np(t):
    return t.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("cid", VU.CASE_IDS)
def test_edge_case_exact(cid):
    """every cloud of voxel_util through hard_voxelize_padded, dynamic_voxelize and Voxelization.  Guards: the inside test and the key
    (:51-56; NaN and inf fail f >= 0 && f < g, -0.0 passes), the sort width bits_for(sentinel) (:137-141, :205, :237-238: with a
    power-of-two cell count the sentinel needs one bit more than any cell, or outside points sort in front of cell 0), run heads and
    the scan in point order (:84, :109), the run head by binary search over blocks (:108), the caps (:110, :112, :119), the decoded
    coordinates (:122-126), voxel_num (:102-103), the zero fill of the padded outputs (:215-220) and the grid by roundf (:176, :197)."""
    from streamingflow_amd.voxelize import Voxelization, dynamic_voxelize, hard_voxelize_padded
    pts, vs, rng, mp, mv = VU.case(cid)
    m, V, K3, N = VU.expected_padded(pts, vs, rng, mp, mv)
    assert m == min(VU.occupied(pts, vs, rng), mv)
    dev = torch.from_numpy(pts).cuda()
    r = hard_voxelize_padded(dev, vs, rng, mp, mv)
    assert r["mean"] is None and r["voxel_num"].dtype == torch.int32 and r["coors"].dtype == torch.int32 and r["num"].dtype == torch.int32
    assert int(r["voxel_num"].item()) == m
    got_v, got_c, got_n = _np(r["voxels"]), _np(r["coors"]), _np(r["num"])
    assert np.array_equal(got_c[:m], K3[:m]) and np.array_equal(got_n[:m], N[:m])
    assert _same_bits(got_v[:m], V[:m])                                       # uint32 view: NaN features are copied bit for bit
    if not np.isnan(V).any():
        assert np.array_equal(got_v[:m], V[:m])
    assert not got_v[m:].view(np.uint32).any() and not got_c[m:].any() and not got_n[m:].any()      # the tail is +0 / 0
    with np.errstate(invalid="ignore"):
        want_dyn = VZ.dynamic_voxelize(pts, vs, rng)
    got_dyn = _np(dynamic_voxelize(dev, vs, rng))
    assert got_dyn.dtype == np.int32 and np.array_equal(got_dyn, want_dyn)
    assert ((got_dyn == -1).all(1) | (got_dyn >= 0).all(1)).all()             # outside on any axis: the whole row is -1
    vox = Voxelization(list(vs), list(rng), mp, (mv, mv)).eval()
    v, c, k = vox(dev)
    assert v.shape[0] == m and _same_bits(_np(v), V[:m]) and np.array_equal(_np(c), K3[:m]) and np.array_equal(_np(k), N[:m])
    assert np.array_equal(_np(Voxelization(list(vs), list(rng), -1, (mv, mv)).eval()(dev)), want_dyn)


def test_high_keys_are_above_2_31_and_the_next_grid_is_refused():
    """keys of the upper half of a 2048 x 2048 x 1023 grid do not fit an int: formed in unsigned (:55-56), decoded in unsigned
    (:122-126).  One more z layer makes 2^32 cells, which the 32-bit key cannot hold: SF_ERR_UNSUPPORTED (:201), nothing written."""
    from streamingflow_amd import _lib
    pts, vs, rng, mp, mv = VU.case("high_keys")
    m, V, K3, N = VU.expected_padded(pts, vs, rng, mp, mv)
    g = VZ.grid_size(vs, rng)
    key = (K3[:m, 2].astype(np.int64) * g[1] + K3[:m, 1]) * g[0] + K3[:m, 0]
    assert (key >= 2 ** 31).sum() >= 100 and key.max() == g[0] * g[1] * g[2] - 1 == 4290772991
    assert N[:m][key == key.max()].tolist() == [mp]                           # the very last cell holds 5 points, 3 kept
    b = _Buffers(pts, mp, mv)
    assert b.hard(vs, rng, mp, mv) == _lib.SF_OK
    assert b.voxel_num() == m and np.array_equal(_np(b.coors)[:m], K3[:m]) and np.array_equal(_np(b.num)[:m], N[:m])
    b = _Buffers(pts, mp, mv)
    wide = tuple(rng[:5]) + (1024.0,)
    assert VZ.grid_size(vs, wide) == [2048, 2048, 1024]
    assert b.hard(vs, wide, mp, mv) == _lib.SF_ERR_UNSUPPORTED
    b.assert_untouched()


def test_crowd_one_keeps_the_first_five():
    """3000 points in one cell, max_points 5: a run of 3000 sorted positions whose head is up to eleven blocks behind (:108), the
    stable sort keeps ascending point index inside the run, slots are the ranks 0..4 (:111-112), the count stops at the cap (:119)."""
    from streamingflow_amd.voxelize import hard_voxelize_padded
    pts, vs, rng, mp, mv = VU.case("crowd_one")
    r = hard_voxelize_padded(torch.from_numpy(pts).cuda(), vs, rng, mp, mv)
    assert int(r["voxel_num"].item()) == 1
    assert _np(r["voxels"])[0, :, 3].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]     # by hand: column 3 is the point index
    assert np.array_equal(_np(r["voxels"])[0], pts[:5])
    assert _np(r["num"]).tolist() == [5, 0, 0, 0] and _np(r["coors"]).tolist() == [[1, 2, 3], [0, 0, 0], [0, 0, 0], [0, 0, 0]]
    m, V, K3, N = VU.expected_padded(pts, vs, rng, mp, mv)                     # and the oracle's
    assert m == 1 and np.array_equal(_np(r["voxels"]), V) and np.array_equal(_np(r["coors"]), K3) and np.array_equal(_np(r["num"]), N)


def test_crowd_two_ranks_across_blocks():
    """two cells alternating by point parity, 1500 points each, max_points 700: rank = j - lower_bound (:108, :111) up to 699 with the
    run head up to five blocks back; slot r of the even cell holds point 2r, of the odd cell point 2r + 1"""
    from streamingflow_amd.voxelize import hard_voxelize_padded
    pts, vs, rng, mp, mv = VU.case("crowd_two")
    r = hard_voxelize_padded(torch.from_numpy(pts).cuda(), vs, rng, mp, mv)
    assert int(r["voxel_num"].item()) == 2 and _np(r["num"]).tolist() == [700, 700, 0, 0]
    v = _np(r["voxels"])
    assert np.array_equal(v[0, :, 3], np.arange(0, 1400, 2, dtype=np.float32)) and np.array_equal(v[1, :, 3], np.arange(1, 1400, 2, dtype=np.float32))
    assert _np(r["coors"])[:2].tolist() == [[3, 0, 2], [0, 3, 1]]


@pytest.mark.parametrize("cid", VU.MEAN_IDS)
def test_mean_only_mode(cid):
    """voxels == NULL, mean_feats != NULL (:112, :127-133): coordinates, counts and voxel_num are those of the call that writes the
    voxels; the mean is the sequential fp32 sum of the first num points in index order (__fadd_rn from +0) and one __fdiv_rn —
    checked exactly against that restatement, and against the float64 mean within (num + 1) * 2^-24 * mean|x_i| (derived in
    voxel_util.mean_oracles).  crowd_one: the voxel hit max_points, the mean is over its first 5 points, not its 3000."""
    from streamingflow_amd.voxelize import hard_voxelize_padded
    pts, vs, rng, mp, mv = VU.case(cid)
    m, V, K3, N = VU.expected_padded(pts, vs, rng, mp, mv)
    dev = torch.from_numpy(pts).cuda()
    full = hard_voxelize_padded(dev, vs, rng, mp, mv, want_voxels=True, want_mean=True)
    only = hard_voxelize_padded(dev, vs, rng, mp, mv, want_voxels=False, want_mean=True)
    assert only["voxels"] is None and int(only["voxel_num"].item()) == int(full["voxel_num"].item()) == m
    assert torch.equal(only["coors"], full["coors"]) and torch.equal(only["num"], full["num"])
    assert np.array_equal(_np(only["coors"]), K3) and np.array_equal(_np(only["num"]), N) and _same_bits(_np(full["voxels"]), V)
    seq32, mean64, bound = VU.mean_oracles(V[:m], N[:m])
    for r in (only, full):
        got = _np(r["mean"])
        assert got.shape == (mv, pts.shape[1]) and not got[m:].view(np.uint32).any()
        err = np.abs(got[:m].astype(np.float64) - mean64)
        print(cid, "max |mean - mean64| / bound =", float((err / np.maximum(bound, 1e-300)).max()), "rows", m)
        assert np.array_equal(got[:m], seq32)
        assert (err <= bound).all()
    if cid == "crowd_one":
        assert N[0] == 5 and _np(only["mean"])[0, 3] == 2.0                   # (0 + 1 + 2 + 3 + 4) / 5


@pytest.mark.parametrize("reduce", [True, False])
def test_voxelize_batch_with_an_empty_sample(reduce):
    """streamingflow.voxelize on [descending, all_outside, one point]: the sample index column, no rows from the empty sample
    (voxel_num == 0 slices to nothing, :102-103), with the mean path and with the padded voxel tensor"""
    from streamingflow_amd.voxelize import Voxelization, voxelize
    vs, rng = VU.GRID4
    mp, mv = 3, 10
    clouds = [VU.case("descending:3x10")[0], VU.case("all_outside")[0], VU.case("block_edges:1")[0]]
    vox = Voxelization(list(vs), list(rng), mp, (mv, mv)).eval()
    feats, coords, sizes = voxelize([torch.from_numpy(p).cuda() for p in clouds], vox, voxelize_reduce=reduce)
    want = [VZ.hard_voxelize(p, vs, rng, mp, mv) for p in clouds]
    assert [w[0].shape[0] for w in want] == [10, 0, 1]
    assert coords.dtype == torch.int32 and _np(coords)[:, 0].tolist() == [0] * 10 + [2]
    assert np.array_equal(_np(coords)[:, 1:], np.concatenate([w[1] for w in want])) and _np(coords)[10].tolist() == [2, 2, 2, 2]
    assert np.array_equal(_np(sizes), np.concatenate([w[2] for w in want]))
    wf, wc, wsz = VZ.sf_voxelize([torch.from_numpy(p) for p in clouds], vs, rng, mp, mv)
    assert torch.equal(coords.cpu(), wc) and torch.equal(sizes.cpu(), wsz)
    if reduce:
        seq32 = np.concatenate([VU.mean_oracles(w[0], w[2])[0] for w in want if w[0].shape[0]])
        assert np.array_equal(_np(feats), seq32) and float((feats.cpu() - wf).abs().max()) <= 1e-6
    else:
        assert np.array_equal(_np(feats), np.concatenate([w[0] for w in want]))


# ---- the C entry points: what the Python wrapper never sends ------------------------------------------------------------------------
class _Buffers:
    """canary-filled outputs and a workspace of the documented size for one direct call of sf_hard_voxelize_fwd"""

    def __init__(self, pts, mp, mv, n=None):
        from streamingflow_amd import _lib
        self.L = _lib.lib()
        self.pts = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32)).cuda()
        self.n, self.F = (pts.shape[0] if n is None else n), pts.shape[1]
        self.voxels = torch.full((mv, mp, self.F), CANARY_F, dtype=torch.float32, device="cuda")
        self.mean = torch.full((mv, self.F), CANARY_F, dtype=torch.float32, device="cuda")
        self.coors = torch.full((mv, 3), CANARY_I, dtype=torch.int32, device="cuda")
        self.num = torch.full((mv,), CANARY_I, dtype=torch.int32, device="cuda")
        self.vnum = torch.full((1,), CANARY_I, dtype=torch.int32, device="cuda")
        self.dyn = torch.full((max(pts.shape[0], 1), 3), CANARY_I, dtype=torch.int32, device="cuda")
        self.ws_need = int(self.L.sf_hard_voxelize_ws_bytes(max(pts.shape[0], 1)))
        self.ws = torch.full((self.ws_need + 4096,), 0xA5, dtype=torch.uint8, device="cuda")

    def hard(self, vs, rng, mp, mv, **kw):
        """one call; keywords replace arguments: points, n, F, coors, num, voxels, mean, vnum, ws (tensor or None), ws_bytes"""
        from streamingflow_amd.runtime import ptr, stream_ptr
        a = dict(points=self.pts, n=self.n, F=self.F, voxels=self.voxels, coors=self.coors, num=self.num, mean=self.mean, vnum=self.vnum,
                 ws=self.ws, ws_bytes=self.ws_need)
        a.update(kw)
        st = self.L.sf_hard_voxelize_fwd(ptr(a["points"]), a["n"], a["F"], (C.c_float * 3)(*vs), (C.c_float * 6)(*rng), mp, mv, ptr(a["voxels"]),
                                         ptr(a["coors"]), ptr(a["num"]), ptr(a["mean"]), ptr(a["vnum"]), ptr(a["ws"]), a["ws_bytes"], stream_ptr())
        torch.cuda.synchronize()
        return st

    def dynamic(self, vs, rng, **kw):
        from streamingflow_amd.runtime import ptr, stream_ptr
        a = dict(points=self.pts, n=self.n, F=self.F, coors=self.dyn)
        a.update(kw)
        st = self.L.sf_dynamic_voxelize_fwd(ptr(a["points"]), a["n"], a["F"], (C.c_float * 3)(*vs), (C.c_float * 6)(*rng), ptr(a["coors"]), stream_ptr())
        torch.cuda.synchronize()
        return st

    def voxel_num(self):
        return int(self.vnum.item())

    def assert_untouched(self):
        assert bool((self.voxels == CANARY_F).all()) and bool((self.mean == CANARY_F).all())
        assert bool((self.coors == CANARY_I).all()) and bool((self.num == CANARY_I).all()) and bool((self.vnum == CANARY_I).all())
        assert bool((self.dyn == CANARY_I).all())


def _abi_case():
    return VU.case("pow2_64")


def test_cabi_direct_call_matches_and_leaves_the_slack_alone():
    """the baseline of the refusal tests: the same buffers with valid arguments give the oracle's result, and nothing is written
    behind the ws_bytes the call was told about (:225-233)"""
    from streamingflow_amd import _lib
    pts, vs, rng, mp, mv = _abi_case()
    m, V, K3, N = VU.expected_padded(pts, vs, rng, mp, mv)
    b = _Buffers(pts, mp, mv)
    assert b.hard(vs, rng, mp, mv) == _lib.SF_OK
    assert b.voxel_num() == m and np.array_equal(_np(b.voxels), V) and np.array_equal(_np(b.coors), K3) and np.array_equal(_np(b.num), N)
    assert bool((b.ws[b.ws_need:] == 0xA5).all())
    assert b.dynamic(vs, rng) == _lib.SF_OK and np.array_equal(_np(b.dyn), VZ.dynamic_voxelize(pts, vs, rng))


def test_cabi_empty_cloud():
    """num_points == 0 with points == NULL and no workspace (:221-224; dynamic :168-170): SF_OK, every output zeroed, voxel_num == 0; the
    wrapper and the module on an empty tensor return no rows"""
    from streamingflow_amd import _lib
    from streamingflow_amd.voxelize import Voxelization, dynamic_voxelize
    pts, vs, rng, mp, mv = _abi_case()
    b = _Buffers(pts, mp, mv)
    assert b.hard(vs, rng, mp, mv, points=None, n=0, ws=None, ws_bytes=0) == _lib.SF_OK
    assert b.voxel_num() == 0
    for t in (b.voxels, b.mean, b.coors, b.num):
        assert not _np(t).view(np.uint32).any()
    assert b.dynamic(vs, rng, points=None, n=0) == _lib.SF_OK and bool((b.dyn == CANARY_I).all())      # no point, no row written
    assert b.dynamic(vs, rng, points=None, n=0, coors=None) == _lib.SF_OK     # the empty [0][3] output of the wrapper is a null pointer
    empty = torch.empty((0, 4), dtype=torch.float32, device="cuda")
    v, c, k = Voxelization(list(vs), list(rng), mp, (mv, mv)).eval()(empty)
    assert tuple(v.shape) == (0, mp, 4) and tuple(c.shape) == (0, 3) and tuple(k.shape) == (0,)
    assert tuple(dynamic_voxelize(empty, vs, rng).shape) == (0, 3)


REFUSED = {
    # name: (keywords of _Buffers.hard / .dynamic, voxel_size, range overrides, max_points, max_voxels, applies to the dynamic call)
    "two_features":     (dict(F=2), None, None, None, None, True),
    "max_points_0":     (dict(), None, None, 0, None, False),
    "max_voxels_0":     (dict(), None, None, None, 0, False),
    "voxel_size_0":     (dict(), (1.0, 0.0, 1.0), None, None, None, True),
    "voxel_size_neg":   (dict(), (1.0, 1.0, -1.0), None, None, None, True),
    "voxel_size_nan":   (dict(), (float("nan"), 1.0, 1.0), None, None, None, True),
    "range_reversed":   (dict(), None, (-2.0, 2.0, -2.0, 2.0, -2.0, 2.0), None, None, True),
    "null_coors":       (dict(coors=None), None, None, None, None, True),
    "null_num":         (dict(num=None), None, None, None, None, False),
    "null_points":      (dict(points=None), None, None, None, None, True),
    "negative_points":  (dict(n=-1), None, None, None, None, True),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_cabi_refuses_invalid_arguments_and_writes_nothing(name):
    """SF_ERR_INVALID from the argument checks (:187-189, :196-198, :209; dynamic :168-177) with every output still holding its canary:
    the checks come before the first memset (:215)"""
    from streamingflow_amd import _lib
    kw, vs2, rng2, mp2, mv2, dyn_too = REFUSED[name]
    pts, vs, rng, mp, mv = _abi_case()
    b = _Buffers(pts, mp, mv)
    vs, rng = vs2 or vs, rng2 or rng
    assert b.hard(vs, rng, mp if mp2 is None else mp2, mv if mv2 is None else mv2, **kw) == _lib.SF_ERR_INVALID
    b.assert_untouched()
    if dyn_too:
        assert b.dynamic(vs, rng, **{k: v for k, v in kw.items() if k in ("points", "n", "F", "coors")}) == _lib.SF_ERR_INVALID
        b.assert_untouched()


def test_cabi_workspace_null_or_one_byte_short():
    """SF_ERR_WORKSPACE (:212) for a null workspace and for one byte less than the call needs, nothing written either time.  What the
    call needs — six aligned arrays and rocprim's two scratch sizes at this grid's sort width — is not exported, so it is found as
    the smallest accepted ws_bytes by bisection (the check is a single comparison, monotonic in ws_bytes); it must not exceed
    sf_hard_voxelize_ws_bytes, and a call given exactly that much is right and stays inside it."""
    from streamingflow_amd import _lib
    pts, vs, rng, mp, mv = _abi_case()
    m, V, K3, N = VU.expected_padded(pts, vs, rng, mp, mv)
    b = _Buffers(pts, mp, mv)
    assert b.hard(vs, rng, mp, mv, ws=None) == _lib.SF_ERR_WORKSPACE
    b.assert_untouched()
    assert b.hard(vs, rng, mp, mv, ws_bytes=0) == _lib.SF_ERR_WORKSPACE
    b.assert_untouched()
    lo, hi = 0, b.ws_need                                                     # refused, accepted
    assert b.hard(vs, rng, mp, mv, ws_bytes=hi) == _lib.SF_OK
    while hi - lo > 1:
        mid = (lo + hi) // 2
        st = b.hard(vs, rng, mp, mv, ws_bytes=mid)
        assert st in (_lib.SF_OK, _lib.SF_ERR_WORKSPACE)
        lo, hi = (lo, mid) if st == _lib.SF_OK else (mid, hi)
    assert 6 * 4 * pts.shape[0] <= hi <= b.ws_need
    b = _Buffers(pts, mp, mv)
    assert b.hard(vs, rng, mp, mv, ws_bytes=hi - 1) == _lib.SF_ERR_WORKSPACE
    b.assert_untouched()
    assert b.hard(vs, rng, mp, mv, ws_bytes=hi) == _lib.SF_OK
    assert b.voxel_num() == m and np.array_equal(_np(b.voxels), V) and np.array_equal(_np(b.coors), K3) and np.array_equal(_np(b.num), N)
    assert bool((b.ws[hi:] == 0xA5).all())
