"""GPU: the kernels of csrc/lift_splat.hip one at a time through the C ABI, where the shipped frustum puts them and the rig cases of
test_gpu_lift.py do not: crowded cells on the fused pooling kernel (one in-flight group / padded groups / more than one 64-point chunk),
the quantiser at the cell edges, the rig quantiser against float64, and the fused chain on a crowded frustum with index and pooling
checked separately.

Every expected value comes from tests/lift_util.py (numpy; pinned to oracle/lift_splat.py by test_lift_util.py) or from float64.  Sums
are compared bit for bit with the sequential fp32 sum in list order; the float64 bound (L + 2) 2^-24 sum|term| for a cell of L points is
the textbook bound of L sequential additions, derived in lift_util.pool_oracle, and is a sanity check on the oracle itself.

What each test was seen to catch (one-line changes of the source built into a scratch library, never kept), a = pool kernels on the
hand-built CSR, b = index at the cell edges / range ends, c = rig index against float64, d = crowded chain:
  base += 64 -> 32 in the chunk loop: a, d            padded slots not zeroed: a, d            readlane index wrong from the second chunk on: a, d
  ray decode p % fHW -> p % (D*fHW) clamped: a (fused), d        blend as one fused multiply-add: a (discount 0.9), d (0.7)
  qx > -1 -> qx >= 0: b, c, d        qy > -1 -> qy >= -1: b (dyadic grid only)        qx < X -> qx <= X: b        divide -> multiply by 1/res: b
  X and Y swapped in the key of cell_of: b, c        in the key or range test of the integer path: b (range ends)
  t / n_cam -> t % n_cam, h and w decoded in swapped order in the rig kernel: c, d"""
import functools

import numpy as np
import pytest
import torch

from util import hashfill
import lift_util as LU
from streamingflow_amd._lib import SF_ERR_INVALID

pytestmark = pytest.mark.gpu

CANARY = 12345.0
PAD = 64


def _api():
    from streamingflow_amd import _lib, runtime
    return _lib.lib(), runtime.ptr, runtime.stream_ptr()


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _grid_args(lo, res, dim):
    from streamingflow_amd import _lib
    C = _lib.C
    return (C.c_float * 3)(*[float(v) for v in lo]), (C.c_float * 3)(*[float(v) for v in res]), (C.c_int32 * 3)(*[int(v) for v in dim])


def _guarded(n, dtype=torch.float32, fill=CANARY):
    """(buffer with PAD canaries on either side, the view between them)"""
    buf = torch.full((PAD + n + PAD,), fill, dtype=dtype, device="cuda")
    return buf, buf[PAD:PAD + n]


def _canaries_intact(buf, fill=CANARY):
    b = buf.cpu()
    return bool((b[:PAD] == fill).all()) and bool((b[-PAD:] == fill).all())


def _index_buffers(n, n_cells):
    from streamingflow_amd import runtime
    L = _api()[0]
    obuf, order = _guarded(n, torch.int32, -7)
    sbuf, start = _guarded(n_cells + 1, torch.int32, -7)
    ws = runtime.workspace(L.sf_lift_index_ws_bytes(n, n_cells), torch.device("cuda"))
    return obuf, order, sbuf, start, ws


# ---- a. pooling kernels on a hand-built CSR ------------------------------------------------------------------------------------------
# 0 / 1 / 15 / 16 points: one in-flight group, empty to full; 17 / 63 / 64: padded groups up to one full chunk; 65 ... 200: the outer
# loop reloads row / dv per 64-point chunk (one point, 63, 64, 65 and 136 = 2 x 64 + 8 points beyond the first chunk)
LENGTHS = [0, 1, 15, 16, 17, 0, 63, 64, 65, 127, 128, 129, 200, 0, 1]
OTHER_FRAME = [3, 0, 20, 1, 0, 7, 9, 0, 0, 30, 2, 0, 18, 10, 0]             # 100 points: the frames before and after in the offset table
ROWS, D, FHW = 3, 11, 35
N = ROWS * D * FHW                                                          # 1155


@functools.lru_cache(maxsize=None)
def _pool_tables():
    """'plain': the cell table starts at list position 0; 'middle': it is the middle third of a three-frame table, as the wrappers pass
    start[f*X*Y:].  -> {name: (order [N], table, first entry of the frame's third)}"""
    assert sum(LENGTHS) == 826 and sum(OTHER_FRAME) == 100 and len(OTHER_FRAME) == len(LENGTHS) == 15
    order = np.random.RandomState(11).permutation(N).astype(np.int64)        # list order is the contract, not point order
    assert (np.diff(order) < 0).any()
    plain = np.concatenate([[0], np.cumsum(LENGTHS)])
    three = np.concatenate([[0], np.cumsum(OTHER_FRAME + LENGTHS + OTHER_FRAME)])
    assert N - plain[-1] == 329 and three[-1] == 1026 and three[15] == 100
    return {"plain": (order, plain, 0), "middle": (order, three, 15)}


@functools.lru_cache(maxsize=None)
def _pool_inputs(C):
    depth = hashfill.uniform("lk_depth", (N,), 0.001, 1.0, 71).numpy()
    feat = hashfill.normal("lk_feat_%d" % C, (ROWS * FHW, C), 72).numpy()
    x = depth[:, None] * feat.reshape(ROWS, 1, FHW, C).repeat(D, 1).reshape(N, C)       # [row][d][hw]: no index decode
    assert x.dtype == np.float32
    prev = hashfill.normal("lk_prev_%d" % C, (len(LENGTHS), C), 73).numpy()
    return depth, feat, x, prev


@pytest.mark.parametrize("table", ["plain", "middle"])
@pytest.mark.parametrize("blend", [None, 0.5, 0.9])
@pytest.mark.parametrize("C", [1, 20, 64, 65, 130])
@pytest.mark.parametrize("kernel", ["fused", "materialised"])
def test_pool_kernels_on_a_hand_built_csr(kernel, C, blend, table):
    """1155 points (3 camera rows x D = 11 x fHW = 35) in a fixed shuffle; 826 of them in the 15 cells, the rest behind the frame's last
    entry; C on either side of the 64-channel chunk; no blend / exact product (0.5) / inexact product (0.9)."""
    L, ptr, st = _api()
    order, tab, first = _pool_tables()[table]
    depth, feat, x, prev = _pool_inputs(C)
    n_cells = len(LENGTHS)
    pv, disc = (None, 1.0) if blend is None else (prev, blend)
    want, s64, sab, length = LU.pool_oracle(order, tab[first:], n_cells, C, x=x, prev=pv, discount=disc)
    if kernel == "fused":
        want_f = LU.pool_oracle(order, tab[first:], n_cells, C, depth=depth, feat=feat, D=D, fHW=FHW, prev=pv, discount=disc)[0]
        assert LU.same_bits(want, want_f)
    assert length.tolist() == LENGTHS
    o_d, t_d = _dev(order, np.int32), _dev(tab, np.int32)
    p_d = None if pv is None else _dev(pv, np.float32)
    buf, out = _guarded(n_cells * C)
    if kernel == "fused":
        f_d, d_d = _dev(feat, np.float32), _dev(depth, np.float32)
        rc = L.sf_lift_pool_fused_fwd(ptr(f_d), ptr(d_d), D, FHW, ptr(o_d), ptr(t_d[first:]), n_cells, C, ptr(p_d), disc, ptr(out), st)
    else:
        x_d = _dev(x, np.float32)
        rc = L.sf_lift_pool_fwd(ptr(x_d), ptr(o_d), ptr(t_d[first:]), n_cells, C, ptr(p_d), disc, ptr(out), st)
    assert rc == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(n_cells, C)
    assert _canaries_intact(buf)
    assert p_d is None or LU.same_bits(p_d.cpu().numpy(), pv)
    bad = np.nonzero((got.view(np.int32) != want.view(np.int32)).any(1))[0]
    assert bad.size == 0, "cells %s (lengths %s) differ from the sequential fp32 sum" % (bad.tolist(), [LENGTHS[i] for i in bad])
    assert (np.abs(got.astype(np.float64) - s64) <= (length[:, None] + 2) * LU.U * sab).all()
    empty = [i for i, n in enumerate(LENGTHS) if n == 0]
    if pv is None:
        assert (got[empty].view(np.int32) == 0).all()                        # +0, not -0
    else:
        assert LU.same_bits(got[empty], pv[empty] * np.float32(disc))


def test_pool_entry_points_refuse_empty_shapes():
    L, ptr, st = _api()
    a = torch.zeros(256, device="cuda")
    i = torch.zeros(256, dtype=torch.int32, device="cuda")
    for n_cells, C in ((0, 4), (-1, 4), (2, 0), (2, -3)):
        assert L.sf_lift_pool_fwd(ptr(a), ptr(i), ptr(i), n_cells, C, None, 1.0, ptr(a), st) == SF_ERR_INVALID
        assert L.sf_lift_pool_fused_fwd(ptr(a), ptr(a), 2, 2, ptr(i), ptr(i), n_cells, C, None, 1.0, ptr(a), st) == SF_ERR_INVALID
    for Dv, fHW in ((0, 2), (-1, 2), (2, 0)):
        assert L.sf_lift_pool_fused_fwd(ptr(a), ptr(a), Dv, fHW, ptr(i), ptr(i), 2, 4, None, 1.0, ptr(a), st) == SF_ERR_INVALID
    assert L.sf_lift_pool_fused_fwd(ptr(a), ptr(a), 2, 2, ptr(i), ptr(i), 2, 4, None, 1.0, ptr(a), st) == 0     # all-empty cells: zeros
    torch.cuda.synchronize()
    assert float(a[:8].abs().max()) == 0.0


# ---- b. the quantiser at the cell edges --------------------------------------------------------------------------------------------------
def _check_index(order, start, n, n_cells, cell):
    """the kernel's CSR against csr_oracle: kept prefix exactly, tail as a set"""
    want_order, want_start = LU.csr_oracle(cell, n_cells)
    kept = int(want_start[-1])
    assert np.array_equal(start, want_start)
    assert np.array_equal(order[:kept], want_order[:kept])
    assert sorted(order[kept:].tolist()) == sorted(want_order[kept:].tolist())
    LU.csr_invariants(order, start, n, n_cells, kept)


def _run_index_geom(pts, grid):
    L, ptr, st = _api()
    n, nb = pts.shape[0], grid["n_batch"]
    X, Y, Z = grid["dim"]
    n_cells = nb * X * Y * Z
    obuf, order, sbuf, start, ws = _index_buffers(n, n_cells)
    cbuf, coords = _guarded(4 * n, torch.int32, -7)
    g = _dev(pts, np.float32)
    lo, res, dim = _grid_args(grid["lo"], grid["res"], grid["dim"])
    assert L.sf_lift_index_fwd(ptr(g), n, nb, lo, res, dim, ptr(coords), ptr(order), ptr(start), ptr(ws), ws.numel() * 4, st) == 0
    torch.cuda.synchronize()
    assert _canaries_intact(obuf, -7) and _canaries_intact(sbuf, -7) and _canaries_intact(cbuf, -7)
    return coords.cpu().numpy().reshape(n, 4), order.cpu().numpy().astype(np.int64), start.cpu().numpy().astype(np.int64), n_cells


def _check_index_geom(pts, grid):
    coords, order, start, n_cells = _run_index_geom(pts, grid)
    n = pts.shape[0]
    idx, kept = LU.quantise_oracle(pts, grid["lo"], grid["res"], grid["dim"])
    b = np.arange(n) // (n // grid["n_batch"])
    want = np.concatenate([idx, np.where(kept, b, -1)[:, None]], 1)
    bad = np.nonzero((coords != want).any(1))[0]
    assert bad.size == 0, "points %s: got %s, want %s" % (pts[bad[:4]].tolist(), coords[bad[:4]].tolist(), want[bad[:4]].tolist())
    _check_index(order, start, n, n_cells, LU.cell_ids(idx, kept, b, grid["dim"]))
    return kept


@pytest.mark.parametrize("grid,dyadic", [(LU.EDGE_GRID, False), (LU.DYADIC_GRID, True)], ids=["edge", "dyadic"])
def test_index_geom_at_the_cell_edges(grid, dyadic):
    pts = LU.edge_points(grid)
    print(LU.edge_conditions(grid, pts, dyadic))                            # the set holds what the test is about (asserted inside)
    kept = _check_index_geom(pts, grid)
    assert 0 < kept.sum() < kept.shape[0]
    two = pts[np.nonzero(kept)[0][[0, -1]]]                                  # n_points = 2: one point per batch element
    assert _check_index_geom(two, grid).all()


def test_index_coords_at_the_range_ends():
    """(x, y, z, b) at -1, 0, dim - 1 and dim on each component, B, Z, X, Y all different: a swapped pair in the key or in the range test shows"""
    L, ptr, st = _api()
    B, Z, X, Y = 2, 3, 21, 14
    vals = [[-1, 0, d - 1, d] for d in (X, Y, Z, B)]
    c = np.array([[x, y, z, b] for x in vals[0] for y in vals[1] for z in vals[2] for b in vals[3]], np.int64)
    c = c[np.random.RandomState(12).permutation(c.shape[0])]
    n, n_cells = c.shape[0], B * Z * X * Y
    kept = ((c >= 0) & (c < np.array([X, Y, Z, B]))).all(1)
    assert kept.sum() == 16
    cell = LU.cell_ids(c[:, :3], kept, c[:, 3], (X, Y, Z))
    more = np.floor(hashfill.uniform("lk_coords", (500, 4), -0.1, 1.1, 74).double().numpy() * np.array([X, Y, Z, B])).astype(np.int64)
    kept2 = ((more >= 0) & (more < np.array([X, Y, Z, B]))).all(1)
    assert 50 < kept2.sum() < 450
    c, cell = np.concatenate([c, more]), np.concatenate([cell, LU.cell_ids(more[:, :3], kept2, more[:, 3], (X, Y, Z))])
    n = c.shape[0]
    obuf, order, sbuf, start, ws = _index_buffers(n, n_cells)
    c_d = _dev(c, np.int32)
    assert L.sf_lift_index_coords_fwd(ptr(c_d), n, B, Z, X, Y, ptr(order), ptr(start), ptr(ws), ws.numel() * 4, st) == 0
    torch.cuda.synchronize()
    assert _canaries_intact(obuf, -7) and _canaries_intact(sbuf, -7)
    _check_index(order.cpu().numpy().astype(np.int64), start.cpu().numpy().astype(np.int64), n, n_cells, cell)


# ---- c. the rig quantiser against float64 ---------------------------------------------------------------------------------------------------
def _run_index_rig(r, A=None):
    L, ptr, st = _api()
    n, n_cells = r["n_points"], r["n_cells"]
    obuf, order, sbuf, start, ws = _index_buffers(n, n_cells)
    a_d, us, vs, ds = (_dev(v, np.float32) for v in (r["A"] if A is None else A, r["us"], r["vs"], r["ds"]))
    lo, res, dim = _grid_args(r["lo"], r["res"], r["dim"])
    assert L.sf_lift_index_rig_fwd(ptr(a_d), ptr(us), ptr(vs), ptr(ds), r["s"], r["n"], r["D"], r["fH"], r["fW"], lo, res, dim, ptr(order),
                                   ptr(start), ptr(ws), ws.numel() * 4, st) == 0
    torch.cuda.synchronize()
    assert _canaries_intact(obuf, -7) and _canaries_intact(sbuf, -7)
    return order, start


def _check_rig_cells(r, order, start):
    """CSR invariants; clear points in their float64 cell (frame part included), the others in a cell within +-margin of q64"""
    n, n_cells = r["n_points"], r["n_cells"]
    o, s = order.cpu().numpy().astype(np.int64), start.cpu().numpy().astype(np.int64)
    LU.csr_invariants(o, s, n, n_cells, int(s[-1]))
    cell = LU.cells_from_csr(o, s, n)
    clear = r["clear"]
    bad = np.nonzero(clear & (cell != r["cell64"]))[0]
    assert bad.size == 0, "%d clear points off their float64 cell, first %s: got %s, want %s" % (bad.size, bad[:4], cell[bad[:4]], r["cell64"][bad[:4]])
    reach = LU.reachable_cells(r["q"][~clear], r["frame"][~clear], r["dim"], r["margin"])
    assert (reach == cell[~clear, None]).any(1).all()
    return o, s, cell


def test_index_rig_against_float64():
    r = LU.rig_case(LU.RIG_SMALL)
    print(LU.rig_conditions(r))
    assert len({r["s"], r["n"], r["D"], r["fH"], r["fW"]}) == 5 and r["dim"] == (24, 20, 1)
    _check_rig_cells(r, *_run_index_rig(r))


# ---- d. the fused chain at a crowded frustum ------------------------------------------------------------------------------------------------
DISCOUNT = 0.7          # not a power of two: prev * discount rounds


@functools.lru_cache(maxsize=None)
def _crowded():
    r = LU.rig_case(LU.RIG_CROWDED)
    found = LU.rig_conditions(r)
    print(found)
    assert found["fullest_cell"] >= 129 and found["cells_17_64"] >= 1 and r["n_points"] == 48384 and r["D"] == 48
    return r


@pytest.mark.parametrize("C", [20, 64])
def test_fused_chain_at_a_crowded_frustum(C):
    """depth_softmax_kernel<48>, the rig index and the fused pooling called directly on 3 frames x 2 cameras x 48 x 28 x 6 points over 16 x 16
    cells (fullest cell 656 points): cells against float64, sums against pool_oracle on the kernel's own lists, mass per frame, and
    LiftSplat.lift_splat on the same inputs bit for bit (frame offsets into the table, prev chain)."""
    L, ptr, st = _api()
    r = _crowded()
    s, n, Dd, fH, fW = r["s"], r["n"], r["D"], r["fH"], r["fW"]
    fHW, rows, XY = fH * fW, s * n, r["dim"][0] * r["dim"][1]
    feat = hashfill.normal("lk_cfeat_%d" % C, (1, s, n, C, fH, fW), 75)
    logits = hashfill.normal("lk_clogits", (1, s, n, Dd, fH, fW), 76, std=2.0)

    # the three kernels called directly
    lg_d = logits.reshape(rows, Dd, fHW).cuda()
    prob_d = torch.empty_like(lg_d)
    assert L.sf_depth_softmax_fwd(ptr(lg_d), ptr(prob_d), rows, Dd, fHW, st) == 0
    order_d, start_d = _run_index_rig(r)
    o, cs, cell = _check_rig_cells(r, order_d, start_d)
    assert np.diff(cs).max() >= 129
    rays = feat.permute(0, 1, 2, 4, 5, 3).reshape(rows * fHW, C).contiguous()
    rays_d = rays.cuda()
    buf, out = _guarded(s * XY * C)
    buf1, out1 = _guarded(s * XY * C)
    out, out1 = out.view(s, XY, C), out1.view(s, XY, C)
    for f in range(s):
        args = (ptr(rays_d), ptr(prob_d), Dd, fHW, ptr(order_d), ptr(start_d[f * XY:]), XY, C)
        assert L.sf_lift_pool_fused_fwd(*args, ptr(out[f - 1]) if f else None, DISCOUNT, ptr(out[f]), st) == 0
        assert L.sf_lift_pool_fused_fwd(*args, None, 1.0, ptr(out1[f]), st) == 0                  # the frame alone
    torch.cuda.synchronize()
    assert _canaries_intact(buf) and _canaries_intact(buf1)
    prob = prob_d.cpu().numpy()
    got, got1 = out.cpu().numpy(), out1.cpu().numpy()

    prev = None
    for f in range(s):
        kw = dict(depth=prob.reshape(-1), feat=rays.numpy(), D=Dd, fHW=fHW)
        want1, s64, sab, length = LU.pool_oracle(o, cs[f * XY:], XY, C, **kw)
        prev = LU.pool_oracle(o, cs[f * XY:], XY, C, prev=prev, discount=DISCOUNT, **kw)[0]
        for name, g, w in (("alone", got1[f], want1), ("blended", got[f], prev)):
            bad = np.nonzero((g.view(np.int32) != w.view(np.int32)).any(1))[0]
            assert bad.size == 0, "frame %d %s: cells %s (lengths %s) differ" % (f, name, bad[:8].tolist(), length[bad[:8]].tolist())
        # mass: what the frame's pooling holds is what its kept points carry — summed per channel in float64, no index decode
        keep = np.zeros((rows * Dd * fHW,), bool)
        keep[o[cs[f * XY]:cs[(f + 1) * XY]]] = True
        assert keep.sum() == length.sum() and keep.reshape(s, -1)[np.arange(s) != f].sum() == 0
        mass = np.einsum("rdh,rhc->c", prob.astype(np.float64) * keep.reshape(rows, Dd, fHW), rays.numpy().astype(np.float64).reshape(rows, fHW, C))
        bound = ((length[:, None] + 2) * LU.U * sab).sum(0)
        assert (np.abs(got1[f].astype(np.float64).sum(0) - mass) <= bound + 1e-12 * sab.sum(0)).all()
        assert np.abs(mass).min() > 0

    # the module on the same inputs: frame offsets into the table and the prev chain of LiftSplat.lift_splat
    from streamingflow_amd.models.lift_splat import LiftSplat
    c = LU.RIG_CROWDED
    m = LiftSplat(c["xb"], c["yb"], c["zb"], c["d_bound"], c["final_dim"], c["down"], DISCOUNT).cuda()
    intr, extr, ego = r["intr"].cuda(), r["extr"].cuda(), r["ego"].cuda()
    aff = m.rig_affines(intr, extr, ego).view(rows, 12).cpu().numpy()
    print("module affines vs lift_util.compose_affines: max-abs %.3e, %d of %d entries differ in bits"
          % (np.abs(aff.astype(np.float64) - r["A"]).max(), int((aff.view(np.int32) != r["A"].view(np.int32)).sum()), aff.size))
    assert LU.same_bits(aff, r["A"])
    bev = m.lift_splat(feat.cuda(), logits.cuda(), intr, extr, ego, nhwc=True)
    assert tuple(bev.shape) == (1, s, r["dim"][0], r["dim"][1], C)
    assert LU.same_bits(bev.cpu().numpy().reshape(s, XY, C), got)
