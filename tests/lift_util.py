"""TEST INFRASTRUCTURE — plain numpy oracles for the kernels of csrc/lift_splat.hip, called one at a time (test_gpu_lift_kernels.py),
and the synthetic inputs of those tests.  Nothing here imports the product; test_lift_util.py pins every function to oracle/lift_splat.py
(itself pinned to the reference's Python), so that a wrong helper cannot agree with a wrong kernel.

Arithmetic contracts restated here (csrc/lift_splat.hip):
  pooling    per (cell, channel): acc = +0; acc = fp32(acc + term) over the cell's list IN LIST ORDER; term = x[p][c] or
             fp32(depth[p] * feat[ray(p)][c]) with ray(p) = (p // (D*fHW))*fHW + p % fHW — product and sum rounded separately, no FMA;
             then, with prev, fp32(fp32(prev * discount) + acc)                                      (streamingflow.py:419)
  quantiser  q = fp32(fp32(g - lo) / res), idx = trunc(q), kept when 0 <= idx < dim on every axis    (streamingflow.py:353-366)
  CSR        stable sort by cell id, dropped points last; cell_start[c] = first list position of cell c, cell_start[n_cells] = kept points
"""
import numpy as np
import torch

from workloads import hashfill

U = 2.0 ** -24          # fp32 unit roundoff
F32 = np.float32


def _np(a, dtype):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a), dtype=dtype)


# ---- pooling ----------------------------------------------------------------------------------------------------------------------
def pool_oracle(order, cell_start, n_cells, C, x=None, depth=None, feat=None, D=None, fHW=None, prev=None, discount=1.0):
    """-> (out fp32 [n_cells, C], sum64 [n_cells, C], sumabs [n_cells, C], length [n_cells]).

    Materialised form (x [n_points, C]) or fused form (depth [n_points], feat [n_rays, C], D, fHW).  ``cell_start`` may be a slice of a
    longer table: entries 0..n_cells are read and index ``order`` as they stand.  ``out`` is the sequential fp32 sum (np.float32 arithmetic
    only), ``sum64`` the float64 sum of the exactly evaluated terms (prev * discount among them), ``sumabs`` the sum of their magnitudes:
    |out - sum64| <= (L + 2) * 2^-24 * sumabs for a cell of L points (one rounding of the product, L additions of which the first is exact,
    one rounding of prev * discount, one of the blend; (L + 2) u covers (1 + u)^(L + 1) - 1 for every L below 2^20)."""
    order = _np(order, np.int64)
    cs = _np(cell_start, np.int64)[:n_cells + 1]
    assert cs.shape[0] == n_cells + 1
    length = np.diff(cs)
    assert (length >= 0).all()
    fused = x is None
    if fused:
        depth, feat = _np(depth, F32), _np(feat, F32).reshape(-1, C)
        DF = int(D) * int(fHW)
    else:
        x = _np(x, F32).reshape(-1, C)
    acc = np.zeros((n_cells, C), F32)
    s64 = np.zeros((n_cells, C), np.float64)
    sab = np.zeros((n_cells, C), np.float64)
    for k in range(int(length.max()) if n_cells else 0):
        live = np.nonzero(length > k)[0]
        p = order[cs[live] + k]
        if fused:
            rows = feat[(p // DF) * fHW + p % fHW]
            term = depth[p][:, None] * rows                                  # fp32 * fp32 -> fp32: rounded once
            t64 = depth[p][:, None].astype(np.float64) * rows.astype(np.float64)
            assert term.dtype == F32
        else:
            term = x[p]
            t64 = term.astype(np.float64)
        acc[live] = acc[live] + term                                         # fp32 + fp32 -> fp32: rounded once
        s64[live] += t64
        sab[live] += np.abs(t64)
    if prev is not None:
        prev = _np(prev, F32).reshape(n_cells, C)
        acc = prev * F32(discount) + acc                                     # two fp32 operations, each rounded
        p64 = prev.astype(np.float64) * np.float64(F32(discount))
        s64 += p64
        sab += np.abs(p64)
    assert acc.dtype == F32
    return acc, s64, sab, length


def same_bits(a, b):
    """fp32 arrays equal bit for bit (tells -0 from +0, unlike ==)."""
    a, b = _np(a, F32), _np(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- quantiser ----------------------------------------------------------------------------------------------------------------------
def quantise_q(geom, lo, res):
    """fp32(fp32(g - lo) / res), [n, 3] fp32 — the reference's expression on the CPU (IEEE subtract and divide)."""
    g, lo, res = _np(geom, F32).reshape(-1, 3), _np(lo, F32), _np(res, F32)
    with np.errstate(all="ignore"):
        q = (g - lo) / res
    assert q.dtype == F32
    return q


def trunc_cells(q, dim):
    """q [n, 3] (any float type) -> (idx int64 [n, 3] — (-1, -1, -1) for a dropped point —, kept bool [n]).  Truncation toward zero;
    kept when 0 <= idx < dim on every axis.  A non-finite q and |q| >= 2^31 are dropped by definition."""
    q = np.asarray(q)
    dim = np.asarray(dim, np.int64)
    fin = np.isfinite(q) & (np.abs(q) < 2.0 ** 31)
    t = np.trunc(np.where(fin, q, -2.0)).astype(np.int64)
    kept = (fin & (t >= 0) & (t < dim)).all(1)
    return np.where(kept[:, None], t, -1), kept


def quantise_oracle(geom, lo, res, dim):
    return trunc_cells(quantise_q(geom, lo, res), dim)


def cell_ids(idx, kept, b, dim):
    """(x, y, z) int64 [n, 3], batch element [n] -> cell id ((b*Z + z)*X + x)*Y + y, -1 for dropped points."""
    X, Y, Z = (int(v) for v in dim)
    cid = ((np.asarray(b, np.int64) * Z + idx[:, 2]) * X + idx[:, 0]) * Y + idx[:, 1]
    return np.where(kept, cid, -1)


# ---- CSR --------------------------------------------------------------------------------------------------------------------------------
def csr_oracle(cell, n_cells):
    """cell [n] int64, -1 = dropped -> (order [n], cell_start [n_cells + 1]).  Stable: ascending point number inside a cell; the dropped
    points follow position cell_start[n_cells], in an order the kernels leave unspecified (compare that tail as a set)."""
    cell = np.asarray(cell, np.int64)
    key = np.where(cell < 0, n_cells, cell)
    order = np.argsort(key, kind="stable")
    start = np.searchsorted(key[order], np.arange(n_cells + 1), side="left")
    return order.astype(np.int64), start.astype(np.int64)


def cells_from_csr(order, cell_start, n):
    """Inverse of a CSR over the whole list: per-point cell id, -1 for the tail behind cell_start[-1]."""
    order, cs = _np(order, np.int64), _np(cell_start, np.int64)
    counts = np.diff(cs)
    assert cs[0] == 0 and (counts >= 0).all() and cs[-1] <= n
    cell = np.full((n,), -1, np.int64)
    cell[order[:cs[-1]]] = np.repeat(np.arange(cs.shape[0] - 1), counts)
    return cell


def csr_invariants(order, cell_start, n, n_cells, n_kept):
    """order is a permutation of 0..n-1, ascending inside every cell; cell_start non-decreasing with n_cells + 1 entries ending at n_kept."""
    order, cs = _np(order, np.int64), _np(cell_start, np.int64)
    assert order.shape == (n,) and cs.shape == (n_cells + 1,)
    assert np.array_equal(np.sort(order), np.arange(n))
    assert cs[0] == 0 and (np.diff(cs) >= 0).all() and cs[-1] == n_kept
    inner = np.ones((n,), bool)                 # positions whose predecessor lies in the same cell
    inner[cs[cs < n]] = False
    inner[cs[-1]:] = False
    assert (np.diff(order)[inner[1:]] > 0).all()


# ---- synthetic camera rig -------------------------------------------------------------------------------------------------------------------
def _euler2mat64(a):
    """utils/geometry.py:124-155 in float64: Rx(x) @ Ry(y) @ Rz(z)."""
    x, y, z = (float(v) for v in a)
    cz, sz, cy, sy, cx, sx = np.cos(z), np.sin(z), np.cos(y), np.sin(y), np.cos(x), np.sin(x)
    zm = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    ym = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    xm = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    return xm @ ym @ zm


def rig_cameras(n_frames, n_cam, final_dim, seed):
    """One sample of ``n_frames`` frames: intrinsics [1, s, n, 3, 3], extrinsics [1, s, n, 4, 4], future_egomotion [1, s, 6], fp32 torch.
    Cameras yawed evenly round the ego vehicle (a few degrees of per-frame jitter: every frame and camera has its own affine), lever arm
    about 1.5 m along the viewing direction, f about 0.9 W, ego motion within 0.6 m and 0.06 rad per frame."""
    s, n = n_frames, n_cam
    H, W = final_dim
    tag = "liftk_rig_%d_%d_" % (s, n)
    f = 0.9 * W * (1.0 + 0.05 * hashfill.uniform(tag + "f", (s, n), -1.0, 1.0, seed).double().numpy())
    yaw = 2.0 * np.pi * np.arange(n)[None, :] / n + hashfill.uniform(tag + "yaw", (s, n), -0.15, 0.15, seed).double().numpy() + 0.3
    arm = 1.5 + hashfill.uniform(tag + "arm", (s, n), -0.2, 0.2, seed).double().numpy()
    height = hashfill.uniform(tag + "h", (s, n), -0.3, 0.3, seed).double().numpy()
    base = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])      # camera z (depth) -> ego x, camera x -> ego -y, camera y -> ego -z
    intr, extr = np.zeros((1, s, n, 3, 3)), np.zeros((1, s, n, 4, 4))
    for t in range(s):
        for c in range(n):
            intr[0, t, c] = [[f[t, c], 0.0, W / 2.0], [0.0, f[t, c], H / 2.0], [0.0, 0.0, 1.0]]
            extr[0, t, c, :3, :3] = _euler2mat64([0.0, 0.0, yaw[t, c]]) @ base
            extr[0, t, c, :3, 3] = [arm[t, c] * np.cos(yaw[t, c]), arm[t, c] * np.sin(yaw[t, c]), height[t, c]]
            extr[0, t, c, 3, 3] = 1.0
    ego = torch.cat([hashfill.uniform(tag + "ego_t", (1, s, 3), -0.6, 0.6, seed), hashfill.uniform(tag + "ego_r", (1, s, 3), -0.06, 0.06, seed)], -1)
    return torch.from_numpy(intr).float(), torch.from_numpy(extr).float(), ego


def compose_affines(intr, extr, ego):
    """[R_cam K^-1 | t_cam] (streamingflow.py:277-292) followed by the cumulative ego-motion warps of :386-396 (frames 0..t moved by pose t,
    t = 0..s-2), composed in float64 from the fp32 inputs and rounded once -> [s*n, 12] fp32."""
    intr, extr, ego = _np(intr, np.float64)[0], _np(extr, np.float64)[0], _np(ego, np.float64)[0]
    s, n = intr.shape[:2]
    A = np.zeros((s, n, 4, 4))
    for t in range(s):
        for c in range(n):
            A[t, c, :3, :3] = extr[t, c, :3, :3] @ np.linalg.inv(intr[t, c])
            A[t, c, :3, 3] = extr[t, c, :3, 3]
            A[t, c, 3, 3] = 1.0
    for t in range(s - 1):
        P = np.eye(4)
        P[:3, :3], P[:3, 3] = _euler2mat64(ego[t, 3:]), ego[t, :3]
        A[:t + 1] = P @ A[:t + 1]
    return np.ascontiguousarray(A[:, :, :3, :].reshape(s * n, 12), F32)


def frustum_axes(d_bound, final_dim, down):
    """us [fW], vs [fH], ds [D] fp32 as LiftSplat.lift_splat takes them from create_frustum (streamingflow.py:149-168)."""
    H, W = final_dim
    us = torch.linspace(0, W - 1, W // down, dtype=torch.float)
    vs = torch.linspace(0, H - 1, H // down, dtype=torch.float)
    ds = torch.arange(*d_bound, dtype=torch.float)
    return us.numpy().copy(), vs.numpy().copy(), ds.numpy().copy()


def rig(n_frames, n_cam, d_bound, final_dim, down, seed):
    """-> (affines [n_frames*n_cam, 12] fp32, us, vs, ds)."""
    return (compose_affines(*rig_cameras(n_frames, n_cam, final_dim, seed)),) + frustum_axes(d_bound, final_dim, down)


def rig_q64(A, us, vs, ds, lo, res):
    """The fp32 affines and vectors evaluated in float64 at every frustum point p = ((t*D + d)*fH + h)*fW + w, t = frame*n_cam + cam:
    -> (q [n, 3] float64 cell coordinates, bound [n, 3]).  bound = 8 * 2^-24 * (|a0||px| + |a1||py| + |a2||d| + |a3| + |lo|) / res covers
    the kernel's six roundings (px or py, three fused multiply-adds, the subtraction of lo, the division), each relative to a partial
    result no larger than that sum."""
    A, us, vs, ds = _np(A, np.float64).reshape(-1, 3, 4), _np(us, np.float64), _np(vs, np.float64), _np(ds, np.float64)
    lo, res = _np(lo, F32).astype(np.float64), _np(res, F32).astype(np.float64)
    T, D, fH, fW = A.shape[0], ds.shape[0], vs.shape[0], us.shape[0]
    d = np.broadcast_to(ds[:, None, None], (D, fH, fW))
    pts = np.stack([us[None, None, :] * d, vs[None, :, None] * d, d, np.ones_like(d)], -1).reshape(-1, 4)       # [D*fH*fW, 4]
    g = np.einsum("tij,pj->tpi", A, pts).reshape(-1, 3)
    mag = np.einsum("tij,pj->tpi", np.abs(A), np.abs(pts)).reshape(-1, 3)
    return (g - lo) / res, 8.0 * U * (mag + np.abs(lo)) / res


def frame_cells64(q, frame, dim):
    """float64 q [n, 3], frame [n] -> cell id with the frame part, -1 outside (same truncation rule as the quantiser)."""
    idx, kept = trunc_cells(q, dim)
    return cell_ids(idx, kept, frame, dim)


def reachable_cells(q, frame, dim, margin):
    """[n, 8] cell ids (or -1) of q moved by +-margin on each axis."""
    out = []
    for sx in (-margin, margin):
        for sy in (-margin, margin):
            for sz in (-margin, margin):
                out.append(frame_cells64(q + np.array([sx, sy, sz]), frame, dim))
    return np.stack(out, 1)


def clear_points(q, margin):
    """q lies more than ``margin`` cells from an integer on every axis."""
    return (np.abs(q - np.round(q)) > margin).all(1)


# ---- cell-edge point sets of the quantiser test ---------------------------------------------------------------------------------------------
EDGE_GRID = dict(dim=(21, 14, 3), lo=(-3.15, -0.7, -1.25), res=(0.3, 0.1, 0.5), n_batch=2)      # res not all powers of two
DYADIC_GRID = dict(dim=(5, 7, 3), lo=(-1.5, -0.75, -1.25), res=(0.5, 0.25, 0.5), n_batch=2)     # every boundary an exact fp32 quotient


def edge_points(grid):
    """[n, 3] fp32, n even: for every axis and k = -2..dim+1 the boundary fp32(lo + k res) and its two fp32 neighbours, three points with
    q in (-1, 0), and -0.0, NaN, +-Inf, +-1e30 on that axis — the other two axes at mid-cell values that change from point to point —,
    in a fixed shuffle so that both batch halves hold every kind, padded with mid-cell points."""
    dim, lo, res = grid["dim"], np.array(grid["lo"], F32), np.array(grid["res"], F32)
    lo64, res64 = lo.astype(np.float64), res.astype(np.float64)
    pts = []

    def mid(i):
        return [F32(lo64[a] + ((i * (3 + 2 * a) + a) % dim[a] + 0.5) * res64[a]) for a in range(3)]

    def add(a, v):
        p = mid(len(pts))
        p[a] = F32(v)
        pts.append(p)

    for a in range(3):
        for k in range(-2, dim[a] + 2):
            v = F32(lo64[a] + k * res64[a])
            for w in (np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf))):
                add(a, w)
        for f in (0.25, 0.5, 0.96875):
            add(a, lo64[a] - f * res64[a])
        for v in (-0.0, np.nan, np.inf, -np.inf, 1e30, -1e30):
            add(a, v)
    pts = np.array(pts, F32)
    pts = pts[np.random.RandomState(20).permutation(pts.shape[0])]
    while pts.shape[0] % grid["n_batch"]:
        pts = np.concatenate([pts, np.array([mid(pts.shape[0])], F32)])
    return pts


def edge_conditions(grid, pts, dyadic):
    """What the point set must contain for the test to mean anything, from CPU arithmetic alone -> dict of the counts found."""
    dim, lo, res = np.array(grid["dim"]), np.array(grid["lo"], F32), np.array(grid["res"], F32)
    q = quantise_q(pts, lo, res)
    idx, kept = trunc_cells(q, dim)
    found = {}
    for a in range(3):
        found["in_-1_0_axis%d" % a] = int(((q[:, a] > -1) & (q[:, a] < 0)).sum())
        found["eq_-1_axis%d" % a] = int((q[:, a] == -1).sum())
        found["eq_dim_axis%d" % a] = int((q[:, a] == dim[a]).sum())
        assert found["in_-1_0_axis%d" % a] >= 3 and found["eq_dim_axis%d" % a] >= 1
        # q == -1 exactly needs fp32(g - lo) == res: g - lo is a multiple of ulp(lo), which 0.3f and 0.1f are not.  There the set
        # holds the nearest quotients on either side of -1 instead; on dyadic grids (and the z axis here) -1 itself.
        assert found["eq_-1_axis%d" % a] >= 1 or (not dyadic and a < 2)
        near = q[(q[:, a] > -1.5) & (q[:, a] < -0.5), a].astype(np.float64)
        assert near[near <= -1].max() >= -1 - 1e-5 and near[near > -1].min() <= -1 + 1e-5

    def axis_cells(qq):         # per axis: the truncated index, -1 where that axis alone drops the point
        return np.stack([trunc_cells(np.stack([qq[:, a]] * 3, 1), [dim[a]] * 3)[0][:, 0] for a in range(3)], 1)

    if not dyadic:
        with np.errstate(all="ignore"):
            rcp = (F32(1.0) / res).astype(F32)
            q_rcp = ((pts - lo) * rcp).astype(F32)
            q_64 = (pts.astype(np.float64) - lo.astype(np.float64)) / res.astype(np.float64)
        for name, alt in (("reciprocal", q_rcp), ("float64", q_64)):
            idx2, kept2 = trunc_cells(alt, dim)
            found[name] = int(((idx2 != idx).any(1) | (kept2 != kept)).sum())
            found[name + "_per_axis"] = [int(v) for v in (axis_cells(alt) != axis_cells(q)).sum(0)]
            assert found[name] >= 1, name
    return found


# ---- the two rig cases (shared by the CPU conditions and the GPU tests) ---------------------------------------------------------------------
# frames, cameras, D_BOUND, final_dim, downsample, X / Y / Z_BOUND, seed.  RIG_SMALL: 2 frames, 3 cameras, D = 13, fH = 5, fW = 7 (five
# different counts), 24 cells of 1.0 m by 20 of 1.5 m.  RIG_CROWDED: 3 frames, 2 cameras, D = 48, fH = 28, fW = 6 = 48 384 points on 16 x 16
# cells of 6.25 m: whole image columns share a cell, as at the shipped size.
RIG_SMALL = dict(s=2, n=3, d_bound=(2.0, 28.0, 2.0), final_dim=(40, 56), down=8, xb=(-12.0, 12.0, 1.0), yb=(-15.0, 15.0, 1.5),
                 zb=(-10.0, 10.0, 20.0), seed=3)
RIG_CROWDED = dict(s=3, n=2, d_bound=(2.0, 50.0, 1.0), final_dim=(224, 48), down=8, xb=(-50.0, 50.0, 6.25), yb=(-50.0, 50.0, 6.25),
                   zb=(-10.0, 10.0, 20.0), seed=5)


def rig_case(case):
    """Everything both test files derive from a case on the CPU: the rig, the grid as the library takes it, the float64 cells."""
    from oracle import cases, lift_splat as LS
    r = dict(case)
    res, start, dim = LS.calculate_birds_eye_view_parameters(list(case["xb"]), list(case["yb"]), list(case["zb"]))
    r["lo"], r["res"], r["dim"] = (start - res / 2.0).numpy().astype(F32), res.numpy().astype(F32), tuple(int(v) for v in dim)
    r["intr"], r["extr"], r["ego"] = rig_cameras(case["s"], case["n"], case["final_dim"], case["seed"])
    r["A"] = compose_affines(r["intr"], r["extr"], r["ego"])
    r["us"], r["vs"], r["ds"] = frustum_axes(case["d_bound"], case["final_dim"], case["down"])
    r["D"], r["fH"], r["fW"] = r["ds"].shape[0], r["vs"].shape[0], r["us"].shape[0]
    r["n_points"] = case["s"] * case["n"] * r["D"] * r["fH"] * r["fW"]
    r["n_cells"] = case["s"] * r["dim"][0] * r["dim"][1] * r["dim"][2]
    r["margin"] = cases.LIFT_MARGIN / 4
    q, bound = rig_q64(r["A"], r["us"], r["vs"], r["ds"], r["lo"], r["res"])
    r["q"], r["bound"] = q, bound
    r["frame"] = np.arange(r["n_points"]) // (case["n"] * r["D"] * r["fH"] * r["fW"])
    r["cell64"] = frame_cells64(q, r["frame"], r["dim"])
    r["clear"] = clear_points(q, r["margin"])
    return r


def rig_conditions(r):
    """Asserted from the float64 reference alone -> dict of the values found."""
    found = dict(max_bound=float(r["bound"].max()), ambiguous_share=float(1.0 - r["clear"].mean()),
                 inside_share=float((r["cell64"] >= 0).mean()))
    assert r["margin"] > found["max_bound"], found                           # fp32 rounding cannot move a clear point to another cell
    assert found["ambiguous_share"] <= 0.01, found
    assert 0.30 <= found["inside_share"] <= 0.70, found
    A = r["A"].reshape(r["s"], r["n"], 12)
    assert len({a.tobytes() for a in A.reshape(-1, 12)}) == r["s"] * r["n"]   # a different affine per frame and camera
    counts = np.bincount(r["cell64"][r["clear"] & (r["cell64"] >= 0)], minlength=r["n_cells"])
    found["fullest_cell"] = int(counts.max())
    found["cells_129_up"] = int((counts >= 129).sum())
    found["cells_17_64"] = int(((counts >= 17) & (counts <= 64)).sum())
    found["cells_1_16"] = int(((counts >= 1) & (counts <= 16)).sum())
    return found
