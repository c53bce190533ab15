"""TEST INFRASTRUCTURE — the edge clouds of the voxelisation tests (test_voxel_oracle.py on the CPU, test_gpu_voxel_kernels.py on the
device; `python -m oracle.gen_golden --only voxel_edges` records the compiled reference on REFERENCE_IDS) and the restatements of the
per-voxel mean.  Nothing here imports the product.  Every cloud is a pure function of its name (workloads.hashfill), has at most 3000
points and aims at one place where csrc/voxelize.hip — key, stable radix sort, run heads, scan, binary search — can go wrong:

  half_cubic, half_flat     (max - min) / size ends in .5: C round() forms 3 cells where round-half-even forms 2
  pow2_64, _256, _4096      the cell count is a power of two: the sentinel key of outside points needs one bit more than any cell
  one_cell, two_cells       the smallest grids: 1 and 2 sort bits
  high_keys                 2048 x 2048 x 1023 cells, the largest class the 32-bit sort accepts: keys above 2^31
  descending:*              arrival order is the reverse of key order; caps at, one below and one above the number of occupied cells
  crowd_one, crowd_two      runs of 3000 / 1500 sorted positions: the run head lies several 256-thread blocks behind its point
  block_edges:n             n = 1, 255, 256, 257 points
  all_outside               no point inside
  nonfinite                 NaN, +inf, -inf on every axis, -0.0 on x, NaN (non-default payload) and inf in feature columns
  wide_rows:F               F = 3 and F = 7 feature columns

case(cid) -> (points float32 [n, F] numpy, voxel_size, coors_range, max_points, max_voxels).
"""
import numpy as np

from oracle import voxelize as VZ
from workloads import hashfill

F32 = np.float32
U = 2.0 ** -24          # fp32 unit roundoff

GRID4 = ((1.0, 1.0, 1.0), (-2.0, -2.0, -2.0, 2.0, 2.0, 2.0))                 # 4^3 cells
NAN_PAYLOAD = 0x7FC12345                                                     # a quiet NaN that is not the default 0x7FC00000

DESCENDING_CAPS = ("1x64", "3x10", "600x1", "2xV-1", "2xV", "2xV+1")
CASE_IDS = (["half_cubic", "half_flat", "pow2_64", "pow2_256", "pow2_4096", "one_cell", "two_cells", "high_keys"]
            + ["descending:" + c for c in DESCENDING_CAPS]
            + ["crowd_one", "crowd_two"] + ["block_edges:%d" % n for n in (1, 255, 256, 257)]
            + ["all_outside", "nonfinite", "wide_rows:3", "wide_rows:7"])
# cubic grids and finite coordinates: what the reference's C++ CPU kernel can be run on (it indexes its [z][y][x] table with (x, y, z),
# and converting NaN / inf to int is undefined in C)
REFERENCE_IDS = ["half_cubic", "pow2_64", "one_cell"] + ["descending:" + c for c in DESCENDING_CAPS] + ["crowd_one", "all_outside"]
MEAN_IDS = ["descending:3x10", "crowd_one", "wide_rows:3", "wide_rows:7"]
# hand-placed coordinates of half_cubic, one of each on every axis (the other two axes at 0.0, inside cell 1).  Cells are
# floor(fp32(fp32(p + 2.5) / 2)), 3 per axis, so [-2.5, 3.5) is inside although the nominal range ends at 2.5:
#   2.5 -> cell 2;  3.0 -> cell 2;  3.5 - 2^-21 -> 5.9999995 / 2 -> cell 2 (the last fp32 that is inside);
#   nextafter(3.5, 0) = 3.5 - 2^-22 -> p + 2.5 is a tie between 5.9999995 and 6.0 and rounds to even, 6.0 -> cell 3, outside;
#   3.5 -> outside;  -2.5000002 = -2.5 - 2^-22 -> -2^-22 / 2 -> floor = -1, outside
HALF_EDGES = np.array([2.5, 3.0, 3.5 - 2.0 ** -21, np.nextafter(F32(3.5), F32(0)), 3.5, -2.5000002], dtype=F32)
HALF_EDGES_INSIDE = [True, True, True, False, False, False]


def _u(name, shape, lo, hi):
    return hashfill.uniform("voxel_edge_" + name, shape, lo, hi, seed=77).numpy()


def _cloud(name, n, F, lo, hi):
    """n points, coordinate a uniform in [lo[a], hi[a]), the other columns uniform in [-1, 1)"""
    p = _u(name + "_feat", (n, F), -1.0, 1.0)
    for a in range(3):
        p[:, a] = _u(name + "_ax%d" % a, (n,), lo[a], hi[a])
    return p


def _shuffle(name, p):
    return p[np.argsort(hashfill.uniform01("voxel_edge_" + name + "_perm", p.shape[0], seed=77), kind="stable")]


def occupied(points, vs, rng):
    """V: the number of occupied cells (the oracle's, without caps)"""
    with np.errstate(invalid="ignore"):
        c, ok = VZ.point_coors(points, vs, rng)
    return len({tuple(r) for r in c[ok].tolist()})


def _pow2_64_points():
    return _cloud("pow2_64", 700, 4, (-2.5,) * 3, (2.5,) * 3)                 # 0.8^3: about half inside


def _descending_points():
    p = _pow2_64_points()
    c = np.floor((p[:, :3] - F32(-2.0)) / F32(1.0))                           # cell of every point, outside ones too
    return p[np.lexsort((-c[:, 0], -c[:, 1], -c[:, 2]))]                      # stable: descending z, then y, then x


def case(cid):
    tag, _, arg = cid.partition(":")
    if tag == "half_cubic":
        p = _cloud(tag, 400, 4, (-3.5,) * 3, (4.5,) * 3)
        for a in range(3):
            rows = slice(a * len(HALF_EDGES), (a + 1) * len(HALF_EDGES))
            p[rows, :3] = 0.0
            p[rows, a] = HALF_EDGES
        return p, (2.0, 2.0, 2.0), (-2.5, -2.5, -2.5, 2.5, 2.5, 2.5), 3, 20
    if tag == "half_flat":                                                    # x: 5 / 2 = 2.5, y: 3 / 1, z: 1.25 / 0.5 = 2.5 -> 3 x 3 x 3
        p = _cloud(tag, 400, 4, (-3.5, -2.0, -1.25), (4.5, 2.0, 1.25))
        return p, (2.0, 1.0, 0.5), (-2.5, -1.5, -0.75, 2.5, 1.5, 0.5), 3, 20
    if tag == "pow2_64":
        return (_pow2_64_points(),) + GRID4 + (3, 40)
    if tag == "pow2_256":                                                     # 8 x 8 x 4
        p = _cloud(tag, 700, 4, (-5.0, -5.0, -2.5), (5.0, 5.0, 2.5))
        return p, (1.0, 1.0, 1.0), (-4.0, -4.0, -2.0, 4.0, 4.0, 2.0), 3, 150
    if tag == "pow2_4096":                                                    # 16^3
        p = _cloud(tag, 700, 4, (-10.0,) * 3, (10.0,) * 3)
        return p, (1.0, 1.0, 1.0), (-8.0, -8.0, -8.0, 8.0, 8.0, 8.0), 3, 300
    if tag == "one_cell":                                                     # (1 / 1.26)^3: half inside
        p = _cloud(tag, 300, 4, (-0.13,) * 3, (1.13,) * 3)
        return p, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0, 1.0, 1.0, 1.0), 7, 1
    if tag == "two_cells":
        p = _cloud(tag, 300, 4, (-0.26, -0.13, -0.13), (2.26, 1.13, 1.13))
        return p, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0, 2.0, 1.0, 1.0), 7, 2
    if tag == "high_keys":                                                    # 2048 * 2048 * 1023 = 4 290 772 992 cells
        hi = _cloud(tag + "_hi", 200, 4, (0.0, 0.0, 512.0), (2048.0, 2048.0, 1023.0))      # keys >= 2^31
        lo = _cloud(tag + "_lo", 80, 4, (0.0, 0.0, 0.0), (2048.0, 2048.0, 512.0))
        last = _cloud(tag + "_last", 5, 4, (2047.0, 2047.0, 1022.0), (2048.0, 2048.0, 1023.0))   # key 4 290 772 991
        out = _cloud(tag + "_out", 15, 4, (0.0, 0.0, 1023.0), (2048.0, 2048.0, 1030.0))
        out[:5, 0] = -out[:5, 0] - 1.0
        out[:5, 2] = 1000.0
        out[5, :3] = (2048.0, 2047.5, 1022.5)
        return _shuffle(tag, np.concatenate([hi, lo, last, out])), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0, 2048.0, 2048.0, 1023.0), 3, 250
    if tag == "descending":
        p = _descending_points()
        V = occupied(p, *GRID4)
        mp, mv = {"1x64": (1, 64), "3x10": (3, 10), "600x1": (600, 1), "2xV-1": (2, V - 1), "2xV": (2, V), "2xV+1": (2, V + 1)}[arg]
        return (p,) + GRID4 + (mp, mv)
    if tag == "crowd_one":                                                    # 3000 points in cell (1, 2, 3); column 3 = point index
        p = _cloud(tag, 3000, 4, (-1.0, 0.0, 1.0), (0.0, 1.0, 2.0))
        p[:, 3] = np.arange(3000, dtype=F32)
        return (p,) + GRID4 + (5, 4)
    if tag == "crowd_two":                                                    # cells (3, 0, 2) and (0, 3, 1), alternating by point parity
        p = _cloud(tag, 3000, 4, (1.0, -2.0, 0.0), (2.0, -1.0, 1.0))
        p[1::2, :3] = _cloud(tag + "_odd", 1500, 3, (-2.0, 1.0, -1.0), (-1.0, 2.0, 0.0))
        p[:, 3] = np.arange(3000, dtype=F32)
        return (p,) + GRID4 + (700, 4)
    if tag == "block_edges":
        p = _cloud(tag, int(arg), 4, (-2.2,) * 3, (2.2,) * 3)
        p[0, :3] = 0.5
        return (p,) + GRID4 + (3, 64)
    if tag == "all_outside":
        p = _cloud(tag, 300, 4, (-2.5,) * 3, (2.5,) * 3)
        far = _u(tag + "_far", (300,), 2.0, 3.0)
        for i in range(300):
            p[i, i % 3] = far[i] if (i // 3) % 2 else -far[i] - F32(1e-3)
        p[0, 0] = 2.0                                                         # the open upper end
        p[1, 1] = np.nextafter(F32(-2.0), F32(-3.0))
        return (p,) + GRID4 + (3, 64)
    if tag == "nonfinite":                                                    # x from 0: -0.0 lies on the lower bound
        p = _cloud(tag, 80, 5, (-0.5, -2.5, -2.5), (4.5, 2.5, 2.5))
        p[:12, :3] = 0.5                                                      # cell (0, 2, 2)
        for a in range(3):
            p[3 * a:3 * a + 3, a] = (np.nan, np.inf, -np.inf)
        p[9, 0] = -0.0                                                        # inside, cell 0
        p.view(np.uint32)[10, 3] = NAN_PAYLOAD                                # inside: the feature is copied, never compared
        p[11, 4] = np.inf
        p[12, 4] = -np.inf
        p[12, :3] = (3.5, -1.5, 1.5)
        return p, (1.0, 1.0, 1.0), (0.0, -2.0, -2.0, 4.0, 2.0, 2.0), 3, 64
    if tag == "wide_rows":
        return (_cloud(cid, 500, int(arg), (-2.5,) * 3, (2.5,) * 3),) + GRID4 + (4, 30)
    raise KeyError(cid)


def expected_padded(points, vs, rng, mp, mv):
    """what the padded entry point must return: (voxel_num, voxels [mv, mp, F], coors [mv, 3], num [mv]) — the oracle's rows, zeros behind"""
    with np.errstate(invalid="ignore"):                                       # NaN / inf coordinates: floor -> int64 of the oracle
        v, c, k = VZ.hard_voxelize(points, vs, rng, mp, mv)
    m = v.shape[0]
    V, C, K = np.zeros((mv, mp, points.shape[1]), F32), np.zeros((mv, 3), np.int32), np.zeros((mv,), np.int32)
    V[:m], C[:m], K[:m] = v, c, k
    return m, V, C, K


def mean_oracles(voxels, num):
    """voxels [M, max_points, F], num [M] (the oracle's) -> (seq32, mean64, bound) [M, F] each.
    seq32: s = +0; s = fp32(s + x_i) over the voxel's first num points in index order; fp32(s / fp32(num)) — np.float32 arithmetic only,
    the order and roundings of vox_assign_kernel (__fadd_rn, __fdiv_rn).
    mean64: the float64 mean.  bound = (num + 1) * 2^-24 * mean(|x_i|): num - 1 rounded additions (the first, to +0, is exact) and one
    rounded division give |seq32 - mean64| <= ((1 + u)^num - 1) * sum|x_i| / num <= (num + 1) u * mean|x_i| for every num below 2^20."""
    v = np.asarray(voxels, F32)
    M, mp, F = v.shape
    s = np.zeros((M, F), F32)
    for q in range(mp):
        live = num > q
        s[live] = s[live] + v[live, q]
    assert s.dtype == F32
    seq32 = s / num.astype(F32)[:, None]
    assert seq32.dtype == F32
    mask = (np.arange(mp)[None, :] < num[:, None])[:, :, None]
    v64 = np.where(mask, v.astype(np.float64), 0.0)
    mean64 = v64.sum(1) / num[:, None]
    bound = (num[:, None] + 1) * U * np.abs(v64).sum(1) / num[:, None]
    return seq32, mean64, bound
