"""GPU: the static form of the LiDAR branch — row buffers of fixed capacity with INACTIVE rows (batch < 0), counts on the device, no
host read, so the branch can be recorded into a graph (include/sfnative.h, "static form of the index entry points";
voxelize.voxelize_static, SparseEncoder.forward_static / check_static, streamingflow.static_lidar).  References: the numpy
restatements of oracle/sparse_encoder_ref.py on the compact sites, and the synchronising product path."""
import numpy as np
import pytest
import torch

import lidar_static_util as LU
from oracle import sparse_encoder_ref as SR
from util import cases, hashfill, maxabs

pytestmark = pytest.mark.gpu

K3, S2, P1, ONE3, ZERO3 = [3, 3, 3], [2, 2, 2], [1, 1, 1], [1, 1, 1], [0, 0, 0]


def _build(tag):
    from streamingflow_amd.models.sparse_encoder import SparseEncoder
    cfg = cases.sparse_cfg(tag)
    m = SparseEncoder(cfg["in_channels"], cfg["sparse_shape"], base_channels=cfg["base_channels"], output_channels=cfg["output_channels"],
                      encoder_channels=cfg["encoder_channels"], encoder_paddings=cfg["encoder_paddings"],
                      block_type=cfg.get("block_type", "basicblock")).eval()
    sd = cases.sparse_state_dict(tag)
    m.load_state_dict(sd)
    return m.cuda(), sd, cfg


def _sites(tag, last_cell=False):
    f, c, B = cases.sparse_inputs(tag)
    f, c = f.numpy(), c.numpy().astype(np.int32)
    if last_cell:      # the largest key of the grid: one below the sentinel's neighbourhood, must be found and must feed its output site
        X, Y, Z = cases.sparse_cfg(tag)["sparse_shape"]
        last = np.array([[B - 1, X - 1, Y - 1, Z - 1]], np.int32)
        assert not (c == last).all(1).any()
        c, f = np.concatenate([c, last]), np.concatenate([f, f[:1] + 1.0])
    return f, c, B


def _roomy(m, B):
    """capacities nothing can exceed: the cells of every stage's grid.  (The hashed sites of oracle.cases are scattered: a stride-2
    convolution gives them more output sites than they are, so the default capacities — made for surfaces — do not fit them.)"""
    return m.default_capacities(1 << 30, B)


def _exact_counts(m, fd, cd, B):
    _, counts = m.forward_static(fd, cd, B, capacities=_roomy(m, B))
    return m.check_static(counts, _roomy(m, B))


# ---- test 1: index kernels, exact -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,layout,last_cell", [("grid32x24x27", "holes", False), ("thin_c8", "holes", False), ("grid32x24x27", "dense", False),
                                                  ("thin_c8", "dense", False), ("grid32x24x27", "holes", True)])
def test_index_kernels_exact(tag, layout, last_cell):
    _, c, B = _sites(tag, last_cell)
    shape = cases.sparse_cfg(tag)["sparse_shape"]
    n = c.shape[0]
    cap, pos = LU.holes(n) if layout == "holes" else LU.dense_rows(n)
    rows, _ = LU.spread(c, None, cap, pos)
    active = rows[:, 0] >= 0
    if layout == "holes":
        assert pos[0] % 64 and (pos[99] + 1) % 64 and cap % 64 and not active[192:512].any()
    else:
        assert active.all()

    def check_table(rc, tab, words, guard_rows, guard_words, rows_out, want):
        assert rc == 0
        live = rows_out[:, 0] >= 0
        assert np.array_equal(LU.compact_table(tab[live], pos), want)
        assert (tab[~live] == -1).all()
        assert (guard_rows == LU.FILL).all() and (guard_words == (LU.FILL & 0xFFFFFFFF)).all()
        ref = LU.tile_words(tab)
        dead = ref == 0
        assert np.array_equal(words[~dead], ref[~dead])
        assert all(bin(int(w)).count("1") == 1 for w in words[dead])
        return int(dead.sum())

    # submanifold table over the buffer
    dead = check_table(*LU.table_static(rows, rows, B, shape, K3, ONE3, ZERO3, True), rows,
                       SR.neighbour_table(c, shape, c, K3, ONE3, ZERO3, True))
    assert dead >= (5 if layout == "holes" else 0)
    # output sites of a strided convolution: the oracle's, then inactive rows up to capacity; the guard keeps its fill
    wc, _ = SR.down_sites(c, shape, K3, S2, P1)
    true = wc.shape[0]
    cap_out = true if layout == "dense" else true + 150
    rc, cnt, out = LU.out_sites_static(rows, B, shape, K3, S2, P1, cap_out)
    assert rc == 0 and cnt == true
    assert np.array_equal(out[:true], wc) and (out[true:cap_out] == -1).all() and (out[cap_out:] == LU.FILL).all()
    if last_cell:
        oshape = SR.out_shape(shape, K3, S2, P1)
        assert wc[-1].tolist() == [B - 1] + [v - 1 for v in oshape]
    # strided table: inactive rows on both sides
    rc, tab, words, g0, g1 = LU.table_static(rows, out[:cap_out], B, shape, K3, S2, P1, False)
    check_table(rc, tab, words, g0, g1, out[:cap_out], SR.neighbour_table(c, shape, wc, K3, S2, P1, False))
    if last_cell:      # the last cell is read by its output site through the centre-most tap that reaches it
        assert (LU.compact_table(tab[true - 1:true], pos) == n - 1).any()


# ---- test 2: overflow ------------------------------------------------------------------------------------------------------------------------
def test_overflow_is_counted_not_written():
    tag = "grid32x24x27"
    m, _, cfg = _build(tag)
    f, c, B = _sites(tag)
    shape = cfg["sparse_shape"]
    cap, pos = LU.holes(c.shape[0])
    rows, feats = LU.spread(c, f, cap, pos)
    true = SR.down_sites(c, shape, K3, S2, P1)[0].shape[0]
    fd, cd = torch.from_numpy(feats).cuda(), torch.from_numpy(rows).cuda()
    exact = _exact_counts(m, fd, cd, B)[1:]
    assert exact[0] == true
    for c0 in (true - 1, 1):
        rc, cnt, out = LU.out_sites_static(rows, B, shape, K3, S2, P1, c0)
        assert rc == 0 and cnt == true and (out[:c0, 0] >= 0).all() and (out[c0:] == LU.FILL).all()
        caps = [c0] + exact[1:]
        dense, counts = m.forward_static(fd, cd, B, capacities=caps)
        assert torch.isfinite(dense).all()
        assert int(counts[1]) == true and int(counts[0]) == c.shape[0]
        with pytest.raises(RuntimeError, match=r"strided convolution 1 .*%d output sites, capacity %d" % (true, c0)):
            m.check_static(counts, caps)
    dense, counts = m.forward_static(fd, cd, B, capacities=exact)
    assert m.check_static(counts, exact) == [c.shape[0]] + exact


# ---- test 3: empty input ---------------------------------------------------------------------------------------------------------------------
def test_empty_input():
    tag = "grid32x24x27"
    m, _, cfg = _build(tag)
    f, c, B = _sites(tag)
    assert B == 2
    # A: every row inactive
    rows = np.tile(LU.INACTIVE, (200, 1))
    dense, counts = m.forward_static(torch.full((200, f.shape[1]), 2.5, device="cuda"), torch.from_numpy(rows).cuda(), B)
    assert dense.shape[0] == B and not dense.any() and not counts.any()
    # B: sample 1 is empty; sample 0 as from a one-sample call over the same buffer with the same capacities
    keep = c[:, 0] == 0
    f0, c0 = f[keep], c[keep]
    cap, pos = LU.holes(c0.shape[0])
    rows, feats = LU.spread(c0, f0, cap, pos)
    fd, cd = torch.from_numpy(feats).cuda(), torch.from_numpy(rows).cuda()
    caps = [v + 70 for v in _exact_counts(m, fd, cd, 1)[1:]]
    two, n2 = m.forward_static(fd, cd, 2, capacities=caps)
    one, n1 = m.forward_static(fd, cd, 1, capacities=caps)
    assert not two[1].any() and one.any()
    assert torch.equal(two[0], one[0]) and torch.equal(n1, n2)


# ---- test 4: encoder values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["grid32x24x27", "thin_c8", "conv_module"])
def test_encoder_values(tag):
    m, sd, cfg = _build(tag)
    f, c, B = _sites(tag)
    n = c.shape[0]
    cap, pos = LU.holes(n)
    rows, feats = LU.spread(c, f, cap, pos)
    want = SR.sparse_encoder_forward(sd, f, c, B, cfg)
    plain = m(torch.from_numpy(f).cuda(), torch.from_numpy(c).cuda(), B)
    fd, cd = torch.from_numpy(feats).cuda(), torch.from_numpy(rows).cuda()
    exact = _exact_counts(m, fd, cd, B)
    caps = [v + 70 for v in exact[1:]]          # dead rows behind every stage's sites too
    got, counts = m.forward_static(fd, cd, B, capacities=caps)
    assert counts.tolist() == exact
    err = maxabs(got, want)
    print(tag, "holes: max-abs to the oracle", err, "to forward", maxabs(got, plain), "site counts", counts.tolist())
    assert err <= 1e-4
    assert torch.equal(got != 0, plain != 0)
    nh, _ = m.forward_static(fd, cd, B, capacities=caps, nhwc=True)
    assert torch.equal(nh.permute(0, 3, 1, 2).contiguous(), got)
    # no holes, capacities = the exact counts: the launches have the sizes of forward's, so the result is forward's
    assert exact[0] == n
    same, counts2 = m.forward_static(torch.from_numpy(f).cuda(), torch.from_numpy(c).cuda(), B, capacities=exact[1:])
    assert counts2.tolist() == exact
    assert torch.equal(same, plain)


def test_encoder_values_crop96():
    """6 000 sites: row counts at which the planner's split choice can differ between capacity and count."""
    tag = "crop96_shipped_widths"
    m, sd, cfg = _build(tag)
    f, c, B = _sites(tag)
    cap, pos = LU.holes(c.shape[0])
    rows, feats = LU.spread(c, f, cap, pos)
    want = SR.sparse_encoder_forward(sd, f, c, B, cfg)
    plain = m(torch.from_numpy(f).cuda(), torch.from_numpy(c).cuda(), B)
    fd, cd = torch.from_numpy(feats).cuda(), torch.from_numpy(rows).cuda()
    caps = [v + 70 for v in _exact_counts(m, fd, cd, B)[1:]]
    got, counts = m.forward_static(fd, cd, B, capacities=caps)
    m.check_static(counts, caps)
    err = maxabs(got, want)
    print(tag, "max-abs to the oracle", err, "largest difference to forward", maxabs(got, plain), "site counts", counts.tolist())
    assert err <= 1e-4
    assert torch.equal(got != 0, plain != 0)


# ---- test 5: voxelize_static against voxelize() ----------------------------------------------------------------------------------------------
def _voxel_clouds():
    import voxel_util as VU
    full = VU.case("descending:2xV")          # reaches max_voxels exactly
    p0, vs, rng, mp, V = full
    assert VU.occupied(p0, vs, rng) == V
    p1 = VU.case("all_outside")[0]            # count 0
    p2 = VU.case("block_edges:255")[0][:40]
    p2 = np.concatenate([p2, np.zeros((20, p2.shape[1]), np.float32)])      # zero rows as the dataset pads: the origin voxel is real
    return [p0, p1, p2], vs, rng, mp, V


@pytest.mark.parametrize("form", ["list", "tensor"])
def test_voxelize_static_matches_voxelize(form):
    from streamingflow_amd.voxelize import Voxelization, voxelize, voxelize_static
    clouds, vs, rng, mp, V = _voxel_clouds()
    if form == "tensor":      # one [K, N, F] tensor: every cloud zero-padded to the longest (then no cloud is empty)
        N = max(p.shape[0] for p in clouds)
        clouds = [np.concatenate([p, np.zeros((N - p.shape[0], p.shape[1]), np.float32)]) for p in clouds]
    vox = Voxelization(voxel_size=list(vs), point_cloud_range=list(rng), max_num_points=mp, max_voxels=(V, V)).eval()
    dev = [torch.from_numpy(p).cuda() for p in clouds]
    wf, wc, _ = voxelize(dev, vox, True)
    per = [int((wc[:, 0] == k).sum()) for k in range(3)]
    assert per[0] == V and len(set(per)) == 3 and (per[1] == 0 or form == "tensor")
    F = clouds[0].shape[1]
    for pad_to in (None, 8):
        feats, coords, counts = voxelize_static(torch.stack(dev) if form == "tensor" else dev, vox, pad_to=pad_to)
        assert feats.shape == (3 * V, pad_to or F) and coords.shape == (3 * V, 4) and coords.dtype == torch.int32
        assert counts.dtype == torch.int32 and counts.tolist() == per
        start = 0
        for k, m in enumerate(per):
            blk = slice(k * V, k * V + m)
            assert torch.equal(coords[blk], wc[start:start + m].to(torch.int32)) and bool((coords[blk, 0] == k).all())
            assert torch.equal(feats[blk, :F], wf[start:start + m])
            assert bool((coords[k * V + m:(k + 1) * V] == -1).all()) and not feats[k * V + m:(k + 1) * V].any()
            start += m
        assert not feats[:, F:].any()


# ---- tests 6 and 7: capture and replay -------------------------------------------------------------------------------------------------------
def _small_model(camera=True, n_future=None):
    from test_gpu_end_to_end import small_cfg
    from streamingflow_amd.models.streamingflow import streamingflow
    cfg, lidar = small_cfg()
    cfg.MODEL.MODALITY.USE_CAMERA = camera
    if n_future is not None:
        cfg.N_FUTURE_FRAMES = n_future
    net = streamingflow(cfg).eval()
    sd = hashfill.fill_state_dict(net.state_dict(), seed=91, gain=0.9)
    pb = "encoders.lidar.backbone."
    sd.update(hashfill.fill_state_dict({k: v for k, v in net.state_dict().items() if k.startswith(pb)}, seed=92, gain=1.6))
    for k, v in net.state_dict().items():
        if k.startswith(("bev_", "lift.", "frustum")):
            sd[k] = v
    net.load_state_dict(sd)
    return cfg, net.cuda()


def _cloud(name, n, total, scale, centre):
    """n points around `centre`, then rows far outside the range up to `total` (they fill the static buffer and voxelise to nothing)"""
    p = torch.cat([hashfill.uniform(name + "_xyz", (n, 3), -1.0, 1.0, seed=93) * torch.tensor(scale) + torch.tensor(centre),
                   hashfill.uniform(name + "_f", (n, 2), 0.0, 1.0, seed=94)], -1)
    return torch.cat([p, torch.full((total - n, 5), 100.0)])


def test_capture_and_replay_lidar_branch():
    _, net = _small_model()
    net.static_lidar = True
    K, N = 2, 600
    A = torch.stack([_cloud("ls_a%d" % k, 600, N, [3.8, 3.8, 2.5], [0.0, 0.0, -1.0]) for k in range(K)]).cuda()
    Bc = torch.stack([_cloud("ls_b%d" % k, 150, N, [0.8, 0.8, 1.0], [2.5, -2.5, -1.0]) for k in range(K)]).cuda()
    buf = A.clone()
    views = [buf[k] for k in range(K)]
    eager = {}
    for name, cloud in (("A", A), ("B", Bc)):
        buf.copy_(cloud)
        out = net.extract_lidar_features(views)
        eager[name] = (out.clone(), net.lidar_site_counts.clone())
    torch.cuda.synchronize()
    backbone = net.encoders["lidar"]["backbone"]
    nA, nB = (backbone.check_static(eager[k][1], backbone.default_capacities(K * 3000, K)) for k in "AB")
    print("site counts A", nA, "B", nB)
    assert nB[0] * 2 < nA[0] and nB[0] > 0 and not torch.equal(eager["A"][0] != 0, eager["B"][0] != 0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = net.extract_lidar_features(views)
        counts = net.lidar_site_counts
    for name, cloud in (("A", A), ("B", Bc), ("A", A)):
        buf.copy_(cloud)
        out.fill_(-7.0)
        counts.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[name][0]), name
        assert torch.equal(counts, eager[name][1]), name


def test_capture_and_replay_model_lidar_only():
    """LiDAR -> temporal_model_lidar -> decoder (camera off, no future frames): deterministic, so the replayed graph, the eager static
    forward and — within the end-to-end bound — the synchronising forward agree."""
    cfg, net = _small_model(camera=False, n_future=0)
    T, N = cfg.TIME_RECEPTIVE_FIELD, 600
    pts = [_cloud("lsm_%d" % t, 600, N, [3.8, 3.8, 2.5], [0.0, 0.0, -1.0])[None].cuda() for t in range(T)]
    ego = torch.zeros((1, cfg.TIME_RECEPTIVE_FIELD, 6), device="cuda")
    args = (None, None, None, ego, None, None, pts, None, None)
    sync = {k: v.clone() for k, v in net(*args).items() if torch.is_tensor(v)}
    net.static_lidar = True
    eager = {k: v.clone() for k, v in net(*args).items() if torch.is_tensor(v)}
    backbone = net.encoders["lidar"]["backbone"]
    assert eager and backbone.check_static(net.lidar_site_counts, backbone.default_capacities(T * 3000, T))[0] > 0
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = net(*args)
    for v in out.values():
        if torch.is_tensor(v):
            v.fill_(-7.0)
    g.replay()
    torch.cuda.synchronize()
    worst = 0.0
    for k, v in eager.items():
        assert torch.equal(out[k], v), k
        worst = max(worst, maxabs(v, sync[k]))
    print("static against synchronising forward: max-abs", worst)
    assert worst <= 1e-3
    assert float(eager["segmentation"].abs().max()) > 1e-2
