"""The LiDAR branch (voxelise -> SparseEncoder -> BEV) three ways on K = 3 shipped-size clouds (350 000 points each, shipped grid and
channel widths): (1) the synchronising ``extract_lidar_features`` (host reads of every count), (2) the static form
(``static_lidar = True``: capacities fixed in advance, inactive rows, no host read) called eagerly, (3) the static form replayed from a
graph.  One process, same weights and clouds (tools/voxelbench.cloud); per form the GPU time between device events, the wall time per
call including the final synchronisation, and the host time until the call returns (medians over --reps after --warmup).  Also the true
site counts against the default capacities and the share of 64-row tiles that hold inactive rows only.  Prints one JSON line; --out
writes it to a file.

    python tools/lidarstaticbench.py --reps 20 --warmup 3 --out profiles/lidar_static_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--clouds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import voxelbench
    from workloads import hashfill
    from streamingflow_amd.models.streamingflow import default_cfg, streamingflow
    from streamingflow_amd.voxelize import voxelize, voxelize_static

    net = streamingflow(default_cfg()).eval()
    sd = net.state_dict()
    pb = "encoders.lidar.backbone."
    sd.update(hashfill.fill_state_dict({k: v for k, v in sd.items() if k.startswith(pb)}, seed=92, gain=1.6))
    net.load_state_dict(sd)
    net = net.cuda()
    K = a.clouds
    buf = torch.stack([voxelbench.cloud(seed=10 + k) for k in range(K)]).cuda()
    views = [buf[k] for k in range(K)]
    backbone, vox = net.encoders["lidar"]["backbone"], net.encoders["lidar"]["voxelize"]

    def timed(fn, n):
        gpu, wall, host = [], [], []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            t1 = time.perf_counter()
            e1.synchronize()
            t2 = time.perf_counter()
            gpu.append(e0.elapsed_time(e1))
            wall.append((t2 - t0) * 1e3)
            host.append((t1 - t0) * 1e3)
        med = lambda v: round(statistics.median(v), 3)
        return {"gpu_ms": med(gpu), "gpu_min_ms": round(min(gpu), 3), "wall_ms": med(wall), "host_ms": med(host)}

    def measure(fn):
        timed(fn, a.warmup)
        return timed(fn, a.reps)

    res = {"workload": "%d clouds of 350 000 points, shipped grid 1600 x 1600 x 41 and widths, max_voxels %d per cloud" % (K, vox.max_voxels[1]),
           "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip}
    net.static_lidar = False
    want = net.extract_lidar_features(views).clone()
    res["synchronising"] = measure(lambda: net.extract_lidar_features(views))

    # capacities: the counts of these clouds (index kernels of the synchronising path) with 10 % head-room.  The clouds of voxelbench are
    # scattered Gaussians, not surfaces: their sites GROW under the first stride-2 convolutions, past the default capacities
    rows = K * int(vox.max_voxels[1])
    _, c, _ = voxelize(views, vox, True)
    c, shape, seen = c.int().contiguous(), list(backbone.sparse_shape), []
    for conv in backbone.strided_convs():
        c, shape = backbone._out_sites(c, K, shape, conv.kernel_size, conv.stride, conv.padding)
        c = c.contiguous()
        seen.append(c.shape[0])
    caps = [n + n // 10 for n in seen]
    res["default_capacities"] = [rows] + backbone.default_capacities(rows, K)
    net.lidar_capacities = caps
    net.static_lidar = True
    got = net.extract_lidar_features(views).clone()
    counts = backbone.check_static(net.lidar_site_counts, caps)
    res["max_abs_static_vs_synchronising"] = float((got - want).abs().max())
    res["site_counts"] = counts
    res["capacities"] = [rows] + caps
    # 64-row tiles without an active row: stage 0 from the coordinates (holes behind every cloud's block), later stages hold their
    # sites as a prefix
    _, coords, _ = voxelize_static(views, vox)
    act = coords[:, 0] >= 0
    pad = (-rows) % 64
    act = torch.cat([act, act.new_zeros(pad)]) if pad else act
    dead = [int((~act.view(-1, 64).any(1)).sum())]
    tiles = [(rows + 63) // 64]
    for cnt, cap in zip(counts[1:], caps):
        tiles.append((cap + 63) // 64)
        dead.append(tiles[-1] - (min(cnt, cap) + 63) // 64)
    res["tiles"] = tiles
    res["dead_tiles"] = dead
    res["dead_tile_share"] = [round(d / t, 4) for d, t in zip(dead, tiles)]
    res["static_eager"] = measure(lambda: net.extract_lidar_features(views))

    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = net.extract_lidar_features(views)
    g.replay()
    torch.cuda.synchronize()
    res["replay_equals_eager"] = bool(torch.equal(out, got))
    res["static_replayed"] = measure(g.replay)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
