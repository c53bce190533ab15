"""PanopticMetric.update (N4) with the scoring on the device (max_instances) against the host path (max_instances=None, the code of
the commits before the device path, unchanged) in the same process: [B, T, 200, 200] instance-id maps with 30 vehicles per sample,
(B, T) = (1, 7), (1, 43), (8, 7), (32, 7); a batch holds a different scene (seed) per sample.

A scene: 9 x 5 boxes that drift, ground-truth ids 1..30; the prediction is the box moved by up to one pixel, under another id from
some frame on for every fifth vehicle (an id switch), missing now and then, plus a few boxes without ground truth.

Wall clock of the whole update with a torch.cuda.synchronize() on each side (the host path's copies in the middle of the call are what
the device path removes), median and minimum of 30 calls after 5 warm-ups (tools/instbench.py: wall_ms).  Each size is timed in this
order: host path, device path with max_instances = 40, device path with max_instances = 255 (the largest table), host path again — the
difference of the two host medians is the run-to-run spread the device figures are read against.  The counters of the three metrics
are compared bit for bit at every size.  One JSON object.
Usage: python3 tools/pqbench.py [--out profiles/pqbench.json]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from instbench import REPS, WARMUP, wall_ms  # noqa: E402

SIZES = ((1, 7), (1, 43), (8, 7), (32, 7))
BOUNDS = (40, 255)
COUNTERS = ("iou", "true_positive", "false_positive", "false_negative")


def scene(T, seed, h=200, w=200, n_obj=30):
    """(pred, gt) [1, T, h, w] int64."""
    rng = np.random.RandomState(seed)
    pred, gt = np.zeros((1, T, h, w), dtype=np.int64), np.zeros((1, T, h, w), dtype=np.int64)
    pos = np.stack([rng.rand(n_obj) * (h - 60) + 30, rng.rand(n_obj) * (w - 60) + 30], 1)
    vel = (rng.rand(n_obj, 2) - 0.5) * 0.8
    for k in range(n_obj):
        switch_at = rng.randint(1, max(T, 2)) if k % 5 == 0 else T
        for t in range(T):
            r, c = (pos[k] + vel[k] * t).round().astype(int)
            gt[0, t, r - 4:r + 5, c - 2:c + 3] = k + 1
            if rng.rand() < 0.1:
                continue
            dr, dc = rng.randint(-1, 2, size=2)
            pred[0, t, r - 4 + dr:r + 5 + dr, c - 2 + dc:c + 3 + dc] = k + 1 if t < switch_at else n_obj + 1 + k // 5
    for t in range(T):
        for s in range(3):
            if rng.rand() < 0.5:
                pred[0, t, 4:9, 6 + 8 * s:9 + 8 * s] = n_obj + 7 + s
    return pred, gt


def batch(B, T):
    parts = [scene(T, seed=5 + b) for b in range(B)]
    return tuple(torch.from_numpy(np.concatenate([p[i] for p in parts])).cuda() for i in (0, 1))


def run():
    from streamingflow_amd.metrics import PanopticMetric
    out = {"workload": "PanopticMetric.update on [B, T, 200, 200] int64 id maps, 30 vehicles per sample, a different seed per sample",
           "device": torch.cuda.get_device_name(0),
           "method": f"wall clock between torch.cuda.synchronize() calls around the whole update, median (and minimum) of {REPS} after {WARMUP} "
                     "warm-ups, ms per call",
           "host_path": "max_instances=None: three maxima and every per-frame histogram copied to the host, numpy per frame; timed first and "
                        "again last",
           "device_path": "max_instances=M: int64 conversion, sf_confusion_frames_fwd, sf_panoptic_score_fwd (two launches), nothing read back; "
                          "M = 40 and M = 255",
           "sizes": {}}
    for B, T in SIZES:
        pred, gt = batch(B, T)
        metrics = {"host": PanopticMetric(2).cuda(), **{f"device_M{M}": PanopticMetric(2, max_instances=M).cuda() for M in BOUNDS}}
        for m in metrics.values():
            m.update(pred, gt)
        row = {"B": B, "T": T, "ids": int(max(pred.max(), gt.max())), "thing_true_positives": float(metrics["host"].true_positive[1]),
               "id_switches_and_unmatched": float(metrics["host"].false_negative[1])}
        row["counters_bitwise_equal"] = all(bool(torch.equal(getattr(metrics["host"], k), getattr(m, k))) for m in metrics.values() for k in COUNTERS)
        call = lambda m: (lambda arg: m.update(*arg))
        row["host_ms"], row["host_min_ms"] = wall_ms(call(metrics["host"]), (pred, gt))
        for M in BOUNDS:
            row[f"device_M{M}_ms"], row[f"device_M{M}_min_ms"] = wall_ms(call(metrics[f"device_M{M}"]), (pred, gt))
        row["host_again_ms"], row["host_again_min_ms"] = wall_ms(call(metrics["host"]), (pred, gt))
        row["host_spread_ms"] = abs(row["host_again_ms"] - row["host_ms"])
        for M in BOUNDS:
            metrics[f"device_M{M}"].compute()      # raises if an update was flagged
            row[f"speedup_M{M}"] = min(row["host_ms"], row["host_again_ms"]) / row[f"device_M{M}_ms"]
        out["sizes"][f"{B}x{T}"] = row
    out["counters_bitwise_equal_at_every_size"] = all(v["counters_bitwise_equal"] for v in out["sizes"].values())
    out["device_not_faster_at"] = [f"{k} M={M}" for k, v in out["sizes"].items() for M in BOUNDS
                                   if v[f"device_M{M}_ms"] >= min(v["host_ms"], v["host_again_ms"]) - v["host_spread_ms"]]
    return out


if __name__ == "__main__":
    res = run()
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
