"""Instance post-processing (N4) on long target sets: predict_instance_segmentation_and_trajectories on B*T = 7 and 43 frames
of 200 x 200 with about 30 objects, the sequence path against the per-frame path it replaced.

Wall clock with a torch.cuda.synchronize() on each side (host round trips are what the sequence path removes), median of 30
calls after 5 warm-ups.  Three forms of the call are timed, in this order:
  parent_commit  (only with --parent FILE) the function of the commit before the sequence kernels: FILE is that commit's
                 streamingflow_amd/instance.py (``git show <parent>:streamingflow_amd/instance.py > FILE``), loaded beside the new
                 module in the same process and on the same library.  The sequence path is judged against THIS figure;
  per_frame      the same path rebuilt here from the unchanged single-frame functions (available without the parent's file);
  sequence       the functions as they are now (regular and short-interval).
One JSON object.
Usage: python3 tools/instbench.py [--parent FILE] [--out profiles/instbench.json]"""
import importlib.util
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS, WARMUP = 30, 5


def scene(frames, h=200, w=200, n_obj=30, seed=5):
    """An eval_scene-like decoder output of one sample: Gaussian centre heat maps of moving boxes, offsets pointing at the centres,
    a constant flow per object."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float), torch.arange(w, dtype=torch.float), indexing="ij")
    seg, center = torch.zeros(1, frames, 2, h, w), torch.zeros(1, frames, 1, h, w)
    offset, flow = torch.zeros(1, frames, 2, h, w), torch.zeros(1, frames, 2, h, w)
    pos = torch.stack([torch.rand(n_obj, generator=g) * (h - 40) + 20, torch.rand(n_obj, generator=g) * (w - 40) + 20], 1)
    vel = (torch.rand(n_obj, 2, generator=g) - 0.5) * 0.8
    for t in range(frames):
        fg = torch.zeros(h, w, dtype=torch.bool)
        for k in range(n_obj):
            cy, cx = pos[k] + vel[k] * t
            m = ((yy - cy).abs() <= 4.5) & ((xx - cx).abs() <= 2.5)
            fg |= m
            center[0, t, 0] = torch.maximum(center[0, t, 0], torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 12.0))
            offset[0, t, 0][m] = (cy.round() - yy)[m]
            offset[0, t, 1][m] = (cx.round() - xx)[m]
            flow[0, t, 0][m] = vel[k, 0]
            flow[0, t, 1][m] = vel[k, 1]
        seg[0, t, 1][fg] = 4.0
        seg[0, t, 0][~fg] = 4.0
    noise = torch.randn(center.shape, generator=g) * 0.01
    return {"segmentation": seg, "instance_center": (center + noise).clamp(0, 1), "instance_offset": offset, "instance_flow": flow}


def per_frame(output):
    """predict_instance_segmentation_and_trajectories before the sequence kernels."""
    from streamingflow_amd import instance as I
    vehicles = output["segmentation"].detach().argmax(dim=2) == 1
    B, T = vehicles.shape[:2]
    centre_maps, offsets = output["instance_center"].detach(), output["instance_offset"].detach()
    maps = torch.stack([torch.stack([I.get_instance_segmentation_and_centers(centre_maps[b, t], offsets[b, t], vehicles[b, t])[0][0]
                                     for t in range(T)]) for b in range(B)])
    flow = output["instance_flow"].detach()
    return torch.cat([I.make_instance_id_temporally_consistent(maps[b:b + 1], flow[b:b + 1]) for b in range(B)])


def wall_ms(fn, arg):
    for _ in range(WARMUP):
        fn(arg)
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(arg)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def load_parent(path):
    """The parent commit's instance.py as a module of the package (its relative imports resolve to this tree's _lib / runtime)."""
    import streamingflow_amd  # noqa: F401
    spec = importlib.util.spec_from_file_location("streamingflow_amd._parent_instance", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def run(parent_path=None):
    from streamingflow_amd import instance as I
    parent = load_parent(parent_path) if parent_path else None
    out = {"workload": "predict_instance_segmentation_and_trajectories, 1 sample of T frames of 200x200, 30 objects",
           "device": torch.cuda.get_device_name(0),
           "method": f"wall clock between torch.cuda.synchronize() calls, median of {REPS} after {WARMUP} warm-ups, ms per call",
           "parent_commit": ("the function of the parent commit's instance.py (--parent), loaded beside the new module, timed first"
                             if parent else "not timed (no --parent file given)"),
           "per_frame": "the per-frame path rebuilt from the unchanged single-frame functions: per-frame centres / grouping / unique, per-sample matching",
           "sequence": "sf_instance_seq_fwd on all frames, one moments launch and host copy, one gather", "sizes": {}}
    for frames in (7, 43):
        o = {k: v.cuda() for k, v in scene(frames).items()}
        a, b = per_frame(o), I.predict_instance_segmentation_and_trajectories(o)
        s = I.predict_instance_segmentation_and_trajectories_short_interval(o)
        row = {}
        if parent:
            row["same_ids_as_parent_commit"] = bool(torch.equal(parent.predict_instance_segmentation_and_trajectories(o), b))
            row["parent_commit_ms"], row["parent_commit_min_ms"] = wall_ms(parent.predict_instance_segmentation_and_trajectories, o)
        old, old_min = wall_ms(per_frame, o)
        new, new_min = wall_ms(I.predict_instance_segmentation_and_trajectories, o)
        short, short_min = wall_ms(I.predict_instance_segmentation_and_trajectories_short_interval, o)
        row.update({"per_frame_ms": old, "per_frame_min_ms": old_min, "sequence_ms": new, "sequence_min_ms": new_min,
                    "short_interval_ms": short, "short_interval_min_ms": short_min, "same_ids_as_per_frame": bool(torch.equal(a, b)),
                    "ids": int(b.max()), "short_interval_ids": int(s.max())})
        row["speedup_over_per_frame"] = old / new
        if parent:
            row["speedup_over_parent_commit"] = row["parent_commit_ms"] / new
        out["sizes"][str(frames)] = row
    against = "parent_commit_ms" if parent else "per_frame_ms"
    out["sequence_not_slower_than"] = against
    out["sequence_not_slower"] = all(v["sequence_ms"] <= v[against] for v in out["sizes"].values())
    out["decision"] = ("both predict_* functions use the sequence path" if out["sequence_not_slower"] else
                       "the sequence path is slower at some size: predict_instance_segmentation_and_trajectories has to stay on the per-frame path")
    return out


if __name__ == "__main__":
    res = run(sys.argv[sys.argv.index("--parent") + 1] if "--parent" in sys.argv else None)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
