"""Instance tracking (N4) on the device against the host matching it replaces: predict_instance_segmentation_and_trajectories on
B samples of T frames of 200 x 200 with 30 objects each, (B, T) = (1, 7), (1, 43), (8, 7), (32, 7); a batch holds a different scene
(seed) per sample.

Wall clock with a torch.cuda.synchronize() on each side (the host round trip in the middle of a call is what the device path
removes), median and minimum of 30 calls after 5 warm-ups (tools/instbench.py: wall_ms).  Each size is timed in this order:
  parent_commit   (only with --parent FILE) the function of the parent commit: FILE is that commit's streamingflow_amd/instance.py
                  (``git show <parent>:streamingflow_amd/instance.py > FILE``), loaded beside the new module in the same process and on
                  the same library; timed TWICE (before and after the others), the difference of the two medians is the run-to-run
                  spread the new figures are read against;
  device          the functions as they are now (sf_instance_track_fwd), once per launch shape of the assign kernel: SF_TRACK_WAVES=1
                  (one wavefront per frame pair) and SF_TRACK_WAVES=4, alternating, each twice, then the default once more;
  host            the new code with SF_TRACK_HOST=1.
One JSON object, with whether the ids equal the parent's at every size.
Usage: python3 tools/trackbench.py [--parent FILE] [--out profiles/trackbench.json]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from instbench import REPS, WARMUP, load_parent, scene, wall_ms  # noqa: E402

SIZES = ((1, 7), (1, 43), (8, 7), (32, 7))
SHAPES = ("1", "4")      # SF_TRACK_WAVES
DEFAULT_SHAPE = "1"      # what csrc/instance_track.hip launches when SF_TRACK_WAVES is unset


def batch(B, T):
    parts = [scene(T, seed=5 + b) for b in range(B)]
    return {k: torch.cat([p[k] for p in parts]).cuda() for k in parts[0]}


def with_env(fn, **env):
    def call(arg):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            return fn(arg)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return call


def run(parent_path=None):
    from streamingflow_amd import instance as I
    parent = load_parent(parent_path) if parent_path else None
    for k in ("SF_TRACK_HOST", "SF_TRACK_WAVES"):
        os.environ.pop(k, None)
    out = {"workload": "predict_instance_segmentation_and_trajectories, B samples of T frames of 200x200, 30 objects each, a different seed per sample",
           "device": torch.cuda.get_device_name(0),
           "method": f"wall clock between torch.cuda.synchronize() calls, median (and minimum) of {REPS} after {WARMUP} warm-ups, ms per call",
           "parent_commit": ("the function of the parent commit's instance.py (--parent), loaded beside the new module; timed first and again last"
                             if parent else "not timed (no --parent file given)"),
           "device_path": "sequence kernels, moments, sf_instance_track_fwd, one gather: nothing read back; per SF_TRACK_WAVES launch shape",
           "host_path": "the new code with SF_TRACK_HOST=1: one host copy of the moments, scipy per sample and frame pair, one upload",
           "sizes": {}}
    fn = I.predict_instance_segmentation_and_trajectories
    for B, T in SIZES:
        o = batch(B, T)
        row = {"B": B, "T": T}
        got = {w: with_env(fn, SF_TRACK_WAVES=w)(o) for w in SHAPES}
        host = with_env(fn, SF_TRACK_HOST="1")(o)
        row["ids"] = int(host.max())
        row["device_ids_equal_host_path"] = all(bool(torch.equal(g, host)) for g in got.values())
        if parent:
            row["same_ids_as_parent_commit"] = all(bool(torch.equal(parent.predict_instance_segmentation_and_trajectories(o), g)) for g in got.values())
            row["parent_commit_ms"], row["parent_commit_min_ms"] = wall_ms(parent.predict_instance_segmentation_and_trajectories, o)
        for again in ("", "_again"):      # the two shapes alternate, each timed twice: a gap between them is read against a shape's own repeat
            for w in SHAPES:
                row[f"device_waves{w}{again}_ms"], row[f"device_waves{w}{again}_min_ms"] = wall_ms(with_env(fn, SF_TRACK_WAVES=w), o)
        row["device_default_ms"], row["device_default_min_ms"] = wall_ms(fn, o)
        row["host_path_ms"], row["host_path_min_ms"] = wall_ms(with_env(fn, SF_TRACK_HOST="1"), o)
        if parent:
            row["parent_commit_again_ms"], row["parent_commit_again_min_ms"] = wall_ms(parent.predict_instance_segmentation_and_trajectories, o)
            row["parent_commit_spread_ms"] = abs(row["parent_commit_again_ms"] - row["parent_commit_ms"])
            row["device_default_minus_parent_ms"] = row["device_default_ms"] - min(row["parent_commit_ms"], row["parent_commit_again_ms"])
            row["speedup_over_parent_commit"] = min(row["parent_commit_ms"], row["parent_commit_again_ms"]) / row["device_default_ms"]
        out["sizes"][f"{B}x{T}"] = row
    if parent:
        out["same_ids_as_parent_commit_at_every_size"] = all(v["same_ids_as_parent_commit"] for v in out["sizes"].values())
        out["device_slower_than_parent_beyond_spread"] = [k for k, v in out["sizes"].items()
                                                          if v["device_default_minus_parent_ms"] > v["parent_commit_spread_ms"]]

    def mean(v, w):
        return 0.5 * (v[f"device_waves{w}_ms"] + v[f"device_waves{w}_again_ms"])
    first = out["sizes"]["1x7"]
    out["launch_shape_mean_ms"] = {k: {w: mean(v, w) for w in SHAPES} for k, v in out["sizes"].items()}
    out["faster_launch_shape_at_1x7"] = min(SHAPES, key=lambda w: mean(first, w))
    out["launch_shape_gap_at_1x7_ms"] = abs(mean(first, SHAPES[0]) - mean(first, SHAPES[1]))
    out["same_shape_repeat_gap_at_1x7_ms"] = max(abs(first[f"device_waves{w}_ms"] - first[f"device_waves{w}_again_ms"]) for w in SHAPES)
    out["launch_shape_faster_at"] = {k: min(SHAPES, key=lambda w: mean(v, w)) for k, v in out["sizes"].items()}
    out["default_launch_shape"] = DEFAULT_SHAPE
    return out


if __name__ == "__main__":
    res = run(sys.argv[sys.argv.index("--parent") + 1] if "--parent" in sys.argv else None)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
