"""Ground-truth label kernels (N4) at data-loader size: instance_labels on B = 1 and B = 8 sequences of T = 7 frames of 200 x 200
with 30 moving boxes (instance ids 1..30) and small random ego-motions.

Wall clock with a torch.cuda.synchronize() on each side, median of 30 calls after 5 warm-ups (as tools/instbench.py).  Nothing
is compared: there was no device implementation before this one, and the reference's function is a CPU loop that is not
available where this runs.  Its two figures below were measured once with the reference function itself on the CPU of a
DIFFERENT machine and are only recorded next to the device times; no ratio is asserted.
One JSON object.
Usage: python3 tools/labelbench.py [--out profiles/labelbench.json]"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS, WARMUP = 30, 5
H = W = 200
T, N_OBJ = 7, 30
EXTENT = (50.0, 50.0)
REFERENCE_CPU_MS = {"64x64, T=7, 6 objects": 150.0, "200x200, T=7, 30 objects": 371.0}


def scene(batch, seed=5):
    """instance [batch, T, H, W] int64 (9 x 5 boxes drifting at up to 0.4 pixels per frame), future_egomotion [batch, T, 6]."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float), torch.arange(W, dtype=torch.float), indexing="ij")
    inst = torch.zeros(batch, T, H, W, dtype=torch.long)
    for b in range(batch):
        pos = torch.stack([torch.rand(N_OBJ, generator=g) * (H - 40) + 20, torch.rand(N_OBJ, generator=g) * (W - 40) + 20], 1)
        vel = (torch.rand(N_OBJ, 2, generator=g) - 0.5) * 0.8
        for t in range(T):
            for k in range(N_OBJ):
                cy, cx = pos[k] + vel[k] * t
                inst[b, t][((yy - cy).abs() <= 4.5) & ((xx - cx).abs() <= 2.5)] = k + 1
    ego = torch.cat([(torch.rand((batch, T, 3), generator=g) - 0.5) * torch.tensor([6.0, 4.0, 0.0]),
                     (torch.rand((batch, T, 3), generator=g) - 0.5) * torch.tensor([0.0, 0.0, 0.12])], -1)
    return inst, ego


def wall_ms(fn):
    for _ in range(WARMUP):
        fn()
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def run():
    from streamingflow_amd import labels as LB
    out = {"workload": f"instance_labels, B sequences of T = {T} frames of {H}x{W}, {N_OBJ} objects, num_instances = {N_OBJ}",
           "device": torch.cuda.get_device_name(0),
           "method": f"wall clock between torch.cuda.synchronize() calls, median of {REPS} after {WARMUP} warm-ups, ms per call "
                     "(pose inversion and sampling matrices in torch, one memset, two launches)",
           "reference_cpu_ms_per_sample": REFERENCE_CPU_MS,
           "reference_cpu_note": "the reference's convert_instance_mask_to_center_and_offset_label on the CPU of a different machine; "
                                 "recorded for scale only, not measured in this run and not compared",
           "sizes": {}}
    for batch in (1, 8):
        inst, ego = scene(batch)
        inst, ego = inst.cuda(), ego.cuda()

        def call():
            return LB.instance_labels(inst, ego, N_OBJ, spatial_extent=EXTENT)

        c, o, f = call()
        med, low = wall_ms(call)
        out["sizes"][str(batch)] = {"ms": med, "min_ms": low, "ms_per_sample": med / batch,
                                    "pixels_with_offset": int((o[:, :, 0] != 255).sum()), "pixels_with_flow": int((f[:, :, 0] != 255).sum()),
                                    "centerness_max": float(c.max())}
    return out


if __name__ == "__main__":
    res = run()
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
