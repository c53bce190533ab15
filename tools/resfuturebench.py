"""The flow-warp kernel alone and one ResFuturePredictionV2 forward, device path against the same object's torch path.

  * ``sf_flow_warp_fwd`` with the fused 2-channel head at 200x200, C = 64, L = 32 (Cf = 96), B = 1 and B = 8: --calls launches between
    two device events, rotating over enough buffer sets that their bytes exceed twice the 256 MiB Infinity Cache (so the figure
    is an HBM figure, not a cache one); median over --reps after --warmup.  Bytes moved = (Cf + 2 C) * 4 * P: feat and the state
    read once, the warped state written once (the taps of neighbouring pixels are expected in L2).  hbm_frac = bytes / time over
    the 8 TB/s roof DESIGN section 5 and bench.py (PEAK_HBM_GBS) use.
  * ``ResFuturePredictionV2(64, 32, n_future=4)`` at 200x200, B = 1: the forward on the device path and, with SF_BEVERSE_TORCH=1,
    on the torch path (torch's own conv2d / grid_sample on the same GPU), same weights, same inputs; the two outputs are compared.
Prints one JSON line; --out writes it to a file.

    python tools/resfuturebench.py --reps 30 --warmup 5 --out profiles/resfuturebench.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_HBM_GBS = 8000.0
CACHE_BYTES = 256 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="kernel launches per timed sample")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: at least 20 repetitions")
    import torch
    from workloads import hashfill
    from streamingflow_amd.beverse import motion_modules as M

    def timed(fn, n):
        out = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
        return out

    C, L, H, W = 64, 32, 200, 200
    Cf = C + L
    res = {"workload": "sf_flow_warp_fwd (fused head) and ResFuturePredictionV2(64, 32, n_future=4), 200x200", "reps": a.reps,
           "warmup": a.warmup, "calls_per_sample": a.calls, "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "hip": torch.version.hip, "peak_hbm_gbs": PEAK_HBM_GBS, "kernel": {}}
    w_off = hashfill.uniform("rb_w", (2, Cf), -1.0, 1.0, 61).cuda() * (3.0 / Cf ** 0.5)
    b_off = torch.zeros(2, device="cuda")
    for B in (1, 8):
        P = B * H * W
        nbytes = (Cf + 2 * C) * 4 * P
        sets = max(2, -(-2 * CACHE_BYTES // nbytes))
        bufs = [(torch.randn((B, H, W, C), device="cuda"), torch.randn((B, H, W, Cf), device="cuda").abs_(),
                 torch.empty((B, H, W, Cf), device="cuda")) for _ in range(sets)]
        turn = [0]

        def launches():
            for _ in range(a.calls):
                state, feat, out = bufs[turn[0] % sets]
                turn[0] += 1
                M.flow_warp_nhwc(state, out, Cf, 0, feat=feat, w_off=w_off, b_off=b_off)

        timed(launches, a.warmup)
        ms = [t / a.calls for t in timed(launches, a.reps)]
        med = statistics.median(ms)
        res["kernel"][f"B{B}"] = {"pixels": P, "buffer_sets": sets, "bytes": nbytes, "ms": round(med, 5), "min_ms": round(min(ms), 5),
                                  "gbs": round(nbytes / (med * 1e-3) / 1e9, 1), "hbm_frac": round(nbytes / (med * 1e-3) / 1e9 / PEAK_HBM_GBS, 4)}
        del bufs

    net = M.ResFuturePredictionV2(C, L, n_future=4)
    net.load_state_dict(hashfill.fill_state_dict(net.state_dict(), seed=2, gain=1.0))
    net = net.eval().cuda()
    sample = hashfill.normal("rf_s", (1, L, H, W), 41).cuda()
    hidden = hashfill.normal("rf_h", (1, C, H, W), 42).cuda()
    fwd = {}
    outs = {}
    for name, env in (("device", None), ("torch", "1")):
        if env is None:
            os.environ.pop("SF_BEVERSE_TORCH", None)
        else:
            os.environ["SF_BEVERSE_TORCH"] = env
        run = lambda: net(sample, hidden)
        timed(run, a.warmup)
        ms = timed(run, a.reps)
        outs[name] = run()
        fwd[name + "_ms"] = round(statistics.median(ms), 3)
        fwd[name + "_min_ms"] = round(min(ms), 3)
    os.environ.pop("SF_BEVERSE_TORCH", None)
    fwd["speedup"] = round(fwd["torch_ms"] / fwd["device_ms"], 3)
    fwd["max_abs_difference"] = float((outs["device"] - outs["torch"]).abs().max())
    res["v2_forward"] = fwd
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
