"""The planner (N5) at the shipped size: Planning.forward on B = 1 and B = 8 samples of N = 600 trajectories, T = 4 waypoints, a
200 x 200 grid, a [64, 28, 60] front-camera map and a 256-wide GRU state (the scenes of tools/gen_planning_golden.py at that size).

Wall clock with a torch.cuda.synchronize() on each side, median of 30 calls after 5 warm-ups, for the device path and for the
module's own plain-torch path (SF_PLAN_TORCH=1) on the same device, and the number of kernel launches of one call of each as
torch.profiler counts them.  Nothing is asserted and no ratio is a claim: there was no planner before this one to compare with, and
the torch path is this project's own code (written for CPU tests, not for speed), not the reference's.
One JSON object.
Usage: python3 tools/planbench.py [--out profiles/planbench.json]"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
REPS, WARMUP = 30, 5
N, T, G, S = 600, 4, 200, 256


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


def launches(fn):
    """Kernel launches of one call, or the reason they could not be counted."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    except Exception as ex:       # recorded, not hidden
        return "not counted: %r" % (ex,)


def run():
    import gen_planning_golden as GEN
    from streamingflow_amd.models.planning import Planning
    out = {"workload": f"Planning.forward, B samples of N = {N} trajectories, T = {T}, grid {G}x{G}, cam_front [B, 64, 28, 60], GRU state {S}",
           "device": torch.cuda.get_device_name(0),
           "method": f"wall clock between torch.cuda.synchronize() calls, median of {REPS} after {WARMUP} warm-ups, ms per call; launches of one "
                     "call counted by torch.profiler",
           "note": "no ratio is asserted or claimed: no planner existed before this one, and the torch path is this project's own plain-torch "
                   "statement of the semantics (written for the CPU tests), not the reference's code",
           "sizes": {}}
    for batch in (1, 8):
        spec = dict(G=G, B=batch, N=N, T=T, hd=4, occ=torch.bool, commands=(["LEFT", "FORWARD", "RIGHT"] * 3)[:batch], zero_target=False,
                    cam=(64, 28, 60), S=S, loud=False)
        sc = GEN.scene("bench", spec)
        net = Planning(sc["cfg"], 64, 6, S).eval()
        net.load_state_dict(GEN.weights(net.state_dict()))
        net = net.cuda()
        args = [sc[k].cuda() if isinstance(sc[k], torch.Tensor) else sc[k] for k in
                ("cam_front", "trajs", "gt_trajs", "cost_volume", "semantic_pred", "hd_map", "commands", "target_points")]

        def call():
            return net(*args)[1]

        res = {}
        for name, env in (("device", None), ("torch", "1")):
            if env is None:
                os.environ.pop("SF_PLAN_TORCH", None)
            else:
                os.environ["SF_PLAN_TORCH"] = env
            ref = call()
            med, low = wall_ms(call)
            res[name] = {"ms": med, "min_ms": low, "launches": launches(call), "first_waypoint": ref[0, 0, :2].tolist()}
        os.environ.pop("SF_PLAN_TORCH", None)
        out["sizes"][str(batch)] = res
    return out


if __name__ == "__main__":
    res = run()
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
