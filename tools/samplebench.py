"""The trajectory sampler (N6) at the shipped size: sf_plan_sample_fwd on B = 1 and B = 8 samples of M = 1800 rows, n_t = 7 kept stamps,
for both launch shapes (SF_PLAN_SAMPLE_LAUNCHES = 1: one workgroup per sample; 2: keys, then rank and rows over (M / 256, B)
workgroups), and, for context, the reference's own ``sample`` + ``[:, ::10]`` + ``.float()`` on the CPU of the machine it is run on.

--device     device time per call: CALLS calls of the entry point alone (fed uniforms, no torch.rand) captured in one graph per launch
             shape, a replay timed between two device events and divided by CALLS (so the host's enqueue rate is not what is measured);
             median and minimum of WINDOWS replays after WARMUP eager calls, the two shapes alternating replay by replay in one process.
             Also the whole ``TrajectorySampler.__call__`` (torch.rand, the frame tensors and the launch), enqueued eagerly back to back
             between two events: that figure includes the host wherever the host is the slower side.
--reference  wall clock of the reference's call (numpy + scipy, float64, one sample), median of 10 after 2; needs the reference tree.
Each mode fills its own section of the JSON file (--out, default profiles/samplebench.json) and keeps the other.  Recorded, not gated:
nothing is asserted and no ratio is a claim (the reference runs on another machine class, and nothing of this existed before)."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
M, N_FUTURE = 1800, 6
CALLS, WINDOWS, WARMUP = 200, 30, 20


def _graph_of(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            for _ in range(CALLS):
                fn()
    torch.cuda.current_stream().wait_stream(side)
    return graph


def _replay_us(graph):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / CALLS


def _window_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / CALLS


def device():
    from streamingflow_amd import sampler as S
    smp = S.TrajectorySampler(N_FUTURE, n_samples=M)
    out = {"device": torch.cuda.get_device_name(0),
           "method": f"entry: {CALLS} calls captured in a graph, one replay between two device events, per call; median / minimum of {WINDOWS} replays "
                     f"after {WARMUP} warm-up calls; launch shapes alternate replay by replay.  sampler_call: {CALLS} eager calls between two events",
           "sizes": {}}
    for B in (1, 8):
        dev = torch.device("cuda")
        gen = torch.Generator(device=dev).manual_seed(B)
        u = torch.rand(B, 5, M, dtype=torch.float64, device=dev, generator=gen)
        v0 = torch.linspace(0.0, 20.0, B, dtype=torch.float64, device=dev)
        kappa = torch.linspace(-0.5, 0.3, B, dtype=torch.float64, device=dev) if B > 1 else torch.tensor([0.3], dtype=torch.float64, device=dev)
        one, zero = torch.ones_like(kappa), torch.zeros_like(kappa)
        t0 = torch.stack([zero, one], dim=1)
        n0 = torch.stack([torch.where(kappa <= 0, one, -one), zero], dim=1)
        tt = smp.tt_kept.to(dev)

        def entry():
            return S.sample_device(v0, kappa, t0, n0, tt, smp.t_key, u, *smp.counts)

        def whole():
            return smp(v0, kappa)

        res, rows = {}, {}
        for shape in ("1", "2"):
            os.environ["SF_PLAN_SAMPLE_LAUNCHES"] = shape
            for _ in range(WARMUP):
                entry()
            rows[shape] = entry()
        same = bool(torch.equal(rows["1"][0], rows["2"][0]) and torch.equal(rows["1"][1], rows["2"][1]))
        graphs = {}
        for shape in ("1", "2"):
            os.environ["SF_PLAN_SAMPLE_LAUNCHES"] = shape      # read when the call is enqueued, that is at capture
            graphs[shape] = _graph_of(entry)
        os.environ.pop("SF_PLAN_SAMPLE_LAUNCHES", None)
        ts = {"1": [], "2": []}
        for shape in ("1", "2"):
            _replay_us(graphs[shape])
        for _ in range(WINDOWS):
            for shape in ("1", "2"):
                ts[shape].append(_replay_us(graphs[shape]))
        for shape in ("1", "2"):
            res[f"entry_us_{shape}_launch"] = {"median": statistics.median(ts[shape]), "min": min(ts[shape])}
        for _ in range(WARMUP):
            whole()
        tw = [_window_us(whole) for _ in range(WINDOWS)]
        res["sampler_call_us_default_shape"] = {"median": statistics.median(tw), "min": min(tw)}
        res["shapes_bitwise_equal"] = same
        out["sizes"][str(B)] = res
    return out


def reference():
    import gen_sampler_golden as GEN
    ref = GEN.reference_sample()
    tt = np.arange(0, N_FUTURE * 0.5 + 0.05, 0.05)
    T0, N0 = np.array([0.0, 1.0]), np.array([-1.0, 0.0])

    def call():
        return torch.from_numpy(ref(4.0, 0.3, T0, N0, tt, M)[:, ::10]).float()

    ts = []
    for i in range(12):
        t = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"what": f"streamingflow/utils/sampler.py sample(M = {M}, {len(tt)} fine stamps) + [:, ::10] + .float(), one sample, numpy + scipy float64",
            "cpu_threads": torch.get_num_threads(), "ms": statistics.median(ts[2:]), "min_ms": min(ts[2:])}


if __name__ == "__main__":
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "samplebench.json")
    res = json.load(open(path)) if os.path.exists(path) else {}
    res["workload"] = f"sf_plan_sample_fwd, B samples of M = {M} rows, n_t = {N_FUTURE + 1} kept stamps"
    res["note"] = "recorded, not gated: no ratio is asserted or claimed"
    if "--device" in sys.argv:
        res["mi355x"] = device()
    if "--reference" in sys.argv:
        res["reference_cpu"] = reference()
    with open(path, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
