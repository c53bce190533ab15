"""EfficientNet-b4 trunk (N8) at the shipped size: 18 images (3 frames x 6 cameras) of 3 x 224 x 480, cut after block 21, endpoints
160 x 14 x 30 and 56 x 28 x 60.  Two forms, alternated round by round in one process, each run timed with device events:

  a  sf_effnet_trunk_fwd (streamingflow_amd/models/efficientnet.py): one call, its own workspace, NHWC endpoints
  b  the plain-torch restatement of tests/effnet_util.py in float32 on the same device (convolutions through MIOpen): the only comparison
     there is — efficientnet_pytorch is not installed

Median of --reps runs (at least 20) after --warmup (at least 3).  Also records the algorithmic bytes — every activation written once and
read once (the image read once, the endpoints written once), plus the weights — and the fraction of the HBM roof they would need the
median time of form a; and the observed errors of form a against the float64 restatement on the GPU tests' trunk cases, with the bounds.
Writes effnet_trunk_bench.json and effnet_trunk_parity.json into profiles/ (or --out DIR) and prints the first.
Usage: python3 tools/trunkbench.py [--reps N] [--warmup N] [--out DIR]"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT_DIR = os.path.join(ROOT, "profiles")
CASES = [("b4", (2, 3, 32, 48), "nominal"), ("b4", (1, 3, 40, 56), "nominal"), ("b0", (2, 3, 32, 32), "nominal"), ("b4", (1, 3, 37, 51), None)]
PEAK_HBM_GBS = 8000.0


def algorithmic_bytes(trunk, n, H, W):
    """Every tensor between two launches written once and read once, the image read once, the endpoints (block outputs like the others)
    counted like them; the SE vectors and the weights once."""
    from streamingflow_amd.models.efficientnet import walk_shapes
    shapes, _ = walk_shapes(trunk.blocks_args, trunk.c_stem, trunk.pads(H, W), H, W)
    act = n * 3 * H * W                                                # the image, read
    act += 2 * n * shapes[0][0] * shapes[0][1] * shapes[0][2]          # stem output
    for a, sin, sout in zip(trunk.blocks_args, shapes, shapes[1:]):
        cexp = a.cin * a.expand
        if a.expand != 1:
            act += 2 * n * cexp * sin[1] * sin[2]                      # expanded tensor
        act += 2 * n * cexp * sout[1] * sout[2]                        # depthwise output
        act += 2 * n * a.cout * sout[1] * sout[2]                      # block output
        if a.skip:
            act += n * a.cout * sout[1] * sout[2]                      # the input read again for the residual
        act += 3 * 2 * n * cexp                                        # sums (8 bytes) and gate, written and read
    weights = sum(p.numel() for p in trunk.parameters()) + sum(b.numel() for b in trunk.buffers() if b.is_floating_point())
    return 4 * act, 4 * weights


def run(reps=30, warmup=3):
    import effnet_util as U
    from streamingflow_amd.models.efficientnet import EfficientNetTrunk
    reps, warmup = max(reps, 20), max(warmup, 3)
    dev = torch.device("cuda", 0)
    n, H, W = 18, 224, 480
    trunk = EfficientNetTrunk("b4")
    trunk.load_state_dict(U.trunk_state("b4"))
    trunk = trunk.eval().to(dev)
    x = U.images("trunkbench", (n, 3, H, W)).to(dev)
    ref = U.RefTrunk(U.trunk_state("b4"), "b4", dtype=torch.float32, device=dev)
    out = {}

    def form_a():
        out["a"] = trunk.endpoints_nhwc(x)

    def form_b():
        out["b"] = ref.walk(x)

    forms = {"a_effnet_trunk_fwd": form_a, "b_restatement_torch_fp32_miopen": form_b}
    for f in forms.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    stat = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                "spread_ms": statistics.quantiles(v, n=4)[2] - statistics.quantiles(v, n=4)[0]} for k, v in times.items()}
    mx = lambda p, q: float((p.double() - q.double()).abs().max())
    agree = {"hi": mx(out["a"][0].permute(0, 3, 1, 2), out["b"][0]), "lo": mx(out["a"][1].permute(0, 3, 1, 2), out["b"][1])}
    act, wts = algorithmic_bytes(trunk, n, H, W)
    a = stat["a_effnet_trunk_fwd"]
    gbs = (act + wts) / (a["median_ms"] * 1e-3) / 1e9
    return {"workload": f"EfficientNet-b4 trunk to block 21, {n} x 3 x {H} x {W}, fp32, hashed weights (tests/effnet_util.py)",
            "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": reps, "warmup": warmup,
            "timing": "device events around one call; the two forms alternate; spread = interquartile range", "forms_ms": stat,
            "a_not_slower_than_b": bool(a["median_ms"] <= stat["b_restatement_torch_fp32_miopen"]["median_ms"]),
            "speedup_a_over_b": stat["b_restatement_torch_fp32_miopen"]["median_ms"] / a["median_ms"],
            "agreement_a_vs_b_max_abs": agree,
            "algorithmic_bytes": {"activations": act, "weights": wts, "rule": "each activation written once and read once, image read once, + weights"},
            "peak_hbm_gbs": PEAK_HBM_GBS, "a_algorithmic_gbs": gbs, "a_fraction_of_hbm_roof": gbs / PEAK_HBM_GBS,
            "a_ms_at_hbm_roof": (act + wts) / (PEAK_HBM_GBS * 1e9) * 1e3}


def parity():
    """The trunk cases of tests/test_gpu_effnet_trunk.py: observed max |device - float64| per endpoint and the bound the test asserts."""
    import effnet_util as U
    from streamingflow_amd.models.efficientnet import NOMINAL, EfficientNetTrunk
    mx = lambda p, q: float((p.double() - q.double()).abs().max())
    cases = []
    for version, shape, size in CASES:
        sd = U.trunk_state(version)
        t = EfficientNetTrunk(version, 8, image_size=NOMINAL if size == "nominal" else size)
        t.load_state_dict(sd)
        t = t.eval().cuda()
        xs = U.images("trunk", shape)
        r64, r32 = U.RefTrunk(sd, version, 8, size).walk(xs), U.RefTrunk(sd, version, 8, size, torch.float32).walk(xs)
        hi, lo = t(xs.cuda())
        cases.append({"version": version, "downsample": 8, "images": list(shape), "padding": "static (nominal size)" if size else "dynamic",
                      "endpoints": [list(r64[0].shape[1:]), list(r64[1].shape[1:])],
                      "max_abs_err_vs_float64": [mx(hi.cpu(), r64[0]), mx(lo.cpu(), r64[1])],
                      "float32_restatement_err_vs_float64": [mx(r32[0], r64[0]), mx(r32[1], r64[1])],
                      "bound_8x": list(U.tolerance(r64, r32)), "max_abs_output": [float(r64[0].abs().max()), float(r64[1].abs().max())]})
    return {"rule": "bound = 8 x the float32 restatement's own max error against float64 on the same inputs, per endpoint (reduction_{k+1}, reduction_k)",
            "device": torch.cuda.get_device_name(0), "weights": "hashed, tests/effnet_util.py", "cases": cases}


if __name__ == "__main__":
    arg = lambda k, d: int(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d
    out_dir = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT_DIR
    r = run(arg("--reps", 30), arg("--warmup", 3))
    os.makedirs(out_dir, exist_ok=True)
    for name, rec in (("effnet_trunk_bench.json", r), ("effnet_trunk_parity.json", parity())):
        with open(os.path.join(out_dir, name), "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(r))
