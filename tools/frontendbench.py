"""Camera image front end (N9) at the shipped size: 18 frames (3 sensor frames x 6 cameras) of 900 x 1600 x 3 uint8 -> 3 x 224 x 480 fp32.

  a  sf_image_frontend_fwd (streamingflow_amd/image_frontend.py): one launch, timed with device events, median of --reps runs (at least
     20) after --warmup (at least 3); a second figure times 20 launches between one pair of events, which takes the events' own
     resolution and the launch gap out of a kernel this short
  b  the same 18 frames through PIL + torch on this machine's CPU, the reference data loader's way (Image.fromarray -> resize -> crop ->
     ToTensor + Normalize arithmetic), wall clock, if PIL imports here; otherwise the field says so

Also records the algorithmic bytes — the source rows the crop keeps, read once, plus the fp32 output written once — the fraction of the
HBM roof they would need the median time of form a, and that the device result equals the numpy restatement on one frame.
Writes frontendbench.json into profiles/ (or --out DIR) and prints it.
Usage: python3 tools/frontendbench.py [--reps N] [--warmup N] [--out DIR]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT_DIR = os.path.join(ROOT, "profiles")
PEAK_HBM_GBS = 8000.0
BURST = 20


def algorithmic_bytes(fe, n):
    """The source rows some output row's vertical taps read, whole rows, once; the fp32 output once."""
    import image_frontend_util as U
    (Hs, Ws), (w_r, h_r), (l, t, r, b) = fe.original, fe.resize_dims, fe.crop
    bounds = U.table(Hs, h_r)[0]
    rows = range(max(t, 0), min(b, h_r))
    first, last = int(bounds[rows[0], 0]), int(bounds[rows[-1]].sum())
    src = n * (last - first) * Ws * 3
    out = n * 3 * (b - t) * (r - l) * 4
    return src, out, (first, last)


def cpu_pipeline(frames, fe):
    from PIL import Image
    mean, std = (torch.tensor(v, dtype=torch.float32).view(3, 1, 1) for v in (fe.mean, fe.std))
    t0 = time.perf_counter()
    out = []
    for f in frames:
        img = Image.fromarray(f).resize(fe.resize_dims, resample=Image.BILINEAR).crop(fe.crop)
        out.append(torch.from_numpy(np.array(img)).permute(2, 0, 1).float().div(255).sub(mean).div(std))
    out = torch.stack(out)
    return (time.perf_counter() - t0) * 1e3, out


def run(reps=30, warmup=3):
    import image_frontend_util as U
    from streamingflow_amd import ImageFrontend
    reps, warmup = max(reps, 20), max(warmup, 3)
    dev = torch.device("cuda", 0)
    n = 18
    fe = ImageFrontend()
    frames = np.stack([U.source(9000 + i, 900, 1600) for i in range(n)])
    raw = torch.from_numpy(frames).to(dev)
    for _ in range(warmup):
        out = fe.images(raw)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    single, burst = [], []
    for _ in range(reps):
        e0.record()
        out = fe.images(raw)
        e1.record()
        e1.synchronize()
        single.append(e0.elapsed_time(e1))
        e0.record()
        for _ in range(BURST):
            fe.images(raw)
        e1.record()
        e1.synchronize()
        burst.append(e0.elapsed_time(e1) / BURST)
    stat = lambda v: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                      "spread_ms": statistics.quantiles(v, n=4)[2] - statistics.quantiles(v, n=4)[0]}
    want = U.normalise(U.resize_and_crop(frames[0], fe.resize_dims, fe.crop))
    src_b, out_b, rows = algorithmic_bytes(fe, n)
    a, a20 = stat(single), stat(burst)
    rec = {"workload": f"{n} frames 900 x 1600 x 3 uint8 -> resize (480, 270) -> crop (0, 46, 480, 270) -> 3 x 224 x 480 fp32",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": reps, "warmup": warmup,
           "timing": "device events; spread = interquartile range; the burst figure is 20 back-to-back calls between one pair of events, per call",
           "a_image_frontend_fwd_one_call": a, "a_image_frontend_fwd_per_call_in_a_burst_of_20": a20,
           "bitwise_equal_to_restatement_frame_0": bool(torch.equal(out[0].cpu(), want)),
           "algorithmic_bytes": {"source": src_b, "output": out_b, "source_rows_kept": list(rows),
                                 "rule": "the source rows the crop keeps, whole, read once + the fp32 output written once"},
           "peak_hbm_gbs": PEAK_HBM_GBS}
    for key, s in (("one_call", a), ("burst", a20)):
        gbs = (src_b + out_b) / (s["median_ms"] * 1e-3) / 1e9
        rec["a_algorithmic_gbs_" + key], rec["a_fraction_of_hbm_roof_" + key] = gbs, gbs / PEAK_HBM_GBS
    rec["a_ms_at_hbm_roof"] = (src_b + out_b) / (PEAK_HBM_GBS * 1e9) * 1e3
    try:
        import PIL
        times = []
        for _ in range(3):
            ms, cpu_out = cpu_pipeline(frames, fe)
            times.append(ms)
        rec["b_pil_torch_cpu"] = {"where": "this machine's CPU, one thread of Python driving PIL and torch", "pillow": PIL.__version__,
                                  "median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times),
                                  "bitwise_equal_to_a": bool(torch.equal(cpu_out, out.cpu()))}
        rec["speedup_a_over_b"] = rec["b_pil_torch_cpu"]["median_ms"] / a["median_ms"]
    except ImportError:
        rec["b_pil_torch_cpu"] = "not measured: PIL does not import on this machine"
    return rec


if __name__ == "__main__":
    arg = lambda k, d: int(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d
    out_dir = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT_DIR
    r = run(arg("--reps", 30), arg("--warmup", 3))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "frontendbench.json"), "w") as f:
        json.dump(r, f, indent=1)
    print(json.dumps(r))
