"""The whole model (``streamingflow.forward``, shipped configuration, 3 clouds of 350 000 points, 3 x 6 cameras, 7 targets) three ways,
for the feature-pair input and again from raw uint8 frames (``camera_encoder(cfg)`` + ``ImageFrontend``): (1) the default synchronising
forward — timed first and again last; it is the parent's behaviour and the baseline —, (2) the eager static forward
(``static_lidar = static_camera = True``: no host read), (3) the replay of ``net.graphed()``'s session (inputs copied into the static
buffers, fed operands filled, one graph launch).  One process, same weights and inputs; per form the GPU time between device events, the
wall time per call including the final synchronisation, and the host time until the call returns (medians over --reps after --warmup).
Prints one JSON line; --out writes it to a file.

    python tools/modelgraphbench.py --reps 20 --warmup 3 --out profiles/model_graph_bench.json
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
    ap.add_argument("--inputs", default="features,frames", help="comma-separated: features (the feature-pair input), frames (uint8 frames)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import liftbench
    import voxelbench
    from oracle import cases
    from workloads import hashfill
    from streamingflow_amd import ImageFrontend
    from streamingflow_amd.models.streamingflow import camera_encoder, default_cfg, streamingflow
    from streamingflow_amd.voxelize import voxelize

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

    T = a.clouds
    b, s, n, C, D, fH, fW = 1, 3, 6, 64, 48, 28, 60
    clouds = [voxelbench.cloud(seed=10 + t)[None].cuda() for t in range(T)]
    cts = torch.tensor([[-1.0, -0.5, 0.0]], dtype=torch.float64)
    lts = torch.tensor([[-0.2 * (T - 1 - t) for t in range(T)]], dtype=torch.float64)
    tts = torch.tensor([[-1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0]], dtype=torch.float64)
    intr, extr, ego = liftbench.synthetic_rig(b, s, n, "cuda")
    res = {"workload": "shipped configuration, batch 1: %d x %d cameras, %d clouds of 350 000 points, %d targets" % (s, n, T, tts.shape[1]),
           "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip}

    for kind in a.inputs.split(","):
        cfg = default_cfg()
        torch.manual_seed(7)
        if kind == "frames":
            fe = ImageFrontend.from_cfg(cfg)
            net = streamingflow(cfg, encoder=camera_encoder(cfg), frontend=fe).eval()
        else:
            net = streamingflow(cfg).eval()
        sd = net.state_dict()
        fill = {k: v for k, v in sd.items() if not k.startswith(("encoder.", "bev_", "lift.", "frustum"))}
        sd.update(hashfill.fill_state_dict(fill, seed=91, gain=0.9))
        pre = "future_prediction_ode."      # (weights that keep the rollout's values finite, as the end-to-end tests fill them)
        sd.update({pre + k: v for k, v in cases.fpode_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}).items()})
        pb = "encoders.lidar.backbone."
        sd.update(hashfill.fill_state_dict({k: v for k, v in sd.items() if k.startswith(pb)}, seed=92, gain=1.6))
        net.load_state_dict(sd)
        net = net.cuda()
        ode = net.future_prediction_ode.gru_ode
        if kind == "frames":
            g = torch.Generator().manual_seed(5)
            image = torch.randint(0, 256, (b, s, n, 900, 1600, 3), dtype=torch.uint8, generator=g).cuda()
            K = intr.clone()      # the intrinsics of the 900 x 1600 frames whose update gives the rig's
            K[..., 0, 0] /= fe.resize_scale
            K[..., 1, 1] /= fe.resize_scale
            K[..., 0, 2] = (intr[..., 0, 2] + fe.crop[0]) / fe.resize_scale
            K[..., 1, 2] = (intr[..., 1, 2] + fe.crop[1]) / fe.resize_scale
        else:
            image = (hashfill.normal("mgb_feat", (b, s, n, C, fH, fW), 95).cuda(), (hashfill.normal("mgb_logits", (b, s, n, D, fH, fW), 96) * 2).cuda())
            K = intr
        args = (image, K, extr, ego, None, cts, clouds, lts, tts)
        r = {}
        with torch.no_grad():
            r["synchronising_first"] = measure(lambda: net(*args))
            # capacities: the counts of these clouds (index kernels of the synchronising path) with 10 % head-room — the clouds of
            # voxelbench are scattered Gaussians, whose sites grow under the first stride-2 convolutions, past the default capacities
            backbone, vox = net.encoders["lidar"]["backbone"], net.encoders["lidar"]["voxelize"]
            _, c, _ = voxelize([p[0].float() for p in clouds], vox, True)
            c, shape, seen = c.int().contiguous(), list(backbone.sparse_shape), []
            for conv in backbone.strided_convs():
                c, shape = backbone._out_sites(c, T, shape, conv.kernel_size, conv.stride, conv.padding)
                c = c.contiguous()
                seen.append(c.shape[0])
            net.lidar_capacities = [v + v // 10 for v in seen]
            r["capacities"] = net.lidar_capacities
            net.static_lidar = net.static_camera = True
            ode.seed_noise(1)
            want = {k: v.clone() for k, v in net(*args).items() if torch.is_tensor(v)}
            r["static_eager"] = measure(lambda: net(*args))
            net.static_lidar = net.static_camera = False
            ode.seed_noise(1)
            session = net.graphed()
            got = session(*args)
            session.check()
            r["replay_equals_eager"] = all(bool(torch.equal(got[k], v)) for k, v in want.items())
            r["session_replay"] = measure(lambda: session(*args))
            r["session_graphs"], r["session_captures"] = len(session), session.captures
            session.drop_graphs()
            net.lidar_capacities = None
            r["synchronising_last"] = measure(lambda: net(*args))
        res[kind] = r
        del net, session, got, want
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
