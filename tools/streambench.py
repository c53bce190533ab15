"""One steady-state frame of a live stream: a session's observe + predict next to the one-shot forward over the same window.

Shipped size (C = 64, BEV 200x200, the shipped time set: 3 camera + 5 LiDAR observations, 7 targets, euler, variable step).  The
one-shot call re-encodes all 8 frames and re-applies every past jump and step; the session encodes the ONE new frame, appends its
segment to the carried state and forks the prediction.  Both sides answer the SAME target set, so the decoder and the head see
the same number of frames: "shipped7" = the shipped 7 offsets from the newest observation (-1, -.5, 0, .5, 1, 1.5, 2; the
session answers the past ones from its kept observation states), "future4" = the 4 future ones on both sides.  Both are timed with
device events (median over --reps after --warmup) in the same process with the same weights.  Prints one JSON line; --out
writes it to a file.

    python tools/streambench.py --reps 30 --warmup 5 --out profiles/streambench.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: at least 20 repetitions")
    import torch
    from util import build_pair, cases
    from streamingflow_amd import schedule as S

    C, H, W = 64, 200, 200
    cts, lts, tts, dt = cases.timeset("shipped")
    net, _ = build_pair(C, "euler", True, True, dt)
    cam, lid = cases.bev_inputs(C, H, W, 3, 5)
    cam, lid, present = cam.cuda(), lid.cuda(), cases.present_input(cam, lid).cuda()
    times, order = S.merge_observations(cts[0].tolist(), lts[0].tolist())
    frames = [(cam if src == 0 else lid)[0, i] for src, i in order]
    period = times[-1] - times[-3] if len(times) > 2 else 0.2      # the stream goes on at the LiDAR rate of the window
    offsets = {"shipped7": [t - times[-1] for t in tts[0].tolist()],                       # relative to the newest observation
               "future4": [t - times[-1] for t in tts[0].tolist() if t > times[-1]]}

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

    res = {"workload": "shipped time set (8 observations), C=64, 200x200, euler, variable step, batch 1; both sides answer the same targets",
           "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip}
    for label, in_kernel in (("in_kernel_noise", None), ("randn_noise", False)):
        net.gru_ode.noise, net.gru_ode.in_kernel_noise = None, in_kernel
        res[label] = {}
        for tname, offs in offsets.items():
            tgt = torch.tensor([[times[-1] + x for x in offs]], dtype=torch.float64)

            def forward():
                return net(present, cam, lid, cts, lts, tgt)[0]

            timed(forward, a.warmup)
            fw = timed(forward, a.reps)
            sess = net.stream()
            for t, f in zip(times, frames):
                sess.observe(t, f)
            assert tuple(sess.predict(tgt).shape) == tuple(forward().shape)      # same number of decoded frames on both sides
            now = [times[-1]]

            def frame():
                now[0] += period
                sess.observe(now[0], frames[-1], "lidar")
                return sess.predict([now[0] + x for x in offs])

            timed(frame, a.warmup)
            st = timed(frame, a.reps)
            assert frame().shape[1] == len(offs)
            res[label][tname] = {"n_targets": len(offs), "forward_ms": round(statistics.median(fw), 3), "forward_min_ms": round(min(fw), 3),
                                 "session_observe_predict_ms": round(statistics.median(st), 3), "session_min_ms": round(min(st), 3),
                                 "session_graphs": len(sess.latent._graphs),
                                 "speedup": round(statistics.median(fw) / statistics.median(st), 3)}
            sess.latent.drop_graphs()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
