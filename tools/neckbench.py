"""Camera encoder neck (N7) at the shipped size: 18 images (3 frames x 6 cameras), EfficientNet-b4 endpoints 160 x 14 x 30 and
56 x 28 x 60, C = 64, D = 48.  Three forms, alternated round by round in one process, each round timed with device events:

  a  sf_camera_neck_fwd: the twin head, one upsampling launch, four convolutions on channel slices, depth_softmax_planar_kernel
  b  the same arithmetic from the entry points the library had before it: two sf_deeplab_head_fwd, torch bilinear upsampling and cat
     (channels-last, so nothing is transposed), four sf_conv2d_ex_fwd, sf_nhwc_to_nchw of the depth logits, sf_depth_softmax_fwd
  c  the reference's formulation in stock PyTorch-ROCm float32 (tools/gen_encoder_neck_golden.py: neck_f64 at float32), NCHW

All three start from device-resident endpoints in their own layout and end with features, depth logits and depth probabilities.
The condition is a <= b within the spread the rounds themselves show.  Also records the observed errors of the GPU test cases
against float64 with their bounds.  Writes profiles/encoder_neck_bench.json and prints it.
Usage: python3 tools/neckbench.py [--rounds N] [--inner K]"""
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

OUT = os.path.join(ROOT, "profiles", "encoder_neck_bench.json")


def run(rounds=15, inner=100):
    import gen_encoder_neck_golden as GEN
    from streamingflow_amd import _lib, packing, runtime
    from streamingflow_amd.models.encoder import Encoder, dead_rates
    from workloads import hashfill
    dev = torch.device("cuda", 0)
    n, H, W, D, C = 18, 14, 30, 48, 64
    net = Encoder(GEN.cfg("b4"), D)
    net.load_state_dict(GEN.hashed_state(net.state_dict()))
    net = net.eval().to(dev)
    c_hi, c_lo = net.c_hi, net.c_lo
    hi = hashfill.normal("neckbench_hi", (n, c_hi, H, W), 71).to(dev)
    lo = hashfill.normal("neckbench_lo", (n, c_lo, 2 * H, 2 * W), 72).to(dev)
    hi_l, lo_l = runtime.to_nhwc(hi), runtime.to_nhwc(lo)
    L, pr, st = _lib.lib(), runtime.ptr, runtime.stream_ptr(dev)
    P2 = n * 4 * H * W

    # ---- a ----
    pk = net.packed(H, W)
    ws_a = runtime.static_workspace(L.sf_camera_neck_ws_bytes(c_hi, c_lo, C, D, 128, n, H, W), dev)
    rays_a = torch.empty((P2, C), device=dev)
    logits_a, prob_a = torch.empty((n, D, 4 * H * W), device=dev), torch.empty((n, D, 4 * H * W), device=dev)

    def form_a():
        _lib.check(L.sf_camera_neck_fwd(pk.struct, pk.convs, pr(hi_l), pr(lo_l), pr(rays_a), pr(logits_a), pr(prob_a), n, H, W, pr(ws_a),
                                        ws_a.numel() * 4, st), "camera_neck")

    # ---- b ----
    heads = (net.feature_layer_1, net.depth_layer_1)
    hp = [h.packed().struct for h in heads]
    ws_h = runtime.static_workspace(L.sf_deeplab_head_ws_bytes(c_hi, 64, n, H, W), dev)
    ws_c = runtime.static_workspace(L.sf_conv2d_ex_ws_bytes(), dev)
    hold = packing.Pack(None)
    joins = []
    for m in (net.feature_layer_2, net.depth_layer_2):      # conv1 reading ONE materialised cat tensor
        sc, bi = packing.bn_fold(m.conv[1])
        c1 = packing.conv_w(hold, m.conv[0].weight, c_lo + c_hi, scale=sc, bias=bi, act="relu", pad=1)
        sc, bi = packing.bn_fold(m.conv[4])
        joins.append((c1, packing.conv_w(hold, m.conv[3].weight, m.out_channels, scale=sc, bias=bi, act="relu", pad=1)))
    head_out = [torch.empty((n, H, W, c_hi), device=dev) for _ in heads]
    mids = [torch.empty((P2, C), device=dev), torch.empty((P2, D), device=dev)]
    rays_b, d_nhwc = torch.empty((P2, C), device=dev), torch.empty((P2, D), device=dev)
    logits_b, prob_b = torch.empty_like(logits_a), torch.empty_like(prob_a)
    lo_cl = lo_l.permute(0, 3, 1, 2)      # NCHW view of NHWC memory = channels_last

    def form_b():
        for i in range(2):
            _lib.check(L.sf_deeplab_head_fwd(hp[i], pr(hi_l), pr(head_out[i]), n, H, W, pr(ws_h), ws_h.numel() * 4, st), "head")
            up = torch.nn.functional.interpolate(head_out[i].permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False)
            cat = torch.cat([lo_cl, up], 1).permute(0, 2, 3, 1)
            assert cat.is_contiguous()
            c1, c2 = joins[i]
            cw = c_lo + c_hi
            _lib.check(L.sf_conv2d_ex_fwd(ctypes.byref(c1), pr(cat), cw, None, 0, None, 0, 0, pr(mids[i]), c1.cout, 0, n, 2 * H, 2 * W, 0,
                                          pr(ws_c), ws_c.numel() * 4, st), "conv1")
            out = rays_b if i == 0 else d_nhwc
            _lib.check(L.sf_conv2d_ex_fwd(ctypes.byref(c2), pr(mids[i]), c1.cout, None, 0, None, 0, 0, pr(out), c2.cout, 0, n, 2 * H, 2 * W, 0,
                                          pr(ws_c), ws_c.numel() * 4, st), "conv2")
        _lib.check(L.sf_nhwc_to_nchw(pr(d_nhwc), pr(logits_b), n, D, 4 * H * W, st), "transpose")
        _lib.check(L.sf_depth_softmax_fwd(pr(logits_b), pr(prob_b), n, D, 4 * H * W, st), "softmax")

    # ---- c ----
    sd = {k: v.to(dev) for k, v in net.state_dict().items()}
    out_c = [None]

    def form_c():
        out_c[0] = GEN.neck_f64(sd, hi, lo, dtype=torch.float32)

    forms = {"a_camera_neck_fwd": form_a, "b_unfused_parent_entry_points": form_b, "c_reference_formulation_torch_fp32": form_c}
    for f in forms.values():      # every shape of the timed window, three times
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in forms}
    for _ in range(rounds):
        for k, f in forms.items():
            e0.record()
            for _ in range(inner):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / inner)
    # same results from a and b (different launch grouping: rounding only), and against c
    feat_c, depth_c, prob_c = out_c[0]
    nchw = lambda r: r.view(n, 2 * H, 2 * W, -1).permute(0, 3, 1, 2)
    mx = lambda x, y: float((x.double() - y.double()).abs().max())
    agree = {"a_vs_b": {"features": mx(rays_a, rays_b), "depth_logits": mx(logits_a, logits_b), "depth_prob": mx(prob_a, prob_b)},
             "a_vs_c": {"features": mx(nchw(rays_a), feat_c), "depth_logits": mx(logits_a.view_as(depth_c), depth_c),
                        "depth_prob": mx(prob_a.view_as(prob_c), prob_c)}}
    stat = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                "spread_ms": statistics.quantiles(v, n=4)[2] - statistics.quantiles(v, n=4)[0]} for k, v in times.items()}
    a, b = stat["a_camera_neck_fwd"], stat["b_unfused_parent_entry_points"]
    margin = max(a["spread_ms"], b["spread_ms"])
    # observed errors of the GPU test cases against float64 (tests/encoder_neck_util.py), with the bounds the tests assert
    import encoder_neck_util as U
    errors = {}
    for name in U.CASES:
        m = U.build(name).to(dev)
        h, l = (t.to(dev) for t in GEN.endpoints(name))
        rays, logits, prob = m.neck_nhwc(h, l)
        ref = U.reference(name)
        c = GEN.CASES[name]
        f = rays.view(c["n"], 2 * c["H"], 2 * c["W"], -1).permute(0, 3, 1, 2).cpu()
        errors[name] = {"max_abs_err_vs_float64": [mx(f, ref[0]), mx(logits.view_as(ref[1]).cpu(), ref[1]), mx(prob.view_as(ref[2]).cpu(), ref[2])],
                        "float32_reference_err_vs_float64": [float(v) for v in U.fixture()[name + "/err32"]],
                        "bound_8x_plus_winograd_allowance": list(U.tolerance(name)), "order": ["features", "depth_logits", "depth_prob"],
                        "collapsed_rates": list(dead_rates((12, 24, 36), c["H"], c["W"]))}
    return {"workload": f"{n} images, hi {c_hi}x{H}x{W}, lo {c_lo}x{2 * H}x{2 * W}, C={C}, D={D}; fp32, Winograd packing {packing.winograd()}",
            "rounds": rounds, "launches_of_each_form_per_round": inner, "timing": "device events around `inner` back-to-back calls; forms alternate "
            "within a round; spread = interquartile range over rounds", "forms_ms": stat,
            "head": "twin (one sf_deeplab_w, hid 128, block-diagonal)", "collapsed_rates_at_14x30": list(dead_rates((12, 24, 36), H, W)),
            "a_le_b_within_spread": bool(a["median_ms"] <= b["median_ms"] + margin), "margin_ms": margin,
            "speedup_a_over_b": b["median_ms"] / a["median_ms"], "speedup_a_over_c": stat["c_reference_formulation_torch_fp32"]["median_ms"] / a["median_ms"],
            "agreement_max_abs": agree, "test_cases": errors}


if __name__ == "__main__":
    arg = lambda k, d: int(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d
    r = run(arg("--rounds", 15), arg("--inner", 100))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(r, f, indent=1)
    print(json.dumps(r))
