"""GPU: the planner's device path (sf_plan_cost_fwd, sf_plan_select_refine_fwd, sf_plan_metric_fwd; streamingflow_amd.cost,
.models.planning, .metrics.PlanningMetric) against the REFERENCE's results (tests/golden/planning.npz) and against the module's own
plain-torch path on inputs beyond the fixtures.  Tolerances: planning_util.py (costs), the generator's refine.tol (refinement);
selected trajectories and metric counters exactly."""
import ctypes

import pytest
import torch

import planning_util as PU
from streamingflow_amd._lib import SF_ERR_INVALID, SF_ERR_WORKSPACE

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag", PU.TAGS)
def test_costs_select_and_forward_match_the_reference(tag):
    PU.check_scene(tag, "cuda")


@pytest.mark.parametrize("tag", PU.TAGS)
def test_planning_metric_matches_the_reference(tag):
    PU.check_metric(tag, "cuda")


def _off_lattice(tag):
    """A fixture scene with its trajectories moved off the quarter-cell lattice by up to 0.4 m (hashed, so the same on every run)."""
    sc = dict(PU.on(PU.scene(tag), "cuda"))
    shift = PU.GEN.hashfill.uniform("planning.shift." + tag, tuple(sc["trajs"].shape[:3]) + (2,), -0.4, 0.4, seed=3).cuda()
    sc["trajs"] = torch.cat([sc["trajs"][..., :2] + shift, sc["trajs"][..., 2:]], -1).contiguous()
    return sc


@pytest.mark.parametrize("tag", ("n66", "t6", "n600"))
def test_device_path_equals_torch_path_beyond_the_fixtures(tag, monkeypatch):
    net, sc = PU.model(tag, "cuda"), _off_lattice(tag)
    lane, drv = PU.maps(sc)
    args = (sc["cost_volume"], sc["trajs"][..., :2], sc["semantic_pred"], lane, drv, sc["target_points"])
    fc, fo, cs = net.cost_function.costs(*args)
    sel = net.select(sc["trajs"], *args[:1], *args[2:])
    monkeypatch.setenv("SF_PLAN_TORCH", "1")
    tfc, tfo, tcs = net.cost_function.costs(*args)
    tsel = net.select(sc["trajs"], *args[:1], *args[2:])
    gaps = [PU.cost_gap(fc, tfc.cpu().numpy(), PU.FC_TOL), PU.cost_gap(fo, tfo.cpu().numpy())]
    print(f"{tag}: device vs torch path, cost_fc gap {gaps[0]:.3f}, cost_fo gap {gaps[1]:.3f} (in units of their bounds)")
    assert max(gaps) <= 1.0, gaps                       # a cell that differed would move a term by whole units
    assert PU.cost_gap(cs, tcs.cpu().numpy()) <= float(fo.shape[-1] + 1)
    assert torch.equal(sel, tsel)


def test_row_stride_3_equals_packed():
    net, sc = PU.model("n66", "cuda"), PU.on(PU.scene("n66"), "cuda")
    lane, drv = PU.maps(sc)
    rest = (sc["semantic_pred"], lane, drv, sc["target_points"])
    strided = sc["trajs"][..., :2]
    assert strided.stride(2) == 3 and not strided.is_contiguous()
    a = net.cost_function.costs(sc["cost_volume"], strided, *rest)
    b = net.cost_function.costs(sc["cost_volume"], strided.contiguous(), *rest)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_metric_accumulates_and_resets():
    one, n = PU.metric_of("n600", "cuda", updates=1)
    two, _ = PU.metric_of("n600", "cuda", updates=2)
    assert two.total.is_cuda and int(two.total) == 2 * n and bool(one.obj_box_col.any())
    for k in ("obj_col", "obj_box_col", "L2"):
        assert torch.equal(getattr(two, k), 2 * getattr(one, k)), k            # doubling is exact
    two.reset()
    assert int(two.total) == 0 and not any(bool(getattr(two, k).any()) for k in ("obj_col", "obj_box_col", "L2"))


def test_forward_is_capturable():
    """Nothing of forward reads the device back (target_points.sum() < 0.5 is formed there), so it can be captured and replayed."""
    net, sc = PU.model("n66", "cuda"), PU.on(PU.scene("n66"), "cuda")
    args = (sc["cam_front"], sc["trajs"], sc["gt_trajs"], sc["cost_volume"], sc["semantic_pred"], sc["hd_map"], sc["commands"], sc["target_points"])
    eager = net(*args)[1].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        net(*args)                                      # this stream's workspace and the packed weights exist before the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            _, out = net(*args)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_entry_points_reject_invalid_arguments():
    from streamingflow_amd import _lib, runtime
    from streamingflow_amd.runtime import ptr
    L = _lib.lib()
    dev = torch.device("cuda")
    B, N, T, G, S = 1, 4, 2, 48, 32
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    trajs, cv, occ, lane, drv, tp = f(B, N, T, 3), f(B, T, G, G), torch.zeros((B, T, G, G), dtype=torch.uint8, device=dev), f(B, G, G), f(B, G, G), f(B, 2)
    rc = torch.zeros((8, 2), dtype=torch.int32, device=dev)
    dx, bx, w = torch.full((2,), 0.5, device=dev), torch.full((2,), -11.75, device=dev), torch.ones(2, device=dev)
    fo, fc, cs = f(B, N, T), f(B, N), f(B, N)
    ws = runtime.workspace(L.sf_plan_cost_ws_bytes(), dev)
    factors = (ctypes.c_float * 7)(*([1.0] * 7))
    st = runtime.stream_ptr(dev)

    def cost(trajs=trajs, rc0=rc, N=N, T=T, H=G, W=G, cs=cs, ws_bytes=ws.numel() * 4):
        return L.sf_plan_cost_fwd(ptr(trajs), 3, ptr(cv), ptr(occ), ptr(lane), ptr(drv), ptr(tp), ptr(rc0), 8, ptr(rc), 8, ptr(dx), ptr(bx), ptr(w),
                                  ctypes.byref(factors), 10.0, 1.0, B, N, T, H, W, ptr(fo), ptr(fc), ptr(cs), ptr(ws), ws_bytes, st)

    assert cost() == 0
    assert cost(trajs=None) == cost(rc0=None) == cost(cs=None) == SF_ERR_INVALID
    assert cost(N=0) == cost(T=0) == cost(H=G, W=G - 8) == cost(H=0, W=0) == SF_ERR_INVALID
    assert cost(ws_bytes=4) == SF_ERR_WORKSPACE

    h0, sel, out = f(B, S), f(B, T, 3), f(B, T, 3)
    wts = [f(3 * S, 6), f(3 * S, S), f(3 * S), f(3 * S), f(S, S), f(S), f(2, S), f(2)]

    def refine(cs=cs, N=N, T=T, S=S, sel=sel, wts=wts, out=out):
        return L.sf_plan_select_refine_fwd(ptr(cs), ptr(trajs), 3, ptr(tp), ptr(h0), *[ptr(t) for t in wts], B, N, T, S, ptr(sel), ptr(out), st)

    assert refine() == 0
    assert refine(S=0, wts=[None] * 8, out=None) == 0                     # selection alone
    assert refine(cs=None) == refine(sel=None) == refine(out=None) == refine(wts=[None] + wts[1:]) == SF_ERR_INVALID
    assert refine(N=0) == refine(T=0) == refine(S=257) == refine(S=-1) == SF_ERR_INVALID

    seg = torch.zeros((B, T, G, G), dtype=torch.uint8, device=dev)
    cnt = [f(T), f(T), f(T), torch.zeros((), dtype=torch.int64, device=dev)]

    pred, truth = trajs[:, 1].contiguous(), trajs[:, 0].contiguous()

    def metric(gt=truth, T=T, H=G, W=G, total=cnt[3]):
        return L.sf_plan_metric_fwd(ptr(pred), ptr(gt), 3, ptr(seg), ptr(rc), 8, ptr(dx), ptr(bx),
                                    B, T, H, W, ptr(cnt[0]), ptr(cnt[1]), ptr(cnt[2]), ptr(total), st)

    assert metric() == 0
    assert metric(gt=None) == metric(total=None) == metric(T=0) == metric(W=G + 1) == SF_ERR_INVALID
    torch.cuda.synchronize()
    assert int(cnt[3]) == B


def test_whole_model_feeds_the_planner():
    """PLANNING.ENABLED at the smallest camera configuration of the end-to-end tests (its rig, 32 feature channels instead of 16: the
    convolution kernels move channels in fours and the planner's last bottleneck has C / 8 of them): the model hands out the front
    camera's features and the cost volume, and the planner turns them into a trajectory."""
    from test_gpu_end_to_end import small_cfg
    from streamingflow_amd.models.streamingflow import streamingflow
    from util import cases, hashfill, maxabs
    cfg, _ = small_cfg()
    cfg.MODEL.MODALITY.USE_LIDAR = False
    C = 32
    cfg.MODEL.ENCODER.OUT_CHANNELS = cfg.MODEL.TEMPORAL_MODEL.START_OUT_CHANNELS = cfg.MODEL.DISTRIBUTION.LATENT_DIM = C
    cfg.MODEL.SMALL_ENCODER.FILTER_SIZE = C
    cfg.PLANNING.ENABLED, cfg.PLANNING.GRU_STATE_SIZE, cfg.PLANNING.SAMPLE_NUM = True, 4, 9       # 4 x 6 features -> 1 x 1 x (C / 8)
    net = streamingflow(cfg).eval()
    sd = hashfill.fill_state_dict(net.state_dict(), seed=91, gain=0.9)
    pre = "future_prediction_ode."
    sd.update({pre + k: v for k, v in cases.fpode_state_dict({k[len(pre):]: v for k, v in net.state_dict().items() if k.startswith(pre)}).items()})
    for k, v in net.state_dict().items():          # geometry, not weights
        if k.startswith(("bev_", "lift.", "frustum", "planning.cost_function.")):
            sd[k] = v
    net.load_state_dict(sd)
    net = net.cuda()
    net.future_prediction_ode.gru_ode.noise = hashfill.HashedNoise(cases.EPS_SEED)
    feat, depth, intr, extr, ego = (t.cuda() for t in cases.lift_rig_inputs("e2e_c16")[:5])
    feat = hashfill.normal("planning.e2e.feat", tuple(feat.shape[:3]) + (C,) + tuple(feat.shape[-2:]), seed=46).cuda()
    cts = torch.tensor([[-1.0, -0.5, 0.0]], dtype=torch.float64)
    tts = torch.tensor([[0.5, 1.0, 1.5, 2.0]], dtype=torch.float64)
    out = net((feat, depth), intr, extr, ego, None, cts, None, None, tts)
    b, T = feat.shape[0], min(cfg.N_FUTURE_FRAMES, out["costvolume"].shape[1])
    G = int(net.bev_dimension[0])
    assert tuple(out["cam_front"].shape) == (b, C) + tuple(feat.shape[-2:]) and torch.equal(out["cam_front"], feat[:, -1, 1])
    cost_volume = out["costvolume"][:, -T:].reshape(b, T, G, G)
    occupancy = out["segmentation"][:, -T:].argmax(dim=2)
    trajs = PU.GEN._snap(hashfill.uniform("e2e.trajs", (b, 9, T, 3), -3.0, 3.0, seed=5)).cuda()
    hd_map = hashfill.uniform("e2e.hd", (b, 2, G, G), 0.0, 1.0, seed=6).cuda()
    loss, traj = net.planning(out["cam_front"], trajs, None, cost_volume, occupancy, hd_map, ["FORWARD"], torch.tensor([[1.0, 3.0]]).cuda())
    assert loss == 0 and tuple(traj.shape) == (b, T, 3) and bool(torch.isfinite(traj).all()) and bool((traj[..., 2] == 0).all())
    assert bool(torch.isfinite(cost_volume).all())
    # the same weights with planning off: no planner outputs, and the other heads are what they were.  Not bit for bit: the decoder's
    # stacked 3x3 head convolution has one head fewer, so the conv dispatch may take another kernel form with another summation order;
    # 1e-3 is the end-to-end bound of these heads
    cfg.PLANNING.ENABLED = False
    off = streamingflow(cfg).eval()
    off.load_state_dict({k: v for k, v in sd.items() if k in off.state_dict()})
    off = off.cuda()
    off.future_prediction_ode.gru_ode.noise = hashfill.HashedNoise(cases.EPS_SEED)
    plain = off((feat, depth), intr, extr, ego, None, cts, None, None, tts)
    assert plain["cam_front"] is None and plain["costvolume"] is None and not hasattr(off, "planning")
    for k in ("segmentation", "instance_center", "instance_offset", "instance_flow"):
        assert maxabs(plain[k], out[k]) <= 1e-3, k
