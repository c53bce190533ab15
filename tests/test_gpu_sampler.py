"""GPU: the trajectory sampler's device path (sf_fresnel_fwd, sf_plan_sample_fwd; streamingflow_amd.sampler) against the REFERENCE's
rows and scipy's Fresnel values (tests/golden/sampler.npz).  The comparison rule and its tolerances: sampler_util.py.  Every case is
one sample-sized launch (M <= 1800)."""
import numpy as np
import pytest
import torch

import sampler_util as SU
from streamingflow_amd._lib import SF_ERR_INVALID, SF_ERR_WORKSPACE, SF_ERR_UNSUPPORTED

pytestmark = pytest.mark.gpu


def test_fresnel_kernel_matches_scipy():
    from streamingflow_amd import _lib, runtime
    from streamingflow_amd.runtime import ptr
    G = SU.golden()
    z = torch.from_numpy(G["fresnel.z"]).cuda()
    S, C = torch.empty_like(z), torch.empty_like(z)
    _lib.check(_lib.lib().sf_fresnel_fwd(ptr(z), z.numel(), ptr(S), ptr(C), runtime.stream_ptr(z.device)), "fresnel")
    es, ec = np.abs(S.cpu().numpy() - G["fresnel.S"]), np.abs(C.cpu().numpy() - G["fresnel.C"])
    print(f"sf_fresnel_fwd: largest |error| against scipy over {z.numel()} points: S {es.max():.3e}, C {ec.max():.3e}")
    assert max(es.max(), ec.max()) <= SU.FRESNEL_TOL
    assert torch.equal(S, -_neg(z)[0]) and torch.equal(C, -_neg(z)[1])      # odd in z, bit for bit
    edge = torch.tensor([float("inf"), -float("inf"), float("nan")], dtype=torch.float64).cuda()
    S, C = torch.empty_like(edge), torch.empty_like(edge)
    _lib.check(_lib.lib().sf_fresnel_fwd(ptr(edge), 3, ptr(S), ptr(C), runtime.stream_ptr(z.device)), "fresnel")
    assert S.tolist()[:2] == C.tolist()[:2] == [0.5, -0.5] and bool(torch.isnan(S[2])) and bool(torch.isnan(C[2]))


def _neg(z):
    from streamingflow_amd import _lib, runtime
    from streamingflow_amd.runtime import ptr
    m = (-z).contiguous()
    S, C = torch.empty_like(m), torch.empty_like(m)
    _lib.check(_lib.lib().sf_fresnel_fwd(ptr(m), m.numel(), ptr(S), ptr(C), runtime.stream_ptr(m.device)), "fresnel")
    return S, C


@pytest.mark.parametrize("launches", ("1", "2"))
@pytest.mark.parametrize("tag", SU.TAGS)
def test_device_path_matches_the_reference(tag, launches, monkeypatch):
    """Both launch shapes (SF_PLAN_SAMPLE_LAUNCHES; the default is one of them) against every scene."""
    monkeypatch.setenv("SF_PLAN_SAMPLE_LAUNCHES", launches)
    out, order = SU.run_scene(tag, "cuda")
    assert out.dtype == torch.float32 and order.dtype == torch.int32 and out.is_cuda
    SU.check_rows(tag, out, order, f" ({launches} launch{'es' if launches == '2' else ''})")


def _batch(smp):
    G = SU.golden()
    u = torch.from_numpy(G["m600.uniforms"])
    us = torch.stack([u, u.flip(-1), u * 0.5]).cuda()
    return torch.tensor([0.0, 4.0, 20.0]).cuda(), torch.tensor([0.3, 0.0, -0.5]).cuda(), us


def test_batch_equals_single_calls_and_runs_repeat_bitwise():
    from streamingflow_amd.sampler import TrajectorySampler
    smp = TrajectorySampler(6, n_samples=600)
    v0, kappa, us = _batch(smp)
    out, order = smp(v0, kappa, uniforms=us, return_order=True)
    again, order2 = smp(v0, kappa, uniforms=us, return_order=True)
    assert torch.equal(out, again) and torch.equal(order, order2)
    for b in range(3):
        one, o1 = smp(v0[b:b + 1], kappa[b:b + 1], uniforms=us[b:b + 1], return_order=True)
        assert torch.equal(out[b], one[0]) and torch.equal(order[b], o1[0]), b
    plain = smp(v0, kappa, uniforms=us)                                       # order = NULL
    assert torch.equal(plain, out)
    assert torch.equal(order.long().sort(dim=1)[0], torch.arange(600, device="cuda").expand(3, -1))
    # the device and the plain-torch path agree as the fixtures demand of either: rows through the device's order, within one fp32 ulp
    rows, _ = smp(v0.cpu(), kappa.cpu(), uniforms=us.cpu(), return_order=True)
    assert rows.device.type == "cpu"
    gap = ((out.cpu().double() - rows.double()).abs() / (SU.ROW_TOL * rows.double().abs().clamp(min=1.0))).max()
    print(f"device against torch path, B = 3: largest row difference {float(gap):.3f} x 2^-23 max(1, |value|)")
    assert float(gap) <= 1.0


def test_entry_point_rejects_invalid_arguments():
    from streamingflow_amd import _lib, runtime
    from streamingflow_amd.runtime import ptr
    L = _lib.lib()
    dev = torch.device("cuda")
    B, M, n_t = 1, 10, 2
    d = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
    v0, kappa, t0, n0, tt, u = d(B), d(B), d(B, 2), d(B, 2), d(n_t), d(B, 5, 4100)
    out = torch.zeros((B, 4100, n_t, 3), dtype=torch.float32, device=dev)
    order = torch.zeros((B, 4100), dtype=torch.int32, device=dev)
    ws = runtime.workspace(L.sf_plan_sample_ws_bytes(B, 4100, n_t), dev)
    st = runtime.stream_ptr(dev)

    def call(v0=v0, tt=tt, u=u, out=out, order=order, ws=ws, counts=(2, 4, 4), B=B, M=M, n_t=n_t, ws_bytes=ws.numel() * 4):
        return L.sf_plan_sample_fwd(ptr(v0), ptr(kappa), ptr(t0), ptr(n0), ptr(tt), 0.5, ptr(u), *counts, B, M, n_t, ptr(out), ptr(order), ptr(ws),
                                    ws_bytes, st)

    assert L.sf_plan_sample_ws_bytes(1, 1800, 7) >= 1800 * 8 and L.sf_plan_sample_ws_bytes(0, 5, 2) == 0
    assert call() == 0 and call(order=None) == 0
    assert call(v0=None) == call(tt=None) == call(u=None) == call(out=None) == call(ws=None) == SF_ERR_INVALID
    assert call(B=0) == call(M=0, counts=(0, 0, 0)) == call(n_t=0) == SF_ERR_INVALID
    assert call(counts=(2, 4, 3)) == call(counts=(-2, 8, 4)) == SF_ERR_INVALID
    assert call(M=4097, counts=(819, 1639, 1639)) == SF_ERR_UNSUPPORTED
    assert call(M=4096, counts=(820, 1638, 1638)) == 0                       # the largest sample the kernel takes
    assert call(ws_bytes=M * 8 - 1) == SF_ERR_WORKSPACE
    torch.cuda.synchronize()


def test_non_finite_inputs_write_nothing_out_of_range():
    """NaN / infinite speed, curvature and uniforms: the rows are unspecified, but every rank stays below M, so the guard rows on either
    side of out and order keep their values and order holds row numbers (or what it held before, where two NaN keys share a rank)."""
    import ctypes
    from streamingflow_amd import _lib, runtime, sampler as S
    from streamingflow_amd.runtime import ptr
    L = _lib.lib()
    M, n_t, pad = 50, 3, 8
    dev = torch.device("cuda")
    nan = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
    u = torch.from_numpy(SU.golden()["m50.uniforms"].copy()).to(dev)[None].contiguous()
    u[0, 0, ::7] = float("nan")
    t0 = torch.tensor([[0.0, 1.0]], dtype=torch.float64, device=dev)
    n0 = torch.tensor([[1.0, 0.0]], dtype=torch.float64, device=dev)
    tt = torch.tensor([0.0, 0.5, 1.0], dtype=torch.float64, device=dev)
    ws = runtime.workspace(L.sf_plan_sample_ws_bytes(1, M, n_t), dev)
    for v0, kappa in ((nan, nan), (nan, torch.zeros_like(nan)), (torch.ones_like(nan), torch.full_like(nan, float("inf")))):
        out = torch.full((M + 2 * pad, n_t, 3), -7.0, dtype=torch.float32, device=dev)
        order = torch.full((M + 2 * pad,), -7, dtype=torch.int32, device=dev)
        _lib.check(L.sf_plan_sample_fwd(ptr(v0), ptr(kappa), ptr(t0), ptr(n0), ptr(tt), 1.0, ptr(u), *S.counts(M), 1, M, n_t,
                                        ctypes.c_void_p(out.data_ptr() + pad * n_t * 3 * 4), ctypes.c_void_p(order.data_ptr() + pad * 4), ptr(ws),
                                        ws.numel() * 4, runtime.stream_ptr(dev)), "plan_sample")
        torch.cuda.synchronize()
        assert bool((out[:pad] == -7).all()) and bool((out[-pad:] == -7).all()) and bool((order[:pad] == -7).all()) and bool((order[-pad:] == -7).all())
        inner = order[pad:-pad]
        assert bool(((inner == -7) | ((inner >= 0) & (inner < M))).all())


def test_sampler_is_capturable_and_feeds_the_planner():
    """Nothing of the sampler reads the device back, so sampler -> Planning.forward is captured and replayed as one graph; the selected
    trajectory is bit for bit one of the sampled rows.  (No device / torch cost equality is asked here: sampled points are not snapped
    away from cell boundaries.)"""
    import planning_util as PU
    from streamingflow_amd.sampler import TrajectorySampler
    net, sc = PU.model("n600", "cuda"), PU.on(PU.scene("n600"), "cuda")
    B, T = sc["trajs"].shape[0], sc["trajs"].shape[2]
    smp = TrajectorySampler(T, n_samples=600)
    v0 = torch.tensor([0.0, 4.0, 20.0], dtype=torch.float64).cuda()[:B]
    kappa = torch.tensor([0.3, 0.0, -0.5], dtype=torch.float64).cuda()[:B]
    us = _batch(smp)[2][:B]
    rest = (sc["gt_trajs"], sc["cost_volume"], sc["semantic_pred"], sc["hd_map"], sc["commands"], sc["target_points"])

    def plan():
        trajs = smp(v0, kappa, uniforms=us)[:, :, 1:]
        return trajs, net(sc["cam_front"], trajs, *rest)[1]

    trajs, eager = plan()
    assert tuple(trajs.shape) == (B, 600, T, 3) and tuple(eager.shape) == (B, T, 3) and bool(torch.isfinite(eager).all())
    lane, drv = PU.maps(sc)
    sel = net.select(net._command_trajs(trajs, sc["commands"]), sc["cost_volume"], sc["semantic_pred"], lane, drv, sc["target_points"])
    for b in range(B):
        assert bool((trajs[b] == sel[b]).flatten(1).all(dim=1).any()), b
    eager = eager.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plan()                                              # this stream's workspaces, the stamps and the packed weights exist before the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rows, out = plan()
    rows.zero_()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(rows, trajs)
