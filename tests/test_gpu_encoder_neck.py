"""GPU: the camera encoder neck (streamingflow_amd/models/encoder.py -> sf_camera_neck_fwd, csrc/camera_neck.hip) against the float64
reference of tests/encoder_neck_util.py on every channel and pixel, at shapes the kernels underneath had not seen: 160 / 216 / 56 / 48
and 112 / 152 / 40 / 20 channels, images smaller than the ASPP dilations.

  case       images  hi -> lo            D   what it exercises
  b4_14x30   2       14x30 -> 28x60      48  the per-camera shape: rate 36 collapsed to its centre tap, rate 24 dead along y only, cin_pad 224
  b4_5x9     1       5x9 -> 10x18        48  every dilated branch collapsed; the upsampling clamps on every row and column; 180 pixels, not
                                             a multiple of the softmax tile
  b0_38x40   3       38x40 -> 76x80      20  nothing collapses; 18 240 second-stage pixels reach the batched kernels; another D

Bound: 8 x the float32 REFERENCE's own max error against float64 (from the fixture, per output and case), + 2e-5 when the
profiler shows a launch of the chain on a kernel with a Winograd form."""
import ctypes

import pytest
import torch

import encoder_neck_util as U
from encoder_neck_util import GEN
from util import hashfill, maxabs

pytestmark = pytest.mark.gpu


def _profiled(fn):
    from streamingflow_amd import _lib
    L = _lib.lib()
    NK = _lib.SF_PROF_KEYS
    calls, ms = (ctypes.c_int32 * NK)(), (ctypes.c_double * NK)()
    fl, by = (ctypes.c_double * NK)(), (ctypes.c_double * NK)()
    L.sf_prof_enable(1)
    try:
        r = fn()
        torch.cuda.synchronize()
        L.sf_prof_collect(calls, ms, fl, by)
    finally:
        L.sf_prof_enable(0)
    return r, {_lib.KERNEL_NAMES[k] for k in range(NK) if calls[k]}


def _device(name, collapse=True):
    net = U.build(name).cuda()
    net.collapse = collapse
    hi, lo = (t.cuda() for t in GEN.endpoints(name))
    return net, hi, lo


def _nchw(name, rays, planar):
    c = GEN.CASES[name]
    n, H2, W2 = c["n"], 2 * c["H"], 2 * c["W"]
    return rays.view(n, H2, W2, -1).permute(0, 3, 1, 2), planar.view(n, c["D"], H2, W2)


def _check(name, collapse):
    from streamingflow_amd.models.encoder import dead_rates
    net, hi, lo = _device(name, collapse)
    (rays, logits, prob), used = _profiled(lambda: net.neck_nhwc(hi, lo))
    ref = U.reference(name)
    c = GEN.CASES[name]
    dead = dead_rates((12, 24, 36), c["H"], c["W"]) if collapse else ()
    branches = net.packed(c["H"], c["W"]).struct.branch      # the pack that ran: 1x1 where collapsed, dilated 3x3 elsewhere
    assert [(b.kh, b.dil) for b in branches] == [(1, 1)] + [(1, 1) if r in dead else (3, r) for r in (12, 24, 36)]
    # the small-P kernel reports one name for its direct and its Winograd form
    wino = any(k.startswith("conv_wino<") or k.startswith("conv_sp<") for k in used)
    tol = U.tolerance(name, wino)
    feat, depth = _nchw(name, rays, logits)
    err = (maxabs(feat, ref[0]), maxabs(depth, ref[1]), maxabs(prob.view_as(depth), ref[2]))
    print(name, "collapse" if collapse else "full 3x3", "max |device - float64| feature %.3e depth %.3e prob %.3e, bounds %.3e %.3e %.3e, kernels %s"
          % (err + tol + (sorted(used),)))
    assert bool(torch.isfinite(rays).all()) and bool(torch.isfinite(logits).all())
    assert all(e <= t for e, t in zip(err, tol)), (name, err, tol)
    return rays, logits, prob


@pytest.mark.parametrize("name", U.CASES)
def test_neck_vs_fp64(name):
    from streamingflow_amd.models.encoder import dead_rates
    c = GEN.CASES[name]
    assert dead_rates((12, 24, 36), c["H"], c["W"]) == {"b4_14x30": (36,), "b4_5x9": (12, 24, 36), "b0_38x40": ()}[name]
    _check(name, True)


@pytest.mark.parametrize("name", ["b4_14x30", "b4_5x9"])
def test_collapsed_and_full_dilated_branches_agree(name):
    """the same head packed with every dilated branch as a full 3x3: the same bound, and the two packs differ by rounding only"""
    a = _check(name, True)
    b = _check(name, False)
    tol = U.tolerance(name)
    diff = tuple(maxabs(x, y) for x, y in zip(a, b))
    print(name, "max |collapsed - full| feature %.3e depth %.3e prob %.3e" % diff)
    assert all(d <= 2 * t for d, t in zip(diff, tol)), (diff, tol)      # each within the bound of the same reference


def test_neck_equals_neck_nhwc_bitwise():
    name = "b4_5x9"
    net, hi, lo = _device(name)
    rays, logits, _ = net.neck_nhwc(hi, lo)
    feat, depth = net.neck(hi, lo)
    want_f, want_d = _nchw(name, rays, logits)
    assert feat.is_contiguous() and tuple(feat.shape) == (1, 64, 10, 18) and tuple(depth.shape) == (1, 48, 10, 18)
    assert torch.equal(feat, want_f) and torch.equal(depth, want_d)


def test_graph_capture_replays_bitwise():
    name = "b4_14x30"
    net, hi, lo = _device(name)
    eager = [t.clone() for t in net.neck_nhwc(hi, lo)]      # also packs the weights: nothing but the chain is captured
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = net.neck_nhwc(hi, lo)
    for t in out:
        t.fill_(-7.0)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, eager))


@pytest.mark.parametrize("D", [20, 48, 128])
@pytest.mark.parametrize("fHW", [35, 64, 180])
def test_depth_softmax_planar(fHW, D):
    """sf_depth_softmax_planar_fwd alone against torch float64: the input is a channel slice of a wider tensor, logits reach +-80 (the max
    subtraction matters), short and tail tiles.  Bound: expf and the division round to about an ulp each, the D-term sum to (D - 1) ulp
    at worst, and x - max carries |x - max| 2^-24 into the exponent, where p |x - max| <= 1 / e: (D + 24) 2^-24 covers them."""
    from streamingflow_amd import _lib, runtime
    rows, cs, co = 3, D + 12, 8
    x = hashfill.normal("dsp_x", (rows * fHW, cs), 61, std=3.0)
    spikes = hashfill.uniform("dsp_s", (rows * fHW, cs), 0.0, 1.0, 62)
    x = torch.where(spikes > 0.97, torch.full_like(x, 80.0), torch.where(spikes < 0.03, torch.full_like(x, -80.0), x)).cuda()
    lead, fill = 64, -777.25
    bufs = [torch.full((lead + rows * D * fHW + lead,), fill, dtype=torch.float32, device="cuda") for _ in range(2)]
    outs = [b[lead:lead + rows * D * fHW].view(rows, D, fHW) for b in bufs]
    rc = _lib.lib().sf_depth_softmax_planar_fwd(runtime.ptr(x), cs, co, runtime.ptr(outs[0]), runtime.ptr(outs[1]), rows, D, fHW,
                                                runtime.stream_ptr(x.device))
    torch.cuda.synchronize()
    assert rc == 0
    want = x[:, co:co + D].view(rows, fHW, D).permute(0, 2, 1)
    assert float(want.max()) == 80.0 and float(want.min()) == -80.0
    assert torch.equal(outs[0], want)
    err = maxabs(outs[1], want.double().softmax(1))
    print("rows %d fHW %d D %d: max |prob - float64| %.3e" % (rows, fHW, D, err))
    assert err <= (D + 24) * 2.0 ** -24
    for b in bufs:
        assert bool((b[:lead] == fill).all()) and bool((b[-lead:] == fill).all())


@pytest.mark.parametrize("D", [50, 132])
def test_depth_softmax_planar_refuses_before_writing(D):
    from streamingflow_amd import _lib, runtime
    rows, fHW, cs = 2, 70, 136
    x = torch.zeros((rows * fHW, cs), dtype=torch.float32, device="cuda")
    outs = [torch.full((rows, D, fHW), -777.25, dtype=torch.float32, device="cuda") for _ in range(2)]
    rc = _lib.lib().sf_depth_softmax_planar_fwd(runtime.ptr(x), cs, 0, runtime.ptr(outs[0]), runtime.ptr(outs[1]), rows, D, fHW,
                                                runtime.stream_ptr(x.device))
    torch.cuda.synchronize()
    assert rc == _lib.SF_ERR_UNSUPPORTED
    assert all(bool((o == -777.25).all()) for o in outs)


def test_lift_splat_takes_the_necks_layouts():
    """lift_splat(rays_nhwc=, depth_prob=) on the neck's outputs against the existing call on the same data (b = 1, two frames of one
    camera: the temporal blend runs).  Fed the existing softmax's probabilities the BEV is bitwise the existing call's.  Fed the neck's
    own probabilities it differs only through the order of the softmax's D-term sum: each probability within 2 (D - 1) 2^-24 relative, so
    each BEV cell within that fraction of the same lift of |features| — a bound from the arithmetic, not from the result."""
    from streamingflow_amd import _lib, runtime
    from streamingflow_amd.models.lift_splat import LiftSplat
    from lift_util import rig_cameras
    name = "b4_14x30"
    c = GEN.CASES[name]
    net, hi, lo = _device(name)
    rays, logits, prob = net.neck_nhwc(hi, lo)
    s, D, fH, fW = c["n"], c["D"], 2 * c["H"], 2 * c["W"]
    lift = LiftSplat(final_dim=(8 * fH, 8 * fW)).cuda()
    intr, extr, ego = (t.cuda() for t in rig_cameras(s, 1, (8 * fH, 8 * fW), 3))
    feat, depth = _nchw(name, rays, logits)
    feat, depth = feat.contiguous().view(1, s, 1, -1, fH, fW), depth.view(1, s, 1, D, fH, fW)
    old = lift.lift_splat(feat, depth, intr, extr, ego)
    assert float(old.abs().max()) > 1.0
    prob_old = torch.empty_like(prob)
    _lib.check(_lib.lib().sf_depth_softmax_fwd(runtime.ptr(logits), runtime.ptr(prob_old), s, D, fH * fW, runtime.stream_ptr(prob.device)), "softmax")
    assert torch.equal(lift.lift_splat(None, depth, intr, extr, ego, rays_nhwc=rays, depth_prob=prob_old), old)
    new = lift.lift_splat(None, depth, intr, extr, ego, rays_nhwc=rays, depth_prob=prob)
    scale = lift.lift_splat(feat.abs(), depth, intr, extr, ego)
    gap = (new.double() - old.double()).abs()
    rel = 2.0 * (D - 1) * 2.0 ** -24
    print("lift: max |new - existing| %.3e, largest allowed %.3e" % (float(gap.max()), rel * float(scale.max())))
    assert bool((gap <= rel * scale.double() + 1e-30).all())


def test_model_hands_the_neck_to_the_lift():
    """streamingflow.calculate_birds_eye_view_features with an Encoder attached: same BEV as the (features, depth_logits) route fed the
    neck's NCHW outputs, depth_prediction [b, s, n, D, fH, fW], cam_front of the present frame's camera 1."""
    from streamingflow_amd.models import streamingflow as SF
    from lift_util import rig_cameras
    name = "b4_5x9"
    net, hi, lo = _device(name)

    class Ends(torch.nn.Module):      # a stand-in trunk: hands every image the case's endpoints, shifted per image
        def forward(self, x):
            k = torch.arange(x.shape[0], device=x.device, dtype=torch.float32).view(-1, 1, 1, 1)
            return hi + 0.25 * k, lo - 0.125 * k

    net.backbone = Ends()
    cfg = SF.default_cfg()
    cfg.IMAGE.FINAL_DIM = (80, 144)
    cfg.MODEL.MODALITY.USE_LIDAR = False
    cfg.N_FUTURE_FRAMES = 0
    model = SF.streamingflow(cfg, encoder=net)
    assert model.encoder is net and SF.streamingflow(cfg).encoder is None
    model.lift.cuda()                   # the camera path up to the BEV only: the later stages have their own tests
    model.planning_enabled = True       # cam_front without building the planner
    b, s, n = 1, 1, 2
    intr, extr, ego = (t.cuda() for t in rig_cameras(s, n, (80, 144), 5))
    images = torch.zeros((b, s, n, 3, 80, 144), device="cuda")
    x, depth, cam_front = model.calculate_birds_eye_view_features(images, intr, extr, ego)
    f, d = net(images.view(b * s * n, 3, 80, 144))
    x2, depth2, cam2 = model.calculate_birds_eye_view_features((f.view(b, s, n, 64, 10, 18), d.view(b, s, n, 48, 10, 18)), intr, extr, ego)
    assert tuple(depth.shape) == (b, s, n, 48, 10, 18) and torch.equal(depth, depth2)
    assert tuple(cam_front.shape) == (b, 64, 10, 18) and torch.equal(cam_front, cam2)
    scale = model.lift.lift_splat(f.view(b, s, n, 64, 10, 18).abs(), depth2, intr, extr, ego)
    assert bool(((x.double() - x2.double()).abs() <= 2.0 * 47 * 2.0 ** -24 * scale.double() + 1e-30).all())
