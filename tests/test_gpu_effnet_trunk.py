"""GPU: the EfficientNet trunk (streamingflow_amd/models/efficientnet.py -> sf_effnet_trunk_fwd, csrc/effnet.hip) against the float64
restatement of tests/effnet_util.py: every kernel alone, every kind of MBConv block, whole trunks.

Bound everywhere (the rule of tests/encoder_neck_util.tolerance): 8 x the float32 restatement's own max error against float64 on the same
inputs, computed here on the CPU per output — it depends on depth and fill and is not fixed in advance.  The channel sums of the
depthwise launch are integers and are checked exactly.

Measured on the MI355X (b4, 2 x 3 x 32 x 48; profiles/effnet_trunk_parity.json has every trunk case): max |device - float64| 4.0e-07 on
reduction_4 and 3.9e-07 on reduction_3, bounds 1.8e-06 and 3.2e-06."""
import ctypes
from types import SimpleNamespace as NS

import pytest
import torch
import torch.nn.functional as F

import effnet_util as U
import encoder_neck_util as NU
from util import hashfill, maxabs

pytestmark = pytest.mark.gpu

FILL = -777.25
FX = 2.0 ** 24


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2)


def guarded(shape, dtype=torch.float32, lead=64):
    """(view of `shape`, whole buffer): the view sits between two guard bands a kernel must not touch."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((lead + n + lead,), FILL if dtype.is_floating_point else -7, dtype=dtype, device="cuda")
    return buf[lead:lead + n].view(shape), buf


def guards_intact(buf, lead=64):
    fill = FILL if buf.dtype.is_floating_point else -7
    return bool((buf[:lead] == fill).all()) and bool((buf[-lead:] == fill).all())


def call(name, *args, scratch=None):
    from streamingflow_amd import runtime
    return runtime.call(name, *args, device=torch.device("cuda"), scratch=scratch)


def status(fn, *args):
    from streamingflow_amd import _lib, runtime
    rc = getattr(_lib.lib(), fn)(*args, runtime.stream_ptr(torch.device("cuda")))
    torch.cuda.synchronize()
    return rc


def make_block(name, k, stride, cin, cout, expand, cse, pad):
    """(MBConvW on the device, its Pack, float32 CPU state under prefix 'b.') of one hashed MBConv block; pad = (top, left, bottom, right)."""
    from streamingflow_amd import _lib, packing
    from streamingflow_amd.models import efficientnet as E
    m = E.MBConvBlock(NS(k=k, stride=stride, cin=cin, cout=cout, expand=expand, cse=cse, skip=stride == 1 and cin == cout))
    sd = hashfill.fill_state_dict({name + "." + key: v for key, v in m.state_dict().items()}, seed=U.SEED, gain=U.GAIN)
    sd = {key[len(name) + 1:]: v for key, v in sd.items()}
    m.load_state_dict(sd)
    m = m.cuda().eval()
    pk = packing.Pack(_lib.MBConvW())
    with torch.no_grad():
        E.pack_mbconv(pk, m, pad, pk.struct)
    return pk.struct, pk, {"b." + key: v for key, v in sd.items()}


def both(fn):
    """fn(dtype) -> tensor(s): (float64 result, bound = 8 x the float32 result's error) per output."""
    with torch.no_grad():
        r64, r32 = fn(torch.float64), fn(torch.float32)
    if torch.is_tensor(r64):
        r64, r32 = (r64,), (r32,)
    return r64, U.tolerance(r64, r32)


# ---- single kernels ----------------------------------------------------------------------------------------------------------------------
def _pads(k, which):
    return ((k - 1) // 2, (k - 1) // 2) if which == "sym" else which


@pytest.mark.parametrize("which", ["sym", (0, 1), (1, 2), (2, 2)])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("k", [3, 5])
def test_depthwise_and_channel_sums(k, stride, which):
    """7 x 9 and 12 x 10: odd and even; 4 x 11: shorter than the 5 x 5 window, which reaches past the image on one side or both."""
    from streamingflow_amd.runtime import ptr
    a, b = _pads(k, which)
    for C in (8, 24, 144):
        w, pk, sd = make_block("dw%d_%d" % (k, C), k, stride, C, 8, 1, max(1, C // 4), (a, a, b, b))
        for H, W in ((7, 9), (12, 10), (4, 11)):
            x = hashfill.normal("dw_x_%d_%d_%d" % (C, H, W), (2, C, H, W), 81)
            assert float((x[0] - x[1]).abs().max()) > 1.0
            ref = lambda dt: U.swish(U.bn({kk: v.to(dt) for kk, v in sd.items()}, "b._bn1", F.conv2d(
                F.pad(x.to(dt), (a, b, a, b)), sd["b._depthwise_conv.weight"].to(dt), stride=stride, groups=C)))
            (want,), (tol,) = both(ref)
            Ho, Wo = want.shape[2:]
            assert (Ho, Wo) == ((H + a + b - k) // stride + 1, (W + a + b - k) // stride + 1)
            out, obuf = guarded((2, Ho, Wo, C))
            sums, sbuf = guarded((2, C), torch.int64)
            xd = nhwc(x).cuda()
            call("effnet_dwconv", ctypes.byref(w), ptr(xd), ptr(out), ptr(sums), 2, H, W)
            torch.cuda.synchronize()
            err = maxabs(nchw(out).cpu(), want)
            print("dw k%d s%d pads %s C %d %dx%d: max |device - float64| %.3e bound %.3e" % (k, stride, (a, b), C, H, W, err, tol))
            assert err <= tol
            # the sums are integers: exactly the fixed-point images of what the launch wrote, summed per image and channel
            fixed = torch.round(out.double().cpu() * FX).to(torch.int64).sum((1, 2))
            assert torch.equal(sums.cpu(), fixed)
            assert guards_intact(obuf) and guards_intact(sbuf)


@pytest.mark.parametrize("planar", [1, 0])
@pytest.mark.parametrize("shape", [(2, 3, 13, 18), (2, 3, 16, 20)])
def test_stem(shape, planar):
    from streamingflow_amd.models.efficientnet import EfficientNetTrunk
    from streamingflow_amd.runtime import ptr
    for version in ("b4", "b0"):
        sd = U.trunk_state(version)
        t = EfficientNetTrunk(version)
        t.load_state_dict(sd)
        t = t.cuda().eval()
        x = U.images("stem", shape)
        ref = lambda dt: (lambda r: U.swish(r._bn0(r._conv_stem(x.to(dt)))))(U.RefTrunk(sd, version, dtype=dt))
        (want,), (tol,) = both(ref)
        n, _, H, W = shape
        out, obuf = guarded((n,) + tuple(want.shape[2:]) + (t.c_stem,))
        img = x.cuda() if planar else nhwc(x).cuda()
        call("effnet_stem", ctypes.byref(t.packed(H, W).struct), ptr(img), planar, ptr(out), n, H, W)
        torch.cuda.synchronize()
        err = maxabs(nchw(out).cpu(), want)
        print("stem %s %s planar %d: max |device - float64| %.3e bound %.3e" % (version, shape, planar, err, tol))
        assert err <= tol and guards_intact(obuf)


@pytest.mark.parametrize("C,cse", [(8, 1), (24, 6), (48, 12)])
def test_se_gate(C, cse):
    from streamingflow_amd.runtime import ptr
    w, pk, sd = make_block("se%d" % cse, 3, 1, C, 8, 1, cse, (1, 1, 1, 1))
    n, HW = 3, 35
    y = hashfill.normal("se_y_%d" % C, (n, HW, C), 82)
    sums = torch.round(y.double() * FX).to(torch.int64).sum(1)

    def ref(dt):
        s = {k: v.to(dt) for k, v in sd.items()}
        mean = (sums.double() / FX / HW).to(dt).view(n, C, 1, 1)
        sq = U.swish(F.conv2d(mean, s["b._se_reduce.weight"], s["b._se_reduce.bias"]))
        return torch.sigmoid(F.conv2d(sq, s["b._se_expand.weight"], s["b._se_expand.bias"])).view(n, C)
    (want,), (tol,) = both(ref)
    gate, gbuf = guarded((n, C))
    sd_ = sums.cuda()
    call("effnet_se_gate", ctypes.byref(w), ptr(sd_), ptr(gate), n, HW)
    torch.cuda.synchronize()
    err = maxabs(gate.cpu(), want)
    print("se gate C %d squeezed %d: max |device - float64| %.3e bound %.3e" % (C, cse, err, tol))
    assert float(want.std()) > 1e-3 and err <= tol and guards_intact(gbuf)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("cout", [24, 56])
@pytest.mark.parametrize("cin", [48, 144])
def test_gated_projection(cin, cout, residual):
    """Three images of 7 x 9 (189 pixels: three tiles, the last short, images changing inside a tile); every image has its own gate and
    the last one's is all zeros: its output is exactly the BatchNorm bias (+ the residual)."""
    from streamingflow_amd import _lib, packing
    from streamingflow_amd.runtime import ptr
    n, H, W = 3, 7, 9
    conv, bnm = torch.nn.Conv2d(cin, cout, 1, bias=False), torch.nn.BatchNorm2d(cout, eps=1e-3)
    tag = "proj_%d_%d" % (cin, cout)
    for mod, name in ((conv, tag + ".conv."), (bnm, tag + ".bn.")):
        filled = hashfill.fill_state_dict({name + k: v for k, v in mod.state_dict().items()}, seed=U.SEED, gain=U.GAIN)
        mod.load_state_dict({k[len(name):]: v for k, v in filled.items()})
    conv, bnm = conv.cuda(), bnm.cuda().eval()
    pk = packing.Pack(_lib.ConvW())
    with torch.no_grad():
        sc, bi = packing.bn_fold(bnm)
        w = packing.conv_w(pk, conv.weight, cin, scale=sc, bias=bi)
    assert (w.cin_pad, w.cout_pad) == ((cin + 31) // 32 * 32, (cout + 15) // 16 * 16) and w.cin_pad != cin
    x = hashfill.normal(tag + "_x", (n, cin, H, W), 83)
    gate = hashfill.uniform(tag + "_g", (n, cin), 0.05, 0.95, 84)
    gate[2] = 0.0
    res = hashfill.normal(tag + "_r", (n, cout, H, W), 85) if residual else None
    sd = {"bn." + k: v.cpu() for k, v in bnm.state_dict().items()}

    def ref(dt):
        y = U.bn({k: v.to(dt) for k, v in sd.items() if v.is_floating_point()}, "bn", F.conv2d(x.to(dt) * gate.to(dt).view(n, cin, 1, 1), conv.weight.detach().cpu().to(dt)))
        return y + res.to(dt) if residual else y
    (want,), (tol,) = both(ref)
    out, obuf = guarded((n, H, W, cout))
    xd, gd, r = nhwc(x).cuda(), gate.cuda(), nhwc(res).cuda() if residual else None      # named: alive until the launch has run
    call("effnet_pointwise", ctypes.byref(w), ptr(xd), ptr(gd), ptr(r), ptr(out), 0, n, H * W)
    torch.cuda.synchronize()
    err = maxabs(nchw(out).cpu(), want)
    print("projection %d -> %d residual %d: max |device - float64| %.3e bound %.3e" % (cin, cout, residual, err, tol))
    assert err <= tol and guards_intact(obuf)
    exact = bi.view(1, 1, cout).expand(H, W, cout)
    assert torch.equal(out[2], exact + r[2] if residual else exact)
    assert float((out[0] - out[1]).abs().max()) > 0.1


# ---- blocks and trunks ---------------------------------------------------------------------------------------------------------------
def device_trunk(version, size="nominal"):
    from streamingflow_amd.models.efficientnet import NOMINAL, EfficientNetTrunk
    t = EfficientNetTrunk(version, 8, image_size=NOMINAL if size == "nominal" else size)
    t.load_state_dict(U.trunk_state(version))
    return t.cuda().eval()


@pytest.mark.parametrize("i,kind", [(0, "ratio 1, no expand conv"), (1, "ratio 1, skip"), (2, "stride 2, no skip"), (3, "stride 1, skip"),
                                    (6, "5x5 stride 2"), (7, "5x5, skip")])
def test_mbconv_block(i, kind):
    """Blocks of the b4 trunk with its static pads, on 2 x 9 x 11 inputs; the workspace is exactly what the query says."""
    from streamingflow_amd import _lib
    from streamingflow_amd.runtime import ptr
    t = device_trunk("b4")
    a = t.blocks_args[i]
    assert (a.expand == 1, a.stride, a.skip, a.k) == {0: (True, 1, False, 3), 1: (True, 1, True, 3), 2: (False, 2, False, 3), 3: (False, 1, True, 3),
                                                       6: (False, 2, False, 5), 7: (False, 1, True, 5)}[i]
    n, H, W = 2, 9, 11
    x = hashfill.normal("mb_x_%d" % i, (n, a.cin, H, W), 86)
    sd = U.trunk_state("b4")
    ref = lambda dt: U.RefTrunk(sd, "b4", dtype=dt)._blocks[i](x.to(dt))
    (want,), (tol,) = both(ref)
    blk = t.packed(H, W).blocks[i]
    need = _lib.lib().sf_mbconv_ws_bytes(ctypes.byref(blk), n, H, W)
    assert need > 0 and need % 256 == 0
    ws, wbuf = guarded((need // 4,))
    out, obuf = guarded((n,) + tuple(want.shape[2:]) + (a.cout,))
    xd = nhwc(x).cuda()
    call("mbconv", ctypes.byref(blk), ptr(xd), ptr(out), n, H, W, scratch=ws)
    torch.cuda.synchronize()
    err = maxabs(nchw(out).cpu(), want)
    print("b4 block %d (%s): max |device - float64| %.3e bound %.3e" % (i, kind, err, tol))
    assert err <= tol and guards_intact(obuf) and guards_intact(wbuf)


TRUNKS = [("b4", (2, 3, 32, 48), "nominal"), ("b4", (1, 3, 40, 56), "nominal"), ("b0", (2, 3, 32, 32), "nominal"), ("b4", (1, 3, 37, 51), None)]


@pytest.mark.parametrize("version,shape,size", TRUNKS)
def test_trunk_vs_fp64(version, shape, size):
    t = device_trunk(version, size)
    x = U.images("trunk", shape)
    sd = U.trunk_state(version)
    want, tol = both(lambda dt: U.RefTrunk(sd, version, 8, size, dt).walk(x))
    if shape == (2, 3, 32, 48):
        assert tuple(want[0].shape[1:]) == (160, 2, 3) and tuple(want[1].shape[1:]) == (56, 4, 6)
    if size is None:      # static and dynamic padding differ on this size
        assert device_trunk(version).pads() != t.pads(*shape[2:])
        other = U.RefTrunk(sd, version, 8, "nominal").walk(x)
        assert other[0].shape != want[0].shape or maxabs(other[0], want[0]) > 100 * tol[0]
    hi, lo = t(x.cuda())
    torch.cuda.synchronize()
    assert tuple(hi.shape) == tuple(want[0].shape) and tuple(lo.shape) == tuple(want[1].shape) and hi.is_contiguous()
    err = (maxabs(hi.cpu(), want[0]), maxabs(lo.cpu(), want[1]))
    print("trunk %s %s image_size %s: max |device - float64| hi %.3e lo %.3e, bounds %.3e %.3e, max |y| %.2f %.2f"
          % (version, shape, size, err[0], err[1], tol[0], tol[1], float(want[0].abs().max()), float(want[1].abs().max())))
    assert bool(torch.isfinite(hi).all()) and all(e <= b for e, b in zip(err, tol)), (err, tol)
    # the NHWC form holds the same numbers
    hi2, lo2 = t.endpoints_nhwc(x.cuda())
    assert torch.equal(nchw(hi2), hi) and torch.equal(nchw(lo2), lo)


def test_eager_runs_and_graph_replay_are_bitwise_equal():
    t = device_trunk("b4")
    x = U.images("trunk", (2, 3, 32, 48)).cuda()
    first = [o.clone() for o in t.endpoints_nhwc(x)]      # also packs the weights: nothing but the chain is captured
    second = t.endpoints_nhwc(x)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = t.endpoints_nhwc(x)
    for o in out:
        o.fill_(-7.0)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, first))


def _encoder():
    from streamingflow_amd.models import streamingflow as SF
    cfg = SF.default_cfg()
    cfg.IMAGE.FINAL_DIM = (32, 48)
    cfg.MODEL.MODALITY.USE_LIDAR = False
    cfg.N_FUTURE_FRAMES = 0
    enc = SF.camera_encoder(cfg)
    neck = {k: v for k, v in enc.state_dict().items() if not k.startswith("backbone.")}
    sd = dict(NU.GEN.hashed_state(neck))
    sd.update(U.state("b4"))
    enc.load_state_dict(sd, strict=True)
    return cfg, enc.cuda().eval(), {k: v for k, v in sd.items() if not k.startswith("backbone.")}


def test_encoder_from_images_and_the_model_takes_them():
    """Encoder(backbone=EfficientNetTrunk("b4")) on images against the float64 neck fed the float64 restatement's endpoints; the bound is
    the neck's: 8 x the error of the same chain in float32, + the Winograd allowance.  Then the model accepts images with that encoder."""
    from streamingflow_amd.models import streamingflow as SF
    from lift_util import rig_cameras
    cfg, enc, neck_sd = _encoder()
    x = U.images("trunk", (2, 3, 32, 48))
    tsd = U.trunk_state("b4")
    chain = lambda dt: NU.GEN.neck_f64(neck_sd, *U.RefTrunk(tsd, "b4", dtype=dt).walk(x), dtype=dt)
    want, tol = both(chain)
    tol = tuple(v + NU.WINO_ALLOWANCE for v in tol)
    rays, logits, prob = enc.forward_nhwc(x.cuda())
    torch.cuda.synchronize()
    feat = nchw(rays.view(2, 4, 6, 64)).cpu()
    err = (maxabs(feat, want[0]), maxabs(logits.view(2, 48, 4, 6).cpu(), want[1]), maxabs(prob.view(2, 48, 4, 6).cpu(), want[2]))
    print("encoder from images: max |device - float64| feature %.3e depth %.3e prob %.3e, bounds %.3e %.3e %.3e" % (err + tol))
    assert all(e <= b for e, b in zip(err, tol)), (err, tol)
    f, d = enc(x.cuda())
    assert torch.equal(f, nchw(rays.view(2, 4, 6, 64))) and torch.equal(d, logits.view(2, 48, 4, 6))
    model = SF.streamingflow(cfg, encoder=enc)
    assert model.encoder is enc and SF.streamingflow(cfg).encoder is None
    model.lift.cuda()
    b, s, n = 1, 1, 2
    intr, extr, ego = (t.cuda() for t in rig_cameras(s, n, (32, 48), 5))
    images = x.cuda().view(b, s, n, 3, 32, 48)
    bev, depth, cam_front = model.calculate_birds_eye_view_features(images, intr, extr, ego)
    assert tuple(depth.shape) == (b, s, n, 48, 4, 6) and torch.equal(depth, d.view(b, s, n, 48, 4, 6)) and cam_front is None
    assert bev.shape[0] == b and bool(torch.isfinite(bev).all()) and float(bev.abs().max()) > 0


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    from streamingflow_amd import _lib
    from streamingflow_amd.runtime import ptr
    L = _lib.lib()
    t = device_trunk("b4")
    n, H, W = 2, 32, 48
    x = U.images("trunk", (n, 3, H, W)).cuda()
    pk = t.packed(H, W)
    need = L.sf_effnet_trunk_ws_bytes(ctypes.byref(pk.struct), n, H, W)
    ws = torch.full((need // 4,), FILL, dtype=torch.float32, device="cuda")
    hi = torch.full((n, 2, 3, 160), FILL, dtype=torch.float32, device="cuda")
    lo = torch.full((n, 4, 6, 56), FILL, dtype=torch.float32, device="cuda")
    run = lambda b: status("sf_effnet_trunk_fwd", ctypes.byref(pk.struct), ptr(x), 1, ptr(hi), ptr(lo), n, H, W, ptr(ws), b)
    untouched = lambda: all(bool((v == FILL).all()) for v in (hi, lo, ws))
    blk = pk.blocks[3]
    for field, bad in (("k", 7), ("k", 4), ("stride", 3), ("stride", 0), ("cexp", blk.cexp + 4), ("cout", blk.cout + 4), ("cin", blk.cin + 4)):
        good = getattr(blk, field)
        setattr(blk, field, bad)
        rc = run(need)
        setattr(blk, field, good)
        assert rc == _lib.SF_ERR_UNSUPPORTED and untouched(), (field, bad, rc)
    good, pk.struct.c_stem = pk.struct.c_stem, 44
    rc = run(need)
    pk.struct.c_stem = good
    assert rc == _lib.SF_ERR_UNSUPPORTED and untouched()
    for short in (need - 256, need // 2, 0):
        assert run(short) == _lib.SF_ERR_WORKSPACE and untouched(), short
    assert status("sf_effnet_trunk_fwd", ctypes.byref(pk.struct), ptr(x), 1, ptr(hi), ptr(lo), n, H, W, None, need) == _lib.SF_ERR_WORKSPACE
    assert untouched()
    # and with exactly the queried size it runs: the query is what the call carves
    assert run(need) == _lib.SF_OK
    want = t.endpoints_nhwc(x)
    assert torch.equal(hi, want[0]) and torch.equal(lo, want[1])
