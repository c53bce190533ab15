"""conv_wino5t_kernel: the tall-tile Winograd arithmetic, F(4,3) along y x F(2,3) along x, on the 32-tile blocks of the plain / concatenated
AFFINE and BLEND launches (conv_wino.hip; dispatch.hip: wino_tall, SF_WINO_TALL — a LIVE switch, read at every plan).  Every case runs
three ways on the same tensors: tall (SF_WINO_TALL=1), F(2x2, 3x3) (SF_WINO_TALL=0) and the direct form.  Bounds, the project's own for a
Winograd layer: <= 2e-4 against torch (asserted inside test_gpu_conv_random._run), <= 5e-5 tall against direct and against F(2x2); cell
level <= 2e-5.  Every case asserts through sf_debug_wino_plan that its launch is 32-tile blocks (>= 1 000 workgroups) in the tall form
with the switch on and in F(2x2) with it off, so that none can silently test the other path."""
import ctypes
import os

import numpy as np
import pytest
import torch

from util import hashfill, maxabs

pytestmark = pytest.mark.gpu

TALL, SPLIT = "SF_WINO_TALL", "SF_WINO_SPLIT_WGS"


class _env:
    """the switches are read at every plan of a launch: set some for the calls inside the block"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.was = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.was.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _plan(c0, c1, cout, n, H, W, in_up=0, epi=0, flags=0):
    """sf_debug_wino_plan under the switches in force: ([(tile rows per block, first tile row, tile rows, workgroups)], tall bits)"""
    from streamingflow_amd import _lib
    cin = c0 + c1
    w = _lib.ConvW(w=64, cout=cout, cout_pad=(cout + 15) // 16 * 16, c0=c0, c1=c1, cin_pad=(cin + 31) // 32 * 32, kh=3, kw=3, dil=1, stride=1,
                   pad=1, act=0, w_wino=64)
    out = (ctypes.c_int32 * _lib.SF_WINO_PLAN_INTS)()
    _lib.check(_lib.lib().sf_debug_wino_plan(ctypes.byref(w), epi, n, H, W, in_up, 1, flags, out, len(out)), "sf_debug_wino_plan")
    assert out[0] == 1
    return [tuple(out[3 + 4 * s:7 + 4 * s]) for s in range(out[2])], out[12]


def _whole_on_32_tile_blocks(layer):
    """the layer as ONE launch of >= 1 000 workgroups on 32-tile blocks (call with SF_WINO_SPLIT_WGS=0): tall with the switch on, not with it off"""
    with _env(**{TALL: 1}):
        segs, tall = _plan(**layer)
        assert len(segs) == 1 and segs[0][0] == 4 and segs[0][3] >= 1000 and tall == 1, (segs, tall)
    with _env(**{TALL: 0}):
        segs0, tall0 = _plan(**layer)
        assert segs0 == segs and tall0 == 0, (segs0, tall0)
    return segs[0]


# the smallest shapes that can break it (every one a whole layer on 32-tile blocks: SF_WINO_SPLIT_WGS=0 keeps the ragged last block row tall)
_CASES = [
    dict(c0=64, c1=0, cout=64, n=64, H=50, W=50),        # 25 tile rows (rows % 4 = 1), concatenated images with odd cn0 (25 tile columns per image)
    dict(c0=32, c1=32, cout=128, n=40, H=53, W=50),      # 27 tile rows (rows % 4 = 3), odd H: the last tall tile is half outside the image; two sources
    dict(c0=64, c1=0, cout=64, n=6, H=181, W=187),       # the plain form, odd in both axes
    dict(c0=128, c1=0, cout=128, n=4, H=200, W=200),     # the wide concatenated form at 200x200
    dict(c0=256, c1=0, cout=64, n=64, H=50, W=50),       # cin = 256: the longest K loop of the forward
]
_FORMS = [4, 4, 2, 4, 4]      # 4: images concatenated along x, 2: plain


def _three_ways(c, seed, layer):
    from test_gpu_conv_random import _run
    with _env(**{TALL: 1}):
        tall = _run(c, seed, wino=True)        # (asserts <= 2e-4 against torch)
    with _env(**{TALL: 0}):
        f22 = _run(c, seed, wino=True)
    direct = _run(c, seed, wino=False)
    d_dir, d_f22 = maxabs(tall, direct), maxabs(tall, f22)
    print(f"{layer}: tall vs direct {d_dir:.3e}, tall vs F(2x2) {d_f22:.3e}, F(2x2) vs direct {maxabs(f22, direct):.3e}")
    assert d_dir <= 5e-5, d_dir
    assert d_f22 <= 5e-5, d_f22
    return tall


@pytest.mark.parametrize("i", range(len(_CASES)))
def test_tall_layer_against_f22_and_the_direct_form(i):
    from util import wino_plan
    c = dict(k=3, stride=1, dil=1, pad=1, act=["relu", "none", "lrelu", "tanh"][i % 4], add=i % 3 != 1, after=i % 2 == 0, in_slack=8 * (i % 2),
             out_slack=[0, 4, 16][i % 3])
    c.update(_CASES[i])
    layer = {k: c[k] for k in ("c0", "c1", "cout", "n", "H", "W")}
    with _env(**{SPLIT: 0}):
        assert wino_plan(**layer)["form"] == _FORMS[i], "the case no longer exercises the form it was chosen for"
        seg = _whole_on_32_tile_blocks(layer)
        assert seg[2] == (c["H"] + 1) // 2
        _three_ways(c, 900 + i, layer)


def test_tall_main_launch_joins_the_f22_remainder_rows():
    """the split layer (25 tile rows: 24 on 32-tile blocks in the tall form, one on 16-tile blocks in F(2x2)) with the switch on"""
    i = 0
    c = dict(k=3, stride=1, dil=1, pad=1, act="relu", add=True, after=True, in_slack=0, out_slack=0)
    c.update(_CASES[i])
    layer = {k: c[k] for k in ("c0", "c1", "cout", "n", "H", "W")}
    with _env(**{SPLIT: 1}):
        with _env(**{TALL: 1}):
            segs, tall = _plan(**layer)
            assert [s[:3] for s in segs] == [(4, 0, 24), (2, 24, 1)] and tall == 1, (segs, tall)      # bit 0: the main launch alone
        _three_ways(c, 900 + i, layer)


def _module_three_ways(run, bound):
    """run(net) on three nets of the same weights: packed with Winograd weights under SF_WINO_TALL=1 / 0, and without them"""
    from util import build_pair, cases
    from streamingflow_amd import packing
    dt = cases.timeset("shipped")[3]

    def build(wino, tall):
        was = packing.winograd()
        packing.set_winograd(wino)
        try:
            net, sd = build_pair(64, "euler", True, True, dt)
            with _env(**{TALL: tall}), torch.no_grad():
                y = run(net, sd)
                torch.cuda.synchronize()
            return y
        finally:
            packing.set_winograd(was)
    on, off, direct = build(True, 1), build(True, 0), build(False, 0)
    for a, b, d in zip(on, off, direct):
        print(f"tall vs F(2x2) {maxabs(a, b):.3e}, tall vs direct {maxabs(a, d):.3e}")
        assert a.shape == b.shape and maxabs(a, b) <= bound, maxabs(a, b)
        assert maxabs(a, d) <= bound, maxabs(a, d)
    return on


def test_tall_pool2_epilogue():
    """The MaxPool2d(2) taken over the 2x2 tile in the epilogue of a 64 -> 64 layer on 16 frames of 100x100.  Only SmallEncoder reaches that
    epilogue (block 0's second convolution), so the test runs an encoder whose layers BEHIND block 0 pass its pooled output through: the
    residual branches of blocks 1 - 4 are switched off (their last BatchNorm has weight = bias = 0), the projections and the last
    convolution's centre tap copy channels, and the closing tanh(y / 8) is undone on the host (|y / 8| stays below 1: atanh is well
    conditioned, ~1e-6 in y).  What is compared is therefore block 0's output (both of its layers run tall) after the encoder's second
    pooling, at the bounds of a single layer; the encoder's own output also against torch."""
    from oracle import ref_torch as R
    from streamingflow_amd import packing
    from streamingflow_amd.layers.res_models import SmallEncoder
    x = hashfill.normal("tall_pool_x", (16, 64, 100, 100), 31)
    S = 0.125

    def weights(m):
        sd = hashfill.fill_state_dict(m.state_dict(), seed=78)
        for k in list(sd):
            blk = k.split(".")[1] if k.startswith("blocks.") else None
            if blk in ("1", "2", "3", "4") and (k.endswith("conv_2.norm.weight") or k.endswith("conv_2.norm.bias")):
                sd[k] = torch.zeros_like(sd[k])
            elif k.endswith("projection.weight"):
                sd[k] = torch.eye(sd[k].shape[0], sd[k].shape[1]).reshape(sd[k].shape)
            elif k.endswith("projection.bias") or k in ("last_conv.0.norm.bias", "last_conv.0.norm.running_mean"):
                sd[k] = torch.zeros_like(sd[k])
            elif k == "last_conv.0.conv.weight":
                w = torch.zeros_like(sd[k])
                w[:, :, 1, 1] = torch.eye(w.shape[0], w.shape[1])
                sd[k] = w
            elif k == "last_conv.0.norm.weight":
                sd[k] = torch.full_like(sd[k], S)
            elif k == "last_conv.0.norm.running_var":
                sd[k] = torch.ones_like(sd[k])
        return sd
    sd = None

    def build(wino, tall):
        nonlocal sd
        was = packing.winograd()
        packing.set_winograd(wino)
        try:
            m = SmallEncoder(64, 64, 64).eval()
            sd = weights(m)
            m.load_state_dict(sd)
            m = m.cuda()
            with _env(**{TALL: tall}), torch.no_grad():
                y = m(x.cuda())
                torch.cuda.synchronize()
            return y.cpu()
        finally:
            packing.set_winograd(was)
    with _env(**{SPLIT: 0}):
        _whole_on_32_tile_blocks(dict(c0=64, c1=0, cout=64, n=16, H=100, W=100, flags=2))
        on, off, direct = build(True, 1), build(True, 0), build(False, 0)
    with torch.no_grad():
        want = R.small_encoder({"e." + k: v for k, v in sd.items()}, "e", x)
    assert maxabs(on, want) <= 2e-4, maxabs(on, want)
    assert float(on.abs().max()) < 0.9      # inside the range where the tanh is undone exactly enough
    back = lambda t: torch.atanh(t.double()) / S
    print(f"pooled block output up to {float(back(on).abs().max()):.2f}: tall vs F(2x2) {maxabs(back(on), back(off)):.3e}, "
          f"tall vs direct {maxabs(back(on), back(direct)):.3e}, F(2x2) vs direct {maxabs(back(off), back(direct)):.3e}")
    assert maxabs(back(on), back(off)) <= 5e-5 and maxabs(back(on), back(direct)) <= 5e-5


def test_tall_upsampled_patch_reads_and_half_size_skip():
    """SmallDecoder of filter size 128 (at the shipped 64 the layer has 728 workgroups and runs on 16-tile blocks) on 8 latents of 25x25:
    block 4 (128 -> 128) reads its 50x50 input upsampled on the fly to 100x100 (in_up: the first convolution's patch loads; add_up: the
    identity skip in the second convolution's epilogue, one half-size source pixel per 2x2 tile)"""
    from oracle import ref_torch as R
    from streamingflow_amd import packing
    from streamingflow_amd.layers.res_models import SmallDecoder
    z = hashfill.normal("tall_up_z", (8, 64, 25, 25), 32) * 0.5
    sd = None

    def build(wino, tall):
        nonlocal sd
        was = packing.winograd()
        packing.set_winograd(wino)
        try:
            m = SmallDecoder(64, 64, 128, False).eval()
            sd = hashfill.fill_state_dict(m.state_dict(), seed=77)
            m.load_state_dict(sd)
            m = m.cuda()
            with _env(**{TALL: tall}), torch.no_grad():
                y = m(z.cuda())
                torch.cuda.synchronize()
            return y
        finally:
            packing.set_winograd(was)
    with _env(**{SPLIT: 0}):
        _whole_on_32_tile_blocks(dict(c0=128, c1=0, cout=128, n=8, H=50, W=50, in_up=1))
        _whole_on_32_tile_blocks(dict(c0=128, c1=0, cout=128, n=8, H=100, W=100, flags=2))
        on, off, direct = build(True, 1), build(True, 0), build(False, 0)
    with torch.no_grad():
        want = R.small_decoder({"d." + k: v for k, v in sd.items()}, "d", z)
    print(f"tall vs F(2x2) {maxabs(on, off):.3e}, tall vs direct {maxabs(on, direct):.3e}, tall vs torch {maxabs(on, want):.3e}")
    assert maxabs(on, off) <= 5e-5 and maxabs(on, direct) <= 5e-5, (maxabs(on, off), maxabs(on, direct))
    assert maxabs(on, want) <= 2e-4, maxabs(on, want)


@pytest.mark.parametrize("B,h,w", [(32, 50, 50), (2, 200, 200)])
def test_tall_gates_with_second_output_and_blend(B, h, w):
    """The conv-GRU cell as in test_gpu_wino_split.test_gates_with_second_output_and_blend: [update ; reset] gates (AFFINE with the reset
    gate's second output) and the candidate with the state blend (BLEND) through SpatialGRU.forward_nhwc, then infer_state (its SE-scaled
    3x3 layers run tall, the sampling layer and the 7x7 tap groups keep F(2x2)): tall on against off and against direct, <= 2e-5 each"""
    C = 64
    with _env(**{TALL: 1}):      # the gates launch under the split rule in force: its 32-tile launch is tall
        segs, tall = _plan(c0=C, c1=C, cout=2 * C, n=B, H=h, W=w, flags=4)
        assert segs[0][0] == 4 and (tall & 1) and sum(s[3] for s in segs) >= 1000, (segs, tall)
    x = (hashfill.normal("wt_x", (3, B, h, w, C), 11) * 0.5)
    s0 = (hashfill.normal("wt_s", (B, h, w, C), 12) * 0.5)

    def run(net, sd):
        gru, ode = net.spatial_grus[0], net.gru_ode
        ode.noise = hashfill.HashedNoise(3)
        y = gru.forward_nhwc(x.cuda(), s0.cuda())
        p, q = ode.infer_state(s0.cuda().permute(0, 3, 1, 2).contiguous())
        return y, p, q
    _module_three_ways(run, 2e-5)


@pytest.mark.parametrize("k,cin,cout", [(3, 64, 64), (7, 64, 64)])
def test_packed_u42_against_fp64(k, cin, cout):
    """the second transformed copy behind sf_conv_w::w_wino: U42[group][cin / 16][yp * 4 + xp][cout_pad][16] = G4 g G2^T (7x7: the nine 3x3
    groups of the 9x9 frame), read back and compared with fp64 on the host: <= 1e-6 of the largest element"""
    from streamingflow_amd import packing
    w = hashfill.uniform(f"u42_w_{k}", (cout, cin, k, k), -1, 1, 3) * (3.0 / (cin * k * k)) ** 0.5
    was = packing.winograd()
    packing.set_winograd(True)
    try:
        pk = packing.Pack(None)
        cw = packing.conv_w(pk, w.cuda(), cin, 0, act="none", dil=1, stride=1, pad=k // 2)
    finally:
        packing.set_winograd(was)
    assert cw.w_wino and cw.cout_pad == cout and cw.cin_pad == cin
    torch.cuda.synchronize()
    blob = pk.keep[-1]
    ngrp = 9 if k == 7 else 1
    at = (cw.w_wino - blob.data_ptr()) // 4 + ngrp * 16 * cout * cin
    got = blob[at:at + ngrp * 24 * cout * cin].cpu().double().numpy().reshape(ngrp, cin // 16, 24, cout, 16)
    G4 = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]])
    G2 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]])
    frame = np.zeros((cout, cin, 9, 9))
    if k == 7:
        frame[:, :, 1:8, 1:8] = w.double().numpy()
    want = np.zeros_like(got)
    for grp in range(ngrp):
        ga, gb = divmod(grp, 3)
        g = frame[:, :, 3 * ga:3 * ga + 3, 3 * gb:3 * gb + 3] if k == 7 else w.double().numpy()
        U = np.einsum("ai,ocij,bj->ocab", G4, g, G2).reshape(cout, cin // 16, 16, 24)      # [co][kc][cl][yp * 4 + xp]
        want[grp] = U.transpose(1, 3, 0, 2)
    err, big = float(np.abs(got - want).max()), float(np.abs(want).max())
    print(f"U42 {k}x{k}: max-abs error {err:.3e}, largest element {big:.3e}")
    assert err <= 1e-6 * big, (err, big)
