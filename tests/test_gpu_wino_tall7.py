"""conv_wino7t_kernel: the 7x7 + LayerNorm + GELU layer's nine tap groups in the tall-tile arithmetic F(4,3) along y x F(2,3) along x, with the
y-positions left out whose packed weights are zero for every layer (conv_wino.hip; dispatch.hip: wino_tall, SF_WINO_TALL — a LIVE switch,
read at every plan).

Zero positions: rows and columns 0 and 8 of the 9x9 frame around the 7x7 are zero, so U42 is zero at y-position 0 of the groups a = 0, at
y-position 5 of the groups a = 2, at x-position 0 of the groups b = 0 and at x-position 3 of the groups b = 2: 56 of the 216 (group,
position) pairs.  The kernel leaves out the y part of them (two of 18 steps); it may leave out only what the packer writes as zeros.

Layer cases: Bottleblock(128 -> 64) through forward_nhwc three ways on the same tensors — tall (SF_WINO_TALL=1), F(2x2) tap groups
(SF_WINO_TALL=0) and the direct form (a block packed without Winograd weights) — at the bounds test_gpu_wino_tall.py holds for the same
comparison of a layer: <= 5e-5 tall against direct and against F(2x2).  profiles/winograd42_7x7_accuracy_study.json: the block emulated on
the CPU at this data law (fp32 transforms and sums against fp64) stays below half of that.  The block's residual (its 1x1 projection) is
added in the epilogue of its last layer; no caller of the library gives the 7x7 launch itself a residual, so the layer is reached with
two inputs (64 + 64) and with one (128 + 0), both with the block's residual behind it."""
import ctypes
import os

import numpy as np
import pytest
import torch

from util import hashfill, maxabs

pytestmark = pytest.mark.gpu

TALL = "SF_WINO_TALL"
EPI_LNG = 2
BOUND = 5e-5


class _env:
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


def _plan(c0, c1, n, H, W):
    from streamingflow_amd import _lib
    w = _lib.ConvW(w=64, cout=64, cout_pad=64, c0=c0, c1=c1, cin_pad=128, kh=7, kw=7, dil=1, stride=1, pad=3, act=0, w_wino=64, scale=64, bias=64)
    out = (ctypes.c_int32 * _lib.SF_WINO_PLAN_INTS)()
    _lib.check(_lib.lib().sf_debug_wino_plan(ctypes.byref(w), EPI_LNG, n, H, W, 0, 1, 0, out, len(out)), "sf_debug_wino_plan")
    assert out[0] == 1 and out[2] == 1 and out[3] == 4, list(out)      # one launch of 32-tile blocks
    return out[1], out[12]


def test_skipped_positions_are_zero_in_the_packed_weights():
    """U42 of a dense random 7x7 layer, read back: exactly 0.0 at every structurally zero (group, position), a non-zero entry at every other;
    the y-positions the kernel leaves out (conv_wino.hip: chunks of the groups a = 0 run y-positions 1 .. 5, of the groups a = 2 0 .. 4)
    are among the zeros"""
    from streamingflow_amd import packing
    cin = cout = 64
    w = hashfill.uniform("u42z_w", (cout, cin, 7, 7), -1, 1, 5) * (3.0 / (cin * 49)) ** 0.5
    assert float(w.abs().min()) > 0.0
    was = packing.winograd()
    packing.set_winograd(True)
    try:
        pk = packing.Pack(None)
        cw = packing.conv_w(pk, w.cuda(), cin, 0, act="none", dil=1, stride=1, pad=3)
    finally:
        packing.set_winograd(was)
    assert cw.w_wino and cw.cout_pad == cout and cw.cin_pad == cin
    torch.cuda.synchronize()
    blob = pk.keep[-1]
    at = (cw.w_wino - blob.data_ptr()) // 4 + 9 * 16 * cout * cin
    got = blob[at:at + 9 * 24 * cout * cin].cpu().numpy().reshape(9, cin // 16, 24, cout, 16)
    zero = {(g, yp * 4 + xp) for g in range(9) for yp in range(6) for xp in range(4)
            if (g // 3 == 0 and yp == 0) or (g // 3 == 2 and yp == 5) or (g % 3 == 0 and xp == 0) or (g % 3 == 2 and xp == 3)}
    kernel_skips = {(g, yp * 4 + xp) for g in range(9) for yp in range(6) for xp in range(4) if (g // 3 == 0 and yp == 0) or (g // 3 == 2 and yp == 5)}
    assert len(zero) == 56 and len(kernel_skips) == 24 and kernel_skips <= zero
    for g in range(9):
        for pos in range(24):
            blockmax = float(np.abs(got[g, :, pos]).max())
            if (g, pos) in zero:
                assert blockmax == 0.0, (g, pos, blockmax)
            else:
                assert blockmax > 0.0, (g, pos)


# (n, H, W, form: 4 = images concatenated along x, 2 = plain); every one >= 65 536 pixels: the size rule of the tap groups holds
_SHAPES = [
    (27, 37, 67, 4),       # H % 4 = 1: seams between images under every group shift
    (27, 67, 37, 4),       # H % 4 = 3
    (2, 182, 181, 2),      # H % 4 = 2, odd width: half a tall tile below the image
    (6, 104, 106, 2),      # H % 4 = 0
]
_cache = {}


def _block():
    """three Bottleblock(128 -> 64) of the same weights: packed with Winograd weights (run tall and F(2x2)) and without (the direct form)"""
    if "blocks" not in _cache:
        from streamingflow_amd import packing
        from streamingflow_amd.layers.convolutions import Bottleblock
        was = packing.winograd()
        nets = []
        try:
            for wino in (True, False):
                packing.set_winograd(wino)
                m = Bottleblock(128, 64).eval()
                m.load_state_dict(hashfill.fill_state_dict(m.state_dict(), seed=71))
                m = m.cuda()
                m.packed()
                nets.append(m)
        finally:
            packing.set_winograd(was)
        _cache["blocks"] = nets
    return _cache["blocks"]


def _input(si):
    if ("x", si) not in _cache:
        n, H, W, _ = _SHAPES[si]
        _cache["x", si] = hashfill.normal(f"t7_x{si}", (n, H, W, 128), 17).cuda()
    return _cache["x", si]


def _run(net, x, two, tall, wino=True):
    """(a module re-packs when the Winograd switch differs from the one it was packed under: the call runs under the same one)"""
    from streamingflow_amd import packing
    was = packing.winograd()
    packing.set_winograd(wino)
    try:
        gen = net.pack_generation()
        with _env(**{TALL: tall}), torch.no_grad():
            y = net.forward_nhwc(x[..., :64].contiguous(), x[..., 64:].contiguous()) if two else net.forward_nhwc(x)
            torch.cuda.synchronize()
        assert net.pack_generation() == gen and bool(net.packed().struct.c7.w_wino) == wino
    finally:
        packing.set_winograd(was)
    return y


@pytest.mark.parametrize("two", [True, False], ids=["64+64", "128+0"])
@pytest.mark.parametrize("si", range(len(_SHAPES)))
def test_tall_tap_groups_against_f22_and_the_direct_form(si, two):
    n, H, W, form = _SHAPES[si]
    assert n * H * W >= 65536
    c0, c1 = (64, 64) if two else (128, 0)
    with _env(**{TALL: 1}):
        assert _plan(c0, c1, n, H, W) == (form, 1)
    with _env(**{TALL: 0}):
        assert _plan(c0, c1, n, H, W) == (form, 0)
    wino, direct = _block()
    x = _input(si)
    tall, f22, dr = _run(wino, x, two, 1), _run(wino, x, two, 0), _run(direct, x, two, 0, wino=False)
    d_dir, d_f22 = maxabs(tall, dr), maxabs(tall, f22)
    print(f"{n}x{H}x{W} {c0}+{c1}: output up to {float(tall.abs().max()):.2f}, tall vs direct {d_dir:.3e}, tall vs F(2x2) {d_f22:.3e}, "
          f"F(2x2) vs direct {maxabs(f22, dr):.3e}")
    assert torch.isfinite(tall).all()
    assert d_dir <= BOUND, d_dir
    assert d_f22 <= BOUND, d_f22
    if si == 0:      # reproducibility: a second run of the case is bitwise equal
        again = _run(wino, x, two, 1)
        assert torch.equal(tall, again)
