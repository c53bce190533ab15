"""GPU: the ASPP head with its 1x1 branch computed inside the projection launch (csrc/conv_igemm.hip: the producer form of conv_glds_kernel,
csrc/api.hip: deeplab_head) against the same head with the branch as a launch of its own, in one process.

SF_GLDS bits 4 and 5 are re-read at every head: 16 = the producer form where the head qualifies, 32 = the branch and the projection on the
128 x 128 LDS-DMA tile at any pixel count (without it that tile starts at 131072 pixels).  With 32 set, 63 and 47 differ in the producer
form alone.  Both GEMMs keep their chunk and k order, so the two forms must agree to the LAST BIT wherever the producer form runs, and
trivially where it must not (hid = 256, the bf16x3 mode).  Which form ran is read off the profiler: launches under the 128 x 128 AFFINE
key, two for the two-launch form, one for the producer form.

Shapes (C = 64, hid = 128 unless said): one image of 8 x 16 = one exactly full pixel tile; 20 x 36 = five full tiles and a ragged sixth;
three images of 20 x 36 = tiles that straddle image boundaries (the per-image bias and the producer's pixels follow one image index);
C = 32 / 96 = one / three producer chunks; and once 368 x 368 = 135424 pixels, where the planner itself puts the projection on the tile
(SF_GLDS = 31 against 15, nothing forced).

Against torch: the reference formulation (convolutions.py:217-280) in fp64 on the CPU, bound 2e-4 — the bound test_gpu_ops.py's
test_deeplab_head_c64_vs_torch holds the same head to at this width."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from util import maxabs

pytestmark = pytest.mark.gpu
TOL_TORCH = 2e-4
KEY = "conv_glds<128x128w8,affine>"
FUSED, TWO_LAUNCHES = "63", "47"


def _head(C, hid, seed, ncls=8):
    import streamingflow_amd.layers.convolutions as Cv
    torch.manual_seed(seed)
    head = Cv.DeepLabHead(C, ncls, hid).eval()
    with torch.no_grad():
        for m in head.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.7, 1.3); m.bias.uniform_(-0.2, 0.2)
                m.running_mean.uniform_(-0.2, 0.2); m.running_var.uniform_(0.5, 1.5)
    return head


def _reference(head, x, pre=None):
    """fp64 on the CPU; x [n, Cin, H, W]; pre: a bias-free 1x1 in front of the head; also the 1x1 branch's pre-activations"""
    with torch.no_grad():
        d = _head(head.in_channels, head.hidden_channel, 0, head[4].out_channels).double()
        d.load_state_dict({k: v.double() for k, v in head.state_dict().items()})
        d.eval()
        xd = x.double()
        if pre is not None:
            xd = F.conv2d(xd, pre.double())
        aspp = d[0]
        pre0 = aspp.convs[0][1](aspp.convs[0][0](xd))
        outs = [b(xd) for b in list(aspp.convs)[:4]]
        outs.append(F.interpolate(aspp.convs[4](xd), size=xd.shape[-2:], mode="bilinear", align_corners=False))
        return d[4](d[3](d[2](d[1](aspp.project(torch.cat(outs, 1)))))), pre0


def _run(head, st, x_nhwc, glds, planar=False):
    """(output, launches under the 128 x 128 AFFINE key) of one head call under SF_GLDS = glds"""
    from streamingflow_amd import _lib
    L = _lib.lib()
    NK = _lib.SF_PROF_KEYS
    calls, ms = (ctypes.c_int32 * NK)(), (ctypes.c_double * NK)()
    fl, by = (ctypes.c_double * NK)(), (ctypes.c_double * NK)()
    old = os.environ.get("SF_GLDS")
    os.environ["SF_GLDS"] = glds
    L.sf_prof_enable(1)
    try:
        with torch.no_grad():
            if not planar:
                out = head.forward_nhwc(x_nhwc, st)
            else:
                n, h, w, _ = x_nhwc.shape
                cout = st.cls.cout
                out = torch.full((n + 1, cout, h, w), 7.0, device="cuda")      # one spare image: must stay untouched
                head.forward_nhwc_into_planar(x_nhwc, out, 1, cout * h * w, cout * h * w, st)      # image i: plane block i
        torch.cuda.synchronize()
        L.sf_prof_collect(calls, ms, fl, by)
    finally:
        L.sf_prof_enable(0)
        if old is None:
            del os.environ["SF_GLDS"]
        else:
            os.environ["SF_GLDS"] = old
    used = {_lib.KERNEL_NAMES[k]: calls[k] for k in range(NK) if calls[k]}
    return out, used.get(KEY, 0)


def _both_signs(pre0):
    """the ReLU matters: the 1x1 branch's pre-activations (fp64, CPU) are negative for about half the elements, and of both signs within at
    least three channels of four (one image of 128 pixels leaves a few channels on one side of zero)"""
    neg = (pre0 < 0).double().mean().item()
    assert 0.3 <= neg <= 0.7, neg
    per_c = (pre0 < 0).double().mean(dim=(0, 2, 3))
    assert float(((per_c > 0) & (per_c < 1)).double().mean()) >= 0.75, per_c


def _check(C, hid, n, H, W, fused_runs, seed, mode="fp32", fold=False):
    from streamingflow_amd import packing, runtime
    head = _head(C, hid, seed)
    torch.manual_seed(seed + 1)
    pre = torch.randn(C, C, 1, 1) * (1.0 / C) ** 0.5 if fold else None
    x = torch.randn(n, C, H, W)
    x[n - 1] += 0.7                      # different pooled vectors per image
    ref, pre0 = _reference(head, x, pre)
    _both_signs(pre0)
    head = head.cuda()
    packing.set_math_mode(mode)
    try:
        pk = head.pack_after(None if pre is None else pre.cuda())
    finally:
        packing.set_math_mode("fp32")
    xn = runtime.to_nhwc(x.cuda())
    got, k_fused = _run(head, pk.struct, xn, FUSED)
    two, k_two = _run(head, pk.struct, xn, TWO_LAUNCHES)
    assert k_two == 2 and k_fused == (1 if fused_runs else 2), (k_fused, k_two)
    d_forms, d_torch = maxabs(got, two), maxabs(runtime.to_nchw(got), ref)
    print(f"C={C} hid={hid} {n}x{H}x{W} {mode} fold={fold}: fused vs two launches {d_forms:.3e}, vs torch fp64 {d_torch:.3e}")
    assert torch.equal(got, two), d_forms
    assert d_torch <= TOL_TORCH, d_torch
    # the planar-output entry point: images as [cout][H][W] planes, written by the classifier itself
    pl, k_pl = _run(head, pk.struct, xn, FUSED, planar=True)
    pl2, _ = _run(head, pk.struct, xn, TWO_LAUNCHES, planar=True)
    assert k_pl == k_fused
    assert torch.equal(pl, pl2)
    assert float((pl[n] - 7.0).abs().max()) == 0.0
    d_pl = maxabs(pl[:n], ref)
    print(f"    planar: vs torch fp64 {d_pl:.3e}")
    assert d_pl <= TOL_TORCH, d_pl


@pytest.mark.parametrize("C,n,H,W", [(64, 1, 8, 16), (64, 1, 20, 36), (64, 3, 20, 36), (32, 1, 20, 36), (96, 3, 20, 36)],
                         ids=["one_full_tile", "ragged_last_tile", "tiles_across_images", "one_producer_chunk", "three_producer_chunks"])
def test_producer_form_is_the_two_launches_to_the_last_bit(C, n, H, W):
    _check(C, 128, n, H, W, True, 100 + C + n + H)


def test_head_with_a_folded_decoder_in_front():
    """pack_after: the branch weights carry a bias-free 1x1 — other weights, the same launches"""
    _check(64, 128, 3, 20, 36, True, 7, fold=True)


def test_hid_256_keeps_the_two_launches():
    """two cout tiles: the producer would run twice per pixel tile"""
    _check(64, 256, 3, 20, 36, False, 8)


def test_bf16x3_keeps_the_two_launches():
    """the opt-in math mode has its own K loop; its own error (~1e-5) is far inside the bound"""
    _check(64, 128, 3, 20, 36, False, 9, mode="bf16x3")


def test_the_planner_takes_the_producer_form_by_itself():
    """368 x 368 = 135424 pixels: nothing forced, the projection is planned on the 128 x 128 tile and the default (31) fuses; 15 does not"""
    head = _head(64, 128, 11).cuda()
    torch.manual_seed(12)
    xn = torch.randn(1, 368, 368, 64, device="cuda")
    pk = head.pack_after(None)
    got, k = _run(head, pk.struct, xn, "31")
    two, k2 = _run(head, pk.struct, xn, "15")
    assert (k, k2) == (1, 2), (k, k2)
    assert torch.equal(got, two), maxabs(got, two)
