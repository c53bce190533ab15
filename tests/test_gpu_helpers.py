"""GPU: the helper kernels around the convolutions (csrc/aux_kernels.hip, depth_softmax_kernel of csrc/lift_splat.hip), each called
directly at the sizes where its own arithmetic branches: the three C == 64 depthwise 7x7 + LayerNorm kernels on either side of their
switches, the ceil-mode pool on all-negative images, bilinear x2 at one-pixel-wide inputs and above the grid cap, channel means with
empty slabs / idle thread rows / one pixel lane, channel broadcast into a slice, the four layout transposes against ``permute``,
LogSigmoid above its grid cap, and every instantiation of the depth softmax.

Every input is a pure function of a name and a seed (workloads.hashfill; the ConvNeXt blocks: torch's seeded generator).  Every reference is plain torch on the CPU in fp64 or an exact
integer / permutation identity.  A bound is either derived beside the test from the arithmetic of the kernel, or it is 4 x the error
that the same formulation has in torch fp32 on the CPU against fp64 on the same inputs (the factor covers another summation order);
those measured errors stand beside their constants."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from util import hashfill, maxabs
from streamingflow_amd._lib import SF_ERR_INVALID, SF_ERR_WORKSPACE

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                                  # fp32 unit roundoff


def _api():
    from streamingflow_amd import _lib, runtime
    return _lib.lib(), runtime.ptr, runtime.stream_ptr()


def _ints(name, shape, lo, hi, seed=0):
    """integer-valued floats in [lo, hi]"""
    return torch.floor(hashfill.uniform(name, shape, lo, hi + 1, seed).double()).clamp_(lo, hi).float()


# ---- 1. depthwise 7x7 + LayerNorm through layers.convolutions.Block --------------------------------------------------------------
BLOCK_TOL = 2e-5      # the bar of test_convnext_mlp_in_one_launch for the same comparison

# (n, H, W) -> the kernel launch_dwconv7_ln picks for C == 64 (csrc/aux_kernels.hip): "lds" below 65536 pixels, above it "pk" (two
# channels per lane) when ceil(H/2) * ceil(W/40) is even and "c64" (one channel per lane, register window) when it is odd
_BLOCK64 = {
    (27, 49, 51): "pk",     # 50 strips per image (the host's reciprocal m_per_img), half-used last row pair, last segment 11 wide
    (70, 31, 33): "pk",     # the 40-wide segment is wider than the image
    (41, 49, 33): "c64",    # 25 x 1 strips: odd; a ragged last 4-row block
    (40, 40, 40): "lds",    # 64000 pixels: below the switch
    (41, 40, 40): "pk",     # 65600 pixels: above it
    (1, 9, 13): "lds",      # ragged 8x8 tiles in both axes
}


def _pk_enabled():
    v = os.environ.get("SF_DWCONV_PK")
    return True if v is None else v.strip() not in ("", "0")


def _dw_route(n, H, W):
    if n * H * W < 65536:
        return "lds"
    return "pk" if _pk_enabled() and (((H + 1) // 2) * ((W + 39) // 40)) % 2 == 0 else "c64"


_BLOCKS = {}


def _block(C):
    """Block(C) as test_convnext_mlp_in_one_launch makes it (seeded default initialisation; random gamma, LayerNorm affine and biases so
    that no term is scaled away; hidden values out to both tails of the GELU).  -> (module on the GPU, its parameters in fp64 on the CPU)"""
    if C not in _BLOCKS:
        import streamingflow_amd.layers.convolutions as Cv
        torch.manual_seed(7000 + C)
        blk = Cv.Block(C, layer_scale_init_value=1.0).eval()
        with torch.no_grad():
            blk.norm.weight.uniform_(0.5, 1.5); blk.norm.bias.uniform_(-0.5, 0.5)
            blk.gamma.uniform_(-1.5, 1.5); blk.pwconv1.bias.uniform_(-1.0, 1.0); blk.pwconv2.bias.uniform_(-1.0, 1.0)
            blk.pwconv1.weight.mul_(3.0)
        p64 = {k: v.detach().double().clone() for k, v in blk.state_dict().items()}
        _BLOCKS[C] = (blk.cuda(), p64)
    return _BLOCKS[C]


def _block_ref(p, x):
    """dwconv -> LayerNorm -> pwconv1 -> GELU -> pwconv2 -> gamma -> residual in fp64"""
    C = x.shape[1]
    xd = x.double()
    y = F.conv2d(xd, p["dwconv.weight"], p["dwconv.bias"], padding=3, groups=C).permute(0, 2, 3, 1)
    y = F.layer_norm(y, (C,), p["norm.weight"], p["norm.bias"], 1e-6)
    y = F.linear(F.gelu(F.linear(y, p["pwconv1.weight"], p["pwconv1.bias"])), p["pwconv2.weight"], p["pwconv2.bias"])
    return xd + (p["gamma"] * y).permute(0, 3, 1, 2)


def _block_run(C, x):
    blk, p64 = _block(C)
    with torch.no_grad():
        got = blk(x.cuda()).cpu()
        ref = _block_ref(p64, x)
    return got, ref


@pytest.mark.parametrize("n,H,W", [(27, 49, 51), (70, 31, 33), (41, 49, 33), (1, 9, 13)])
def test_block64_dwconv_routes_vs_fp64(n, H, W):
    want = _BLOCK64[(n, H, W)]
    assert _dw_route(n, H, W) == (want if want != "pk" or _pk_enabled() else "c64")      # the table above holds by the source's rule
    x = hashfill.normal(f"hb_x_{n}_{H}_{W}", (n, 64, H, W), 10)
    got, ref = _block_run(64, x)
    err = maxabs(got, ref)
    print(f"block64 {(n, H, W)} {_dw_route(n, H, W)}: max-abs vs fp64 = {err:.3e}")
    assert err <= BLOCK_TOL, err


def test_block64_dwconv_switch_pair_agrees():
    """40 and 41 images of 40 x 40 lie on either side of the 65536-pixel switch (LDS-tile kernel / register-window kernel): the same
    weights, the first 40 images the same — both against fp64, and the 40 common images against each other."""
    assert _dw_route(40, 40, 40) == "lds" and _dw_route(41, 40, 40) in ("pk", "c64")
    x = hashfill.normal("hb_x_switch", (41, 64, 40, 40), 11)
    lo, ref_lo = _block_run(64, x[:40].contiguous())
    hi, ref_hi = _block_run(64, x)
    e_lo, e_hi, e_pair = maxabs(lo, ref_lo), maxabs(hi, ref_hi), maxabs(hi[:40], lo)
    print(f"block64 switch pair: low {e_lo:.3e}, high {e_hi:.3e}, low vs high {e_pair:.3e}")
    assert e_lo <= BLOCK_TOL and e_hi <= BLOCK_TOL and e_pair <= BLOCK_TOL, (e_lo, e_hi, e_pair)


@pytest.mark.parametrize("C", [8, 16, 32])
def test_block_narrow_dwconv_instantiations_vs_fp64(C):
    """dwconv7_ln_kernel<8,1>, <16,2>, <32,4> on 2 x 9 x 13: 8x8 tiles ragged in both axes"""
    x = hashfill.normal(f"hb_x_narrow_{C}", (2, C, 9, 13), 12)
    got, ref = _block_run(C, x)
    err = maxabs(got, ref)
    print(f"block{C} (2, 9, 13): max-abs vs fp64 = {err:.3e}")
    assert err <= BLOCK_TOL, err


def test_block64_cases_in_a_child_process_without_the_two_channel_kernel():
    """SF_DWCONV_PK is read once per process: the Block(64) cases of this file again in a fresh process with the two-channel kernel
    switched off — every map of >= 65536 pixels then runs the one-channel register-window kernel, small images and 33-wide ones
    included.  The same oracle, the same tolerance."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env["SF_DWCONV_PK"] = "0"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", "-x",
                        os.path.join(root, "tests", "test_gpu_helpers.py"), "-k", "block64 and not child_process"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=root)
    tail = r.stdout[-1500:] + r.stderr[-1500:]
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, tail


# ---- 2. ceil-mode 2x2 pool on the Bottleneck skip path ----------------------------------------------------------------------------
def _bottleneck(cin, cout):
    import streamingflow_amd.layers.convolutions as Cv
    m = Cv.Bottleneck(cin, cout, downsample=True).eval()
    with torch.no_grad():
        for k, t in m.state_dict().items():
            nm = f"hk_{cin}_{k}"
            if k.endswith("num_batches_tracked"):
                continue
            if k.endswith("running_mean"):
                t.copy_(hashfill.uniform(nm, t.shape, -0.2, 0.2, 1))
            elif k.endswith("running_var"):
                t.copy_(hashfill.uniform(nm, t.shape, 0.5, 1.5, 2))
            elif t.dim() == 4:
                t.copy_(hashfill.uniform(nm, t.shape, -1, 1, 3) * (3.0 / (t.shape[1] * t.shape[2] * t.shape[3])) ** 0.5)
            elif k.endswith("weight"):
                t.copy_(hashfill.uniform(nm, t.shape, 0.5, 1.5, 4))
            else:
                t.copy_(hashfill.uniform(nm, t.shape, -0.5, 0.5, 5))
    return m


def _bottleneck_ref(sd, x):
    """Bottleneck(downsample=True) in the dtype of x: 1x1 / BN / ReLU, 3x3 stride 2 / BN / ReLU, 1x1 / BN / ReLU, plus the skip path:
    zero-pad to even size, MaxPool2d(2), 1x1, BN"""
    p = {k: v.detach().to(x.dtype) for k, v in sd.items()}

    def bn(t, pre):
        return F.batch_norm(t, p[pre + ".running_mean"], p[pre + ".running_var"], p[pre + ".weight"], p[pre + ".bias"], False, 0.0, 1e-5)
    y = F.relu(bn(F.conv2d(x, p["layers.conv_down_project.weight"]), "layers.abn_down_project.0"))
    y = F.relu(bn(F.conv2d(y, p["layers.conv.weight"], stride=2, padding=1), "layers.abn.0"))
    y = F.relu(bn(F.conv2d(y, p["layers.conv_up_project.weight"]), "layers.abn_up_project.0"))
    s = F.max_pool2d(F.pad(x, (0, x.shape[-1] % 2, 0, x.shape[-2] % 2), value=0.0), 2, 2)
    return y + bn(F.conv2d(s, p["projection.conv_skip_proj.weight"]), "projection.bn_skip_proj")


def _negative(name, shape):
    return -(hashfill.normal(name, shape, 21).abs() + 1.0)


# (cin, n, H, W) -> 4 x the max-abs error of _bottleneck_ref in torch fp32 on the CPU against fp64, same weights and input
_BOTTLENECK_BAR = {
    (16, 1, 1, 1): 4 * 1.532e-07,      # max |ref| 1.14
    (16, 2, 5, 7): 4 * 8.985e-07,      # max |ref| 4.97
    (16, 2, 13, 21): 4 * 1.050e-06,    # max |ref| 6.08
    (16, 1, 12, 20): 4 * 1.038e-06,    # max |ref| 6.45
    (6, 2, 5, 7): 4 * 5.936e-07,       # max |ref| 4.02
}


@pytest.mark.parametrize("n,H,W", [(1, 1, 1), (2, 5, 7), (2, 13, 21), (1, 12, 20)])
def test_bottleneck_ceil_pool_on_all_negative_images(n, H, W):
    """The missing row / column of an odd image counts as ZERO in the pool, which only shows where the real values are negative:
    every border window must then give 0, not its largest real value."""
    m = _bottleneck(16, 32)
    x = _negative(f"hk_x_{n}_{H}_{W}", (n, 16, H, W))
    with torch.no_grad():
        ref = _bottleneck_ref(m.state_dict(), x.double())
        got = m.cuda()(x.cuda())
    assert got.shape == (n, 32, (H + 1) // 2, (W + 1) // 2)
    err = maxabs(got, ref)
    print(f"bottleneck16 {(n, H, W)}: max-abs vs fp64 = {err:.3e}, bar {_BOTTLENECK_BAR[(16, n, H, W)]:.3e}")
    assert err <= _BOTTLENECK_BAR[(16, n, H, W)], err


def test_bottleneck_with_channels_not_in_fours_is_right_or_refused():
    """Bottleneck(6, 12): Cin % 4 != 0 and a mid width of 3, while the pool and the convolutions move channels in fours.  Either the
    result agrees with the reference or the call raises — never a silent result with channels missing."""
    n, H, W = 2, 5, 7
    m = _bottleneck(6, 12)
    x = _negative("hk_x_c6", (n, 6, H, W))
    with torch.no_grad():
        ref = _bottleneck_ref(m.state_dict(), x.double())
        try:
            got = m.cuda()(x.cuda())
            torch.cuda.synchronize()
        except (RuntimeError, ValueError) as ex:
            print("Bottleneck(6, 12) refused:", ex)
            return
    err = maxabs(got, ref)
    assert err <= _BOTTLENECK_BAR[(6, n, H, W)], err


# ---- 3. sf_upsample_bilinear2_add_fwd ---------------------------------------------------------------------------------------------
def _upsample(x, skip):
    L, ptr, st = _api()
    n, h, w, c = x.shape
    out = torch.full((n, 2 * h, 2 * w, c), 7.0, device="cuda")
    xg, sg = x.cuda(), (skip.cuda() if skip is not None else None)
    rc = L.sf_upsample_bilinear2_add_fwd(ptr(xg), ptr(sg), ptr(out), n, h, w, c, st)
    assert rc == 0, rc
    return out.cpu()


def _upsample_ref(x, skip):
    r = F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    return r + skip.double() if skip is not None else r


@pytest.mark.parametrize("with_skip", [True, False])
@pytest.mark.parametrize("n,h,w,c", [(1, 1, 1, 4), (2, 1, 5, 8), (1, 3, 1, 12), (2, 7, 9, 64), (1, 130, 130, 64)])
def test_upsample_bilinear2_add_is_exact_on_integers(n, h, w, c, with_skip):
    """Integer inputs in [-64, 64] and weights that are products of 0.25 / 0.75 / 0 / 1: every product and sum is exact in fp32, so
    the kernel must equal the fp64 interpolation bit for bit — one-pixel-high and -wide inputs (both taps clamped onto the same
    pixel), with and without the skip tensor, and 1 081 600 float4 items (above the 4096 x 256 grid: the stride loop)."""
    x = _ints(f"hu_x_{n}_{h}_{w}_{c}", (n, h, w, c), -64, 64, 31)
    skip = _ints(f"hu_s_{n}_{h}_{w}_{c}", (n, 2 * h, 2 * w, c), -64, 64, 32) if with_skip else None
    got, ref = _upsample(x, skip), _upsample_ref(x, skip).float()
    assert torch.equal(got, ref), maxabs(got, ref)


def test_upsample_bilinear2_add_on_normal_inputs():
    """bound: four products, three sums and the skip add, each rounded once, of values no larger than max|in| + max|skip|"""
    n, h, w, c = 2, 7, 9, 64
    x = hashfill.normal("hu_xn", (n, h, w, c), 33)
    skip = hashfill.normal("hu_sn", (n, 2 * h, 2 * w, c), 34)
    bound = 8 * U * (float(x.abs().max()) + float(skip.abs().max()))
    err = maxabs(_upsample(x, skip), _upsample_ref(x, skip))
    print(f"upsample normal: max-abs vs fp64 = {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("c", [6, 0])
def test_upsample_bilinear2_add_refuses_channels_not_in_fours(c):
    L, ptr, st = _api()
    x, out = torch.zeros(64, device="cuda"), torch.zeros(256, device="cuda")
    assert L.sf_upsample_bilinear2_add_fwd(ptr(x), None, ptr(out), 1, 1, 1, c, st) == SF_ERR_INVALID


# ---- 4. sf_channel_mean_fwd -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("HW", [1, 63, 64, 65, 4099])
@pytest.mark.parametrize("C", [4, 12, 96, 1024])
def test_channel_mean_counts_every_pixel_once(C, HW):
    """64 slabs per image: HW < 64 leaves most of them empty (their first pixel beyond the image), C = 12 and 96 leave thread rows
    idle (256 % (C / 4) != 0), C = 1024 has one pixel lane.  Integer inputs in [-8, 8] and 4096 planted at the last pixel of each
    image: every partial sum is an integer below 2^24, exact in any order, so the only roundings are 1 / HW and the product with it:
    |got - ref| <= 2 * 2^-24 * |ref|.  A dropped or doubled pixel is off by >= 1 / HW of an integer: orders of magnitude more."""
    from streamingflow_amd import runtime
    L, ptr, st = _api()
    n = 3
    x = _ints(f"hm_x_{C}_{HW}", (n, HW, C), -8, 8, 41)
    x[:, HW - 1, :] = 4096.0
    ref = x.double().mean(1)
    xg = x.cuda()
    out = torch.full((n, C), 7.0, device="cuda")
    ws = runtime.workspace(L.sf_channel_mean_ws_bytes(C, n), "cuda")
    rc = L.sf_channel_mean_fwd(ptr(xg), ptr(out), n, HW, C, ptr(ws), ws.numel() * 4, st)
    assert rc == 0, rc
    got = out.cpu().double()
    assert float(ref.abs().min()) > 0.0
    worst = float(((got - ref).abs() / ref.abs()).max())
    assert bool(((got - ref).abs() <= 2 * U * ref.abs()).all()), worst


def test_channel_mean_refuses_bad_shapes_and_a_short_workspace():
    L, ptr, st = _api()
    n, HW = 3, 5
    x, out = torch.zeros(n * HW * 1028, device="cuda"), torch.zeros(n * 1028, device="cuda")
    ws = torch.zeros(n * 64 * 1028 + 64, device="cuda")
    assert L.sf_channel_mean_fwd(ptr(x), ptr(out), n, HW, 1028, ptr(ws), ws.numel() * 4, st) == SF_ERR_INVALID
    assert L.sf_channel_mean_fwd(ptr(x), ptr(out), n, HW, 6, ptr(ws), ws.numel() * 4, st) == SF_ERR_INVALID
    need = L.sf_channel_mean_ws_bytes(8, n)
    assert need == n * 64 * 8 * 4
    assert L.sf_channel_mean_fwd(ptr(x), ptr(out), n, HW, 8, ptr(ws), need - 4, st) == SF_ERR_WORKSPACE
    assert L.sf_channel_mean_fwd(ptr(x), ptr(out), n, HW, 8, ptr(ws), need, st) == 0


# ---- 5. sf_broadcast_channels_fwd -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,HW,k,out_cs,out_co", [(3, 1, 4, 4, 0), (2, 37, 12, 20, 8), (2, 40000, 64, 64, 0)])
def test_broadcast_channels_fills_its_slice_and_nothing_else(n, HW, k, out_cs, out_co):
    """the last case has 1 280 000 float4 items: above the 4096 x 256 grid"""
    L, ptr, st = _api()
    vec = hashfill.normal(f"hc_v_{n}_{HW}_{k}", (n, k), 51)
    vg = vec.cuda()
    out = torch.full((n, HW, out_cs), 7.0, device="cuda")
    rc = L.sf_broadcast_channels_fwd(ptr(vg), ptr(out), n, HW, k, out_cs, out_co, st)
    assert rc == 0, rc
    o = out.cpu()
    assert torch.equal(o[..., out_co:out_co + k], vec[:, None, :].expand(n, HW, k))
    rest = torch.cat([o[..., :out_co], o[..., out_co + k:]], -1)
    assert rest.numel() == 0 or float((rest - 7.0).abs().max()) == 0.0


def test_broadcast_channels_refuses_a_slice_outside_the_tensor():
    L, ptr, st = _api()
    vec, out = torch.zeros(64, device="cuda"), torch.zeros(1024, device="cuda")
    assert L.sf_broadcast_channels_fwd(ptr(vec), ptr(out), 1, 4, 8, 12, 8, st) == SF_ERR_INVALID      # out_co + k > out_cs
    assert L.sf_broadcast_channels_fwd(ptr(vec), ptr(out), 1, 4, 6, 12, 0, st) == SF_ERR_INVALID      # k = 6


# ---- 6. layout transposes ---------------------------------------------------------------------------------------------------------
_LAYOUT = [(3, 5, 33), (1, 64, 1), (2, 1, 70), (2, 96, 1023)]


@pytest.mark.parametrize("n,C,HW", _LAYOUT)
def test_layout_transposes_equal_permute(n, C, HW):
    """against ``permute`` (a round trip also passes with a self-inverse bug): ragged 32 x 32 tiles in both axes, one row, one column"""
    L, ptr, st = _api()
    x = hashfill.normal(f"hl_x_{n}_{C}_{HW}", (n, C, HW), 61)
    xg = x.cuda()
    a = torch.full((n, HW, C), 7.0, device="cuda")
    assert L.sf_nchw_to_nhwc(ptr(xg), ptr(a), n, C, HW, st) == 0
    assert torch.equal(a.cpu(), x.permute(0, 2, 1).contiguous())
    yg = x.permute(0, 2, 1).contiguous().cuda()      # [n][HW][C]
    b = torch.full((n, C, HW), 7.0, device="cuda")
    assert L.sf_nhwc_to_nchw(ptr(yg), ptr(b), n, C, HW, st) == 0
    assert torch.equal(b.cpu(), x)


@pytest.mark.parametrize("n,C,HW", _LAYOUT)
def test_strided_layout_transposes_keep_to_their_images(n, C, HW):
    """images src_stride / dst_stride floats apart, both larger than C * HW, the slack on both sides filled with 7.0: the slack of the
    destination stays, the slack of the source does not reach the result"""
    L, ptr, st = _api()
    x = hashfill.normal(f"hl_xs_{n}_{C}_{HW}", (n, C, HW), 62)
    sz, ss, ds = C * HW, C * HW + 5, C * HW + 3

    def run(fn, src_img, want_img):
        src = torch.full((n, ss), 7.0)
        src[:, :sz] = src_img.reshape(n, sz)
        sg = src.cuda()
        dst = torch.full((n, ds), 7.0, device="cuda")
        assert fn(ptr(sg), ss, ptr(dst), ds, n, C, HW, st) == 0
        d = dst.cpu()
        assert torch.equal(d[:, :sz], want_img.reshape(n, sz))
        assert float((d[:, sz:] - 7.0).abs().max()) == 0.0
    xt = x.permute(0, 2, 1).contiguous()
    run(L.sf_nchw_to_nhwc_strided, x, xt)
    run(L.sf_nhwc_to_nchw_strided, xt, x)


def test_strided_layout_transposes_refuse_overlapping_images():
    L, ptr, st = _api()
    a, b = torch.zeros(4096, device="cuda"), torch.zeros(4096, device="cuda")
    for fn in (L.sf_nchw_to_nhwc_strided, L.sf_nhwc_to_nchw_strided):
        assert fn(ptr(a), 5 * 33 - 1, ptr(b), 5 * 33, 3, 5, 33, st) == SF_ERR_INVALID
        assert fn(ptr(a), 5 * 33, ptr(b), 5 * 33 - 1, 3, 5, 33, st) == SF_ERR_INVALID
        assert fn(ptr(a), 5 * 33, ptr(b), 5 * 33, 3, 5, 33, st) == 0


# ---- 7. sf_logsigmoid_fwd ---------------------------------------------------------------------------------------------------------
_LOGSIG_SPECIAL = [0.0, 1e-8, -1e-8, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0]
FLT_MIN = 2.0 ** -126

# The documentation installed with the ROCm toolchain states no ulp errors for expf / log1pf, so the bound is measured: the largest
# error of torch's fp32 F.logsigmoid on the CPU against fp64, relative to max(|ref|, FLT_MIN) (below FLT_MIN a result has absolute,
# not relative, precision), times 4.  The values of every n are the first n of one sequence, and the error is measured over the
# longest (16 777 219 values: the special ones and a dense cover of [-100, 100]) — the largest error among one or 255 values says
# nothing about the function.  Measured: 1.788e-07
LOGSIG_BAR = 4 * 1.788e-07


def _logsig_values(n):
    v = hashfill.uniform("hs_x", (n,), -100, 100, 71)      # a pure function of the index: a shorter case is a prefix of a longer one
    k = min(n, len(_LOGSIG_SPECIAL))
    v[:k] = torch.tensor(_LOGSIG_SPECIAL[:k])
    return v


def _logsig_relerr(got, x):
    ref = F.logsigmoid(x.double())
    return float(((got.double() - ref).abs() / ref.abs().clamp_min(FLT_MIN)).max())


@pytest.mark.parametrize("n", [1, 255, 257, 65536 * 256 + 3])
def test_logsigmoid_vs_fp64(n):
    """one block short of a full one, one element into a second block, and three elements above the 65536-block grid (stride loop)"""
    L, ptr, st = _api()
    x = _logsig_values(n)
    xg = x.cuda()
    out = torch.full((n + 8,), 7.0, device="cuda")
    assert L.sf_logsigmoid_fwd(ptr(xg), ptr(out), n, st) == 0
    o = out.cpu()
    assert float((o[n:] - 7.0).abs().max()) == 0.0
    err = _logsig_relerr(o[:n], x)
    print(f"logsigmoid n={n}: relative error vs fp64 = {err:.3e}, bar {LOGSIG_BAR:.3e}")
    assert err <= LOGSIG_BAR, err


# ---- 8. sf_depth_softmax_fwd ------------------------------------------------------------------------------------------------------
def _softmax_logits(D, fHW):
    rows = 3
    x = hashfill.normal(f"hd_x_{D}_{fHW}", (rows, D, fHW), 81) * 4.0
    x[0, :, 0] = 1.5                        # all-equal ray
    x[1, D // 2, 1] += 80.0                 # one spike
    if D > 1:
        x[2, 0, fHW - 1] = float("-inf")    # -inf beside finite logits
    return x


# (D, fHW) -> 4 x the max-abs error of torch's fp32 softmax on the CPU against fp64 on the same logits.  D = 16 / 32 / 48 / 64 run the
# register-resident instantiations, every other D the three-pass one
_SOFTMAX_BAR = {
    (1, 7): 4 * 0.0, (1, 65): 4 * 0.0,      # one bin: expf(0) / 1, exact
    (5, 7): 4 * 7.513e-08, (5, 65): 4 * 1.566e-07,
    (16, 7): 4 * 1.873e-07, (16, 65): 4 * 2.566e-07,
    (32, 7): 4 * 9.515e-08, (32, 65): 4 * 3.370e-07,
    (41, 7): 4 * 2.903e-07, (41, 65): 4 * 4.667e-07,
    (48, 7): 4 * 1.983e-07, (48, 65): 4 * 3.518e-07,
    (64, 7): 4 * 1.486e-07, (64, 65): 4 * 3.928e-07,
    (80, 7): 4 * 1.473e-07, (80, 65): 4 * 3.903e-07,
}


@pytest.mark.parametrize("fHW", [7, 65])
@pytest.mark.parametrize("D", [1, 5, 16, 32, 41, 48, 64, 80])
def test_depth_softmax_vs_fp64(D, fHW):
    L, ptr, st = _api()
    x = _softmax_logits(D, fHW)
    xg = x.cuda()
    out = torch.full((3, D, fHW), 7.0, device="cuda")
    assert L.sf_depth_softmax_fwd(ptr(xg), ptr(out), 3, D, fHW, st) == 0
    got = out.cpu()
    ref = torch.softmax(x.double(), 1)
    sums = got.double().sum(1)
    assert float((sums - 1.0).abs().max()) <= D * U, float((sums - 1.0).abs().max())
    err = maxabs(got, ref)
    print(f"depth softmax D={D} fHW={fHW}: max-abs vs fp64 = {err:.3e}, bar {_SOFTMAX_BAR[(D, fHW)]:.3e}")
    assert err <= _SOFTMAX_BAR[(D, fHW)], err
