"""EfficientNet trunk of the camera ``Encoder`` on the MI355X: images to the two endpoints the neck reads.

The reference's encoder walks a third-party ``efficientnet_pytorch.EfficientNet`` (streamingflow/models/encoder.py:19, :64-105): stem,
MBConv blocks up to the version's break index, an endpoint recorded whenever the resolution drops.  The architecture is public, small
and fixed; ``EfficientNetTrunk`` restates it with ``efficientnet_pytorch``'s attribute names — ``_conv_stem``, ``_bn0``,
``_blocks.<i>.{_expand_conv,_bn0,_depthwise_conv,_bn1,_se_reduce,_se_expand,_project_conv,_bn2}`` — so the ``encoder.backbone.*`` keys of a
released checkpoint load with ``strict=True``.  The head (``_conv_head``, ``_bn1``, ``_fc``) and the blocks behind the break index do not
exist, as the reference deletes them (encoder.py:44-62).

The whole trunk is ONE library call (``sf_effnet_trunk_fwd``, csrc/effnet.hip): stem, then per block expand 1x1, depthwise with the SE's
channel sums in the same launch, the SE gate, and the projection that multiplies the gate into its input as it loads.

Padding follows ``efficientnet_pytorch`` 0.7.x: ``EfficientNet.from_pretrained`` builds STATIC "same" padding from the version's nominal
image size (380 for b4), not from the actual input — per layer with nominal input size s: o = ceil(s / stride),
p = max((o - 1) * stride + k - s, 0), p // 2 in front and p - p // 2 behind, and the next layer's nominal size is o.
``image_size=None`` selects dynamic "same" padding from the actual input (``from_name`` without a size).

Inference only: ``.eval()`` is required.  No CPU fallback: CPU tensors raise.
"""
import ctypes
import math
from types import SimpleNamespace as NS

import torch
import torch.nn as nn

from .. import _lib, packing, runtime
from ..runtime import ptr
from .encoder import BREAK_INDEX, REDUCTION_CHANNEL

# efficientnet_pytorch utils.py: (kernel, repeats, in, out, expand, stride) per stage; se_ratio 0.25 everywhere
BASE_STAGES = [(3, 1, 32, 16, 1, 1), (3, 2, 16, 24, 6, 2), (5, 2, 24, 40, 6, 2), (3, 3, 40, 80, 6, 2), (5, 3, 80, 112, 6, 1),
               (5, 4, 112, 192, 6, 2), (3, 1, 192, 320, 6, 1)]
# version -> (width, depth, nominal image size)
SCALING = {"b0": (1.0, 1.0, 224), "b4": (1.4, 1.8, 380), "b7": (2.0, 3.1, 600)}
STEM_FILTERS, SE_RATIO, BN_EPS = 32, 0.25, 1e-3
NOMINAL = "nominal"


def round_filters(filters, width, divisor=8):
    """Channel counts scale by the width and round to multiples of 8, never below 90 % of the scaled count."""
    filters *= width
    new = max(divisor, int(filters + divisor / 2) // divisor * divisor)
    if new < 0.9 * filters:
        new += divisor
    return int(new)


def round_repeats(repeats, depth):
    return int(math.ceil(depth * repeats))


def block_args(version, downsample=8):
    """The trunk's blocks in order, ``NS(k, stride, cin, cout, expand, cse, skip)``: every block of the version, or the blocks up to the
    break index at downsample 8 (encoder.py:44-56)."""
    width, depth, _ = SCALING[version]
    blocks = []
    for k, r, cin, cout, expand, stride in BASE_STAGES:
        cin, cout = round_filters(cin, width), round_filters(cout, width)
        for i in range(round_repeats(r, depth)):
            ci, s = (cin, stride) if i == 0 else (cout, 1)
            blocks.append(NS(k=k, stride=s, cin=ci, cout=cout, expand=expand, cse=max(1, int(ci * SE_RATIO)), skip=s == 1 and ci == cout))
    return blocks[:BREAK_INDEX[version] + 1] if downsample == 8 else blocks


def same_pad(size, k, stride):
    """-> (nominal output size, pad in front, pad behind) of TensorFlow "same" padding on an input of ``size``."""
    o = -(-size // stride)
    p = max((o - 1) * stride + k - size, 0)
    return o, p // 2, p - p // 2


def layer_pads(blocks, size):
    """(top, left, bottom, right) of the stem and of every block's depthwise layer, "same" padding computed on a ``size`` = (h, w) input:
    the nominal size (static padding) or the actual one (dynamic)."""
    h, w = size
    pads = []
    for k, stride in [(3, 2)] + [(b.k, b.stride) for b in blocks]:
        (h, t, bt), (w, l, r) = same_pad(h, k, stride), same_pad(w, k, stride)
        pads.append((t, l, bt, r))
    return pads


def walk_shapes(blocks, c_stem, pads, H, W):
    """[(C, h, w)] after the stem and after every block on an H x W image, and the producers of the endpoints by the reference's rule
    (encoder.py:83-101): the tensor in front of every block that lowers the height, then the last output.  Producer -1 is the stem."""
    out = lambda s, k, stride, a, b: (s + a + b - k) // stride + 1
    h, w = out(H, 3, 2, pads[0][0], pads[0][2]), out(W, 3, 2, pads[0][1], pads[0][3])
    shapes, ends = [(c_stem, h, w)], []
    for i, (b, (t, l, bt, r)) in enumerate(zip(blocks, pads[1:])):
        h2, w2 = out(h, b.k, b.stride, t, bt), out(w, b.k, b.stride, l, r)
        if h > h2:
            ends.append(i - 1)
        h, w = h2, w2
        shapes.append((b.cout, h, w))
    ends.append(len(blocks) - 1)
    return shapes, ends


class MBConvBlock(nn.Module):
    """The parameters of one MBConv block under ``efficientnet_pytorch``'s names (model.py: MBConvBlock)."""

    def __init__(self, a):
        super().__init__()
        self.args = a
        cexp = a.cin * a.expand
        if a.expand != 1:
            self._expand_conv = nn.Conv2d(a.cin, cexp, 1, bias=False)
            self._bn0 = nn.BatchNorm2d(cexp, eps=BN_EPS)
        self._depthwise_conv = nn.Conv2d(cexp, cexp, a.k, stride=a.stride, groups=cexp, bias=False)
        self._bn1 = nn.BatchNorm2d(cexp, eps=BN_EPS)
        self._se_reduce = nn.Conv2d(cexp, a.cse, 1)
        self._se_expand = nn.Conv2d(a.cse, cexp, 1)
        self._project_conv = nn.Conv2d(cexp, a.cout, 1, bias=False)
        self._bn2 = nn.BatchNorm2d(a.cout, eps=BN_EPS)

    def forward(self, x):
        raise RuntimeError("MBConvBlock holds parameters only: the blocks run inside EfficientNetTrunk (sf_effnet_trunk_fwd)")


def pack_mbconv(pk, m, pad, b=None):
    """Fill the ``_lib.MBConvW`` ``b`` (a new one by default) from the ``MBConvBlock`` ``m`` with the depthwise pads (top, left, bottom,
    right); ``pk`` (a ``packing.Pack``) owns the packed tensors."""
    a, b = m.args, _lib.MBConvW() if b is None else b
    cexp = a.cin * a.expand
    if a.expand != 1:
        sc, bi = packing.bn_fold(m._bn0)
        b.expand = packing.conv_w(pk, m._expand_conv.weight, a.cin, scale=sc, bias=bi)
    sc, bi = packing.bn_fold(m._bn2)
    b.project = packing.conv_w(pk, m._project_conv.weight, cexp, scale=sc, bias=bi)
    b.dw_w = pk.hold(m._depthwise_conv.weight.detach()[:, 0].permute(1, 2, 0).reshape(a.k * a.k, cexp))      # [ky][kx] rows, channels along a row
    b.dw_scale, b.dw_bias = (pk.hold(t) for t in packing.bn_fold(m._bn1))
    b.se_reduce_w, b.se_reduce_b = pk.hold(m._se_reduce.weight.detach().reshape(a.cse, cexp)), pk.hold(m._se_reduce.bias)
    b.se_expand_w, b.se_expand_b = pk.hold(m._se_expand.weight.detach().reshape(cexp, a.cse)), pk.hold(m._se_expand.bias)
    b.cin, b.cexp, b.cout, b.cse, b.k, b.stride, b.skip = a.cin, cexp, a.cout, a.cse, a.k, a.stride, int(a.skip)
    b.pad_t, b.pad_l, b.pad_b, b.pad_r = pad
    return b


class EfficientNetTrunk(nn.Module):
    """``Encoder(cfg, D, backbone=EfficientNetTrunk("b4"))``: [N, 3, H, W] -> (reduction_{k+1}, reduction_k), k = log2(downsample)."""

    def __init__(self, version, downsample=8, image_size=NOMINAL):
        super().__init__()
        if version not in SCALING:
            raise NotImplementedError("EfficientNet version %r: b0 / b4 / b7 only" % (version,))
        self.version, self.downsample = version, int(downsample)
        self.index = int(math.log2(self.downsample))
        if 2 ** self.index != self.downsample or not 1 <= self.index < len(REDUCTION_CHANNEL[version]) - 1:
            raise NotImplementedError("EfficientNetTrunk: downsample must be 2, 4, 8 or 16")
        if image_size == NOMINAL:
            image_size = SCALING[version][2]
        self.image_size = None if image_size is None else (tuple(image_size) if isinstance(image_size, (tuple, list)) else (int(image_size),) * 2)
        self.blocks_args = block_args(version, self.downsample)
        self.c_stem = round_filters(STEM_FILTERS, SCALING[version][0])
        self._conv_stem = nn.Conv2d(3, self.c_stem, 3, stride=2, bias=False)
        self._bn0 = nn.BatchNorm2d(self.c_stem, eps=BN_EPS)
        self._blocks = nn.ModuleList([MBConvBlock(a) for a in self.blocks_args])

    def __getstate__(self):
        return runtime.strip_runtime_state(self.__dict__)

    # ---- geometry ---------------------------------------------------------------------------------------------------
    def pads(self, H=None, W=None):
        """The four pads of the stem and of every depthwise layer: static (from ``image_size``) or, with ``image_size=None``, from H x W."""
        return layer_pads(self.blocks_args, self.image_size or (H, W))

    def plan(self, H, W):
        """-> (pads, (C, h, w) of reduction_{k+1}, (C, h, w) of reduction_k) on an H x W image."""
        pads = self.pads(H, W)
        shapes, ends = walk_shapes(self.blocks_args, self.c_stem, pads, H, W)
        if len(ends) < self.index + 1 or min(min(s[1:]) for s in shapes) < 1:
            raise ValueError("EfficientNetTrunk: a %d x %d image is too small to reach reduction_%d" % (H, W, self.index + 1))
        return pads, shapes[ends[self.index] + 1], shapes[ends[self.index - 1] + 1]

    # ---- packing ----------------------------------------------------------------------------------------------------
    def _pack(self, pads):
        if self.training:
            raise RuntimeError("streamingflow_amd is inference-only: call .eval() (BatchNorm uses running statistics)")
        pk = packing.Pack(_lib.EffNetW())
        s = pk.struct
        s.stem_w = pk.hold(self._conv_stem.weight.detach().permute(2, 3, 1, 0).reshape(27, self.c_stem))      # [ky][kx][c] rows, cout along a row
        s.stem_scale, s.stem_bias = (pk.hold(t) for t in packing.bn_fold(self._bn0))
        s.c_stem, s.n_blocks, s.index = self.c_stem, len(self._blocks), self.index
        s.pad_t, s.pad_l, s.pad_b, s.pad_r = pads[0]
        arr = (_lib.MBConvW * len(self._blocks))()
        for b, m, pad in zip(arr, self._blocks, pads[1:]):
            pack_mbconv(pk, m, pad, b)
        pk.blocks = arr      # the struct points into it
        s.blocks = ctypes.cast(arr, ctypes.POINTER(_lib.MBConvW))
        return pk

    def packed(self, H, W):
        """The packed trunk: re-packed when a parameter changed (as PackedModule); one copy per padding, i.e. one in all with static
        padding and one per image size with ``image_size=None``."""
        sig = (packing.math_mode(), packing.winograd()) + tuple((p.data_ptr(), p._version, p.device)
                                                                 for p in list(self.parameters()) + list(self.buffers()))
        cache = self.__dict__.get("_sf_trunk_packs")
        if cache is None or cache[0] != sig:
            self.__dict__["_sf_trunk_packs"] = cache = (sig, {})
        key = None if self.image_size else (H, W)
        if key not in cache[1]:
            runtime.require_cuda(self._conv_stem.weight)
            with torch.no_grad():
                cache[1][key] = self._pack(self.pads(H, W))
        return cache[1][key]

    # ---- forward ----------------------------------------------------------------------------------------------------
    def endpoints_nhwc(self, x):
        """x [N, 3, H, W] (planar, as the model passes images) -> (reduction_{k+1} [N, h, w, c_hi], reduction_k [N, 2h, 2w, c_lo]), NHWC: what
        ``Encoder.neck_from_nhwc`` reads."""
        runtime.require_cuda(x)
        runtime.require_no_grad(x)
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("EfficientNetTrunk: images [N, 3, H, W], got %s" % (tuple(x.shape),))
        x = runtime.f32c(x)
        n, _, H, W = x.shape
        _, (c_hi, h_hi, w_hi), (c_lo, h_lo, w_lo) = self.plan(H, W)
        pk = self.packed(H, W)
        hi = torch.empty((n, h_hi, w_hi, c_hi), dtype=torch.float32, device=x.device)
        lo = torch.empty((n, h_lo, w_lo, c_lo), dtype=torch.float32, device=x.device)
        w = ctypes.byref(pk.struct)      # the entry points take the extension header's structs as const void*
        runtime.call("effnet_trunk", w, ptr(x), 1, ptr(hi), ptr(lo), n, H, W, device=x.device, scratch=("effnet_trunk", w, n, H, W))
        return hi, lo

    def forward(self, x):
        hi, lo = self.endpoints_nhwc(x)
        return runtime.to_nchw(hi), runtime.to_nchw(lo)
