"""Shared by test_effnet_trunk.py (CPU) and test_gpu_effnet_trunk.py: the EfficientNet trunk restated in plain torch, hashed weights,
tolerances.

``RefTrunk`` is written from the architecture alone (efficientnet_pytorch 0.7.x: stage table, width / depth scaling, static "same"
padding from the nominal image size, MBConv in eval mode), NOT from streamingflow_amd/models/efficientnet.py: its own stage table, its
own rounding, its own padding arithmetic.  It runs on the CPU in float64 (the reference) and float32 (whose own error against float64
sets every bound, x 8: the rule of tests/encoder_neck_util.tolerance), and on the GPU in float32 for tools/trunkbench.py.  It carries
the attribute names ``EfficientNetEndpoints`` walks (``_conv_stem``, ``_bn0``, ``_swish``, ``_blocks``, ``_global_params``).

Weights come from the hash filler (workloads/hashfill.fill_state_dict: seeded from (key, shape), fan-in scaled, BatchNorm statistics
randomised so that the fold is exercised)."""
import functools
import math
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

from util import hashfill

SEED, GAIN = 11, 1.2      # gain: endpoints of O(1) on every version (2.0 overflows b4 by block 21, 1.4 b7)
# (kernel, repeats, in, out, expand, stride)
STAGES = ((3, 1, 32, 16, 1, 1), (3, 2, 16, 24, 6, 2), (5, 2, 24, 40, 6, 2), (3, 3, 40, 80, 6, 2), (5, 3, 80, 112, 6, 1), (5, 4, 112, 192, 6, 2),
          (3, 1, 192, 320, 6, 1))
VERSIONS = {"b0": (1.0, 1.0, 224), "b4": (1.4, 1.8, 380), "b7": (2.0, 3.1, 600)}      # width, depth, nominal size
LAST_BLOCK_AT_8 = {"b0": 10, "b4": 21, "b7": 37}
EPS = 1e-3


def filters(f, width):
    f = f * width
    r = max(8, (int(f + 4) // 8) * 8)
    return r + 8 if r < 0.9 * f else r


def blocks_of(version, downsample):
    """[(k, stride, cin, cout, expand, se channels)] of the blocks the reference keeps."""
    width, depth, _ = VERSIONS[version]
    out = []
    for k, r, ci, co, e, s in STAGES:
        ci, co = filters(ci, width), filters(co, width)
        for j in range(int(math.ceil(depth * r))):
            cin, stride = (ci, s) if j == 0 else (co, 1)
            out.append((k, stride, cin, co, e, max(1, int(cin * 0.25))))
    return out[:LAST_BLOCK_AT_8[version] + 1] if downsample == 8 else out


def expected_keys(version, downsample):
    """The state_dict keys of the trunk as the issue lists them."""
    bn = lambda p: [p + "." + s for s in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    keys = ["_conv_stem.weight"] + bn("_bn0")
    for i, (k, stride, cin, co, e, se) in enumerate(blocks_of(version, downsample)):
        p = "_blocks.%d." % i
        if e != 1:
            keys += [p + "_expand_conv.weight"] + bn(p + "_bn0")
        keys += [p + "_depthwise_conv.weight"] + bn(p + "_bn1")
        keys += [p + "_se_reduce.weight", p + "_se_reduce.bias", p + "_se_expand.weight", p + "_se_expand.bias"]
        keys += [p + "_project_conv.weight"] + bn(p + "_bn2")
    return keys


def pad4(h, w, k, stride):
    """"same" padding of one layer on an h x w input -> ((left, right, top, bottom) as F.pad takes them, output size)."""
    oh, ow = -(-h // stride), -(-w // stride)
    ph, pw = max((oh - 1) * stride + k - h, 0), max((ow - 1) * stride + k - w, 0)
    return (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2), (oh, ow)


def swish(x):
    return x * torch.sigmoid(x)


def bn(sd, p, x):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, EPS)


def mbconv(sd, p, x, k, stride, pad, skip):
    """One MBConv block in eval mode on the state ``sd`` under prefix ``p``; ``pad`` as F.pad takes it."""
    inp = x
    if p + "_expand_conv.weight" in sd:
        x = swish(bn(sd, p + "_bn0", F.conv2d(x, sd[p + "_expand_conv.weight"])))
    x = swish(bn(sd, p + "_bn1", F.conv2d(F.pad(x, pad), sd[p + "_depthwise_conv.weight"], stride=stride, groups=x.shape[1])))
    s = x.mean((2, 3), keepdim=True)
    s = swish(F.conv2d(s, sd[p + "_se_reduce.weight"], sd[p + "_se_reduce.bias"]))
    x = torch.sigmoid(F.conv2d(s, sd[p + "_se_expand.weight"], sd[p + "_se_expand.bias"])) * x
    x = bn(sd, p + "_bn2", F.conv2d(x, sd[p + "_project_conv.weight"]))
    return x + inp if skip else x


class _Block:
    def __init__(self, trunk, i):
        self.trunk, self.i = trunk, i

    def __call__(self, x, drop_connect_rate=None):      # drop-connect is the identity in eval mode
        t, i = self.trunk, self.i
        k, stride, cin, co, e, se = t.blocks[i]
        pad = t.static_pads[i + 1] if t.static_pads else pad4(x.shape[2], x.shape[3], k, stride)[0]
        return mbconv(t.sd, "_blocks.%d." % i, x, k, stride, pad, stride == 1 and cin == co)


class RefTrunk:
    """The trunk on a state dict (the trunk's own keys, no prefix) in ``dtype``.  image_size: "nominal", an int / pair, or None (dynamic)."""

    def __init__(self, sd, version, downsample=8, image_size="nominal", dtype=torch.float64, device="cpu"):
        self.version, self.downsample = version, downsample
        self.sd = {k: v.to(device=device, dtype=dtype) for k, v in sd.items() if v.is_floating_point()}
        self.dtype, self.device = dtype, device
        self.blocks = blocks_of(version, downsample)
        size = VERSIONS[version][2] if image_size == "nominal" else image_size
        self.static_pads = None
        if size is not None:
            h, w = (size, size) if isinstance(size, int) else size
            self.static_pads = []
            for k, stride in [(3, 2)] + [(b[0], b[1]) for b in self.blocks]:
                pad, (h, w) = pad4(h, w, k, stride)
                self.static_pads.append(pad)
        self._blocks = [_Block(self, i) for i in range(len(self.blocks))]
        self._global_params = NS(drop_connect_rate=0.2)
        self._swish = swish

    def _conv_stem(self, x):
        pad = self.static_pads[0] if self.static_pads else pad4(x.shape[2], x.shape[3], 3, 2)[0]
        return F.conv2d(F.pad(x, pad), self.sd["_conv_stem.weight"], stride=2)

    def _bn0(self, x):
        return bn(self.sd, "_bn0", x)

    def walk(self, x):
        """-> (reduction_{k+1}, reduction_k): an endpoint is the tensor in front of every block that lowers the height; the last block's
        output is the final endpoint."""
        with torch.no_grad():
            x = swish(self._bn0(self._conv_stem(x.to(device=self.device, dtype=self.dtype))))
            ends = []
            for blk in self._blocks:
                y = blk(x)
                if y.shape[2] < x.shape[2]:
                    ends.append(x)
                x = y
            ends.append(x)
            k = int(math.log2(self.downsample))
            return ends[k], ends[k - 1]


@functools.lru_cache(maxsize=None)
def state(version, downsample=8):
    """Hashed state of the version's trunk under the reference's ``backbone.`` keys (``trunk_state``: without the prefix), float32 CPU.  Computed once; callers do not modify it."""
    from streamingflow_amd.models.efficientnet import EfficientNetTrunk
    sd = EfficientNetTrunk(version, downsample).state_dict()
    return hashfill.fill_state_dict({"backbone." + k: v for k, v in sd.items()}, seed=SEED, gain=GAIN)


def trunk_state(version, downsample=8):
    return {k[len("backbone."):]: v for k, v in state(version, downsample).items()}


def images(name, shape):
    return hashfill.uniform("effnet_img_" + name, shape, -1.0, 1.0, 71)


def tolerance(ref64, ref32):
    """8 x the float32 restatement's own max error against float64 on the same inputs, per output."""
    return tuple(8.0 * float((a.double() - b).abs().max()) for a, b in zip(ref32, ref64))


def placeholder_trunk(version, downsample, pads, index=None):
    """(``_lib.EffNetW``, keep-alive) with the version's integers around placeholder pointers (ws_layout_util.HOLE): for the size query
    and for calls that must refuse before they launch.  ``pads``: (top, left, bottom, right) of the stem and of every block."""
    import ctypes
    from streamingflow_amd import _lib
    from ws_layout_util import HOLE, conv
    blocks = blocks_of(version, downsample)
    arr = (_lib.MBConvW * len(blocks))()
    for b, (k, stride, cin, co, e, se), pad in zip(arr, blocks, pads[1:]):
        cexp = cin * e
        if e != 1:
            b.expand = conv(cexp, cin)
        b.project = conv(co, cexp)
        b.dw_w = b.dw_scale = b.dw_bias = b.se_reduce_w = b.se_reduce_b = b.se_expand_w = b.se_expand_b = HOLE.value
        b.cin, b.cexp, b.cout, b.cse, b.k, b.stride, b.skip = cin, cexp, co, se, k, stride, int(stride == 1 and cin == co)
        b.pad_t, b.pad_l, b.pad_b, b.pad_r = pad
    w = _lib.EffNetW()
    w.stem_w = w.stem_scale = w.stem_bias = HOLE.value
    w.blocks = ctypes.cast(arr, ctypes.POINTER(_lib.MBConvW))
    w.c_stem, w.n_blocks, w.index = filters(32, VERSIONS[version][0]), len(blocks), int(math.log2(downsample)) if index is None else index
    w.pad_t, w.pad_l, w.pad_b, w.pad_r = pads[0]
    return w, arr
