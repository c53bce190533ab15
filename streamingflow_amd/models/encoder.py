"""Camera ``Encoder`` (streamingflow/models/encoder.py): the neck on the MI355X, the EfficientNet trunk pluggable.

The reference's encoder is an EfficientNet trunk (third-party ``efficientnet_pytorch``; restated on the device in models/efficientnet.py:
``backbone=EfficientNetTrunk("b4")``) followed by
StreamingFlow's own neck: per branch (features, depth) one ``DeepLabHead(c_hi, c_hi, hidden_channel=64)`` on the /16 endpoint
and one ``UpsamplingConcat(c_hi + c_lo, C or D)`` joining the /8 endpoint (encoder.py:34-39, :107-112).  ``Encoder`` keeps the
reference's sub-module names and ``state_dict`` keys (``feature_layer_1/2``, ``depth_layer_1/2``): a released checkpoint's
``encoder.*`` slice minus ``backbone.*`` loads with ``strict=True`` when no backbone is attached.

The neck is ONE library call (``sf_camera_neck_fwd``, csrc/camera_neck.hip):

* both heads read the same input, so they are packed as one twin head of hidden width 2 * 64 — branch and pooling weights stacked on
  cout, projection / 3x3 / classifier block-diagonal (``twin_head_tensors``); the zero blocks contribute exact zeros;
* a dilated 3x3 branch whose rate is >= both H and W reads only padding through its eight outer taps (``dead_rates``): it is packed as
  the 1x1 convolution of its centre tap — exact; the pack is cached per set of dead rates, i.e. per (H, W);
* the depth branch ends in ``depth_softmax_planar_kernel``: planar logits (``depth_prediction``) and planar probabilities (what the
  lift reads) from the NHWC logits in one pass.

Inference only: ``.eval()`` is required.  No CPU fallback: CPU tensors raise.
"""
import math

import torch
import torch.nn as nn

from .. import _lib, packing, runtime
from ..layers.convolutions import DeepLabHead, UpsamplingConcat
from ..runtime import ptr

# encoder.py:22-30
REDUCTION_CHANNEL = {"b0": [0, 16, 24, 40, 112, 320], "b4": [0, 24, 32, 56, 160, 448], "b7": [0, 32, 48, 80, 224, 640]}
UPSAMPLING_OUT_CHANNEL = [0, 48, 64, 128, 512]
# encoder.py:47-53, :92-98: the last block walked at DOWNSAMPLE == 8
BREAK_INDEX = {"b0": 10, "b4": 21, "b7": 37}
HIDDEN = 64


def dead_rates(rates, H, W):
    """The dilation rates whose 3x3 branch (padding = rate) degenerates to its centre tap on an H x W image: an outer tap is
    rate rows or columns away, so with rate >= H and rate >= W all eight read padding only.  A rate that is dead along one
    axis only (24 at 14 x 30) still has two live taps and stays a full 3x3."""
    return tuple(r for r in rates if r >= H and r >= W)


def _block_diag(a, b):
    """[oa + ob][ia + ib][...] with a and b on the diagonal, exact zeros elsewhere."""
    out = a.new_zeros((a.shape[0] + b.shape[0], a.shape[1] + b.shape[1]) + tuple(a.shape[2:]))
    out[:a.shape[0], :a.shape[1]] = a
    out[a.shape[0]:, a.shape[1]:] = b
    return out


def twin_head_tensors(feature_head, depth_head, collapsed=()):
    """The weights of ONE DeepLabHead of hidden width 2 * hid computing [feature_head(x) | depth_head(x)], as plain tensors on the
    heads' own device (no BatchNorm folded: ``bn`` holds the module pairs):
      branch_w[i]   [2 hid][C][k][k]   the two heads' branch i stacked on cout (k = 1 for branch 0 and for a rate in ``collapsed``)
      pool_w        [2 hid][C]
      project_w     [2 hid][4 * 2 hid] branch i of the cat is [feature | depth]: block-diagonal inside every branch's 2 hid columns
      proj_pool_w   [2 hid][2 hid], conv3_w [2 hid][2 hid][3][3], cls_w [2 c][2 hid][1][1]: block-diagonal;  cls_b [2 c]
    """
    f, d = feature_head, depth_head
    hid = f.hidden_channel
    assert d.hidden_channel == hid and d.in_channels == f.in_channels
    fa, da = f[0], d[0]
    t = {"branch_w": [], "branch_dil": [], "hid": 2 * hid, "C": f.in_channels}
    for i in range(4):
        wf, wd = fa.convs[i][0].weight.detach(), da.convs[i][0].weight.detach()
        dil = fa.convs[i][0].dilation[0]
        if i and dil in collapsed:
            wf, wd, dil = wf[:, :, 1:2, 1:2], wd[:, :, 1:2, 1:2], 1
        t["branch_w"].append(torch.cat([wf, wd], 0).contiguous())
        t["branch_dil"].append(dil)
    t["pool_w"] = torch.cat([fa.convs[4][1].weight.detach(), da.convs[4][1].weight.detach()], 0).reshape(2 * hid, f.in_channels)
    pf, pd = fa.project[0].weight.detach(), da.project[0].weight.detach()                # [hid][5 hid][1][1]
    t["project_w"] = torch.cat([_block_diag(pf[:, i * hid:(i + 1) * hid], pd[:, i * hid:(i + 1) * hid]) for i in range(4)], 1).contiguous()
    t["proj_pool_w"] = _block_diag(pf[:, 4 * hid:, 0, 0], pd[:, 4 * hid:, 0, 0])
    t["conv3_w"] = _block_diag(f[1].weight.detach(), d[1].weight.detach())
    t["cls_w"] = _block_diag(f[4].weight.detach(), d[4].weight.detach())
    t["cls_b"] = torch.cat([f[4].bias.detach(), d[4].bias.detach()])
    return t


class EfficientNetEndpoints(nn.Module):
    """Plain-torch adapter around an ``efficientnet_pytorch.EfficientNet`` (any module with ``_conv_stem``, ``_bn0``, ``_swish``,
    ``_blocks`` and ``_global_params``): the walk of encoder.py:64-105 — stem, then the blocks with the scaled drop-connect rate, an
    endpoint recorded whenever the resolution drops, the version's last block at DOWNSAMPLE == 8 — returning
    ``(reduction_{k+1}, reduction_k)``, k = log2(downsample).  Nothing here runs on this package's kernels: it exists so that a user
    who has the trunk can plug it into ``Encoder(cfg, D, backbone=...)``."""

    def __init__(self, module, version, downsample):
        super().__init__()
        if version not in BREAK_INDEX:
            raise NotImplementedError("EfficientNet version %r: b0 / b4 / b7 only" % (version,))
        self.module, self.version, self.downsample = module, version, int(downsample)
        self.index = int(math.log2(self.downsample))

    def forward(self, x):
        m = self.module
        brk = BREAK_INDEX[self.version] if self.downsample == 8 else None
        # the reference deletes the blocks behind the break before it walks: the drop-connect scale divides by what is left
        n_blocks = len(m._blocks) if brk is None else min(len(m._blocks), brk + 1)
        endpoints = {}
        x = m._swish(m._bn0(m._conv_stem(x)))
        prev_x = x
        for idx, block in enumerate(m._blocks):
            drop_connect_rate = m._global_params.drop_connect_rate
            if drop_connect_rate:
                drop_connect_rate *= float(idx) / n_blocks
            x = block(x, drop_connect_rate=drop_connect_rate)
            if prev_x.size(2) > x.size(2):
                endpoints["reduction_%d" % (len(endpoints) + 1)] = prev_x
            prev_x = x
            if idx == brk:
                break
        endpoints["reduction_%d" % (len(endpoints) + 1)] = x
        return endpoints["reduction_%d" % (self.index + 1)], endpoints["reduction_%d" % self.index]


class Encoder(nn.Module):
    def __init__(self, cfg, D, backbone=None):
        super().__init__()
        self.D = D
        self.C = cfg.OUT_CHANNELS
        self.use_depth_distribution = cfg.USE_DEPTH_DISTRIBUTION
        self.downsample = cfg.DOWNSAMPLE
        self.version = cfg.NAME.split('-')[1]
        if self.version not in REDUCTION_CHANNEL:
            raise NotImplementedError("Encoder: EfficientNet b0 / b4 / b7 only (encoder.py:22-29)")
        if not self.use_depth_distribution:
            raise NotImplementedError("Encoder: USE_DEPTH_DISTRIBUTION=False is not built (no shipped config uses it)")
        self.reduction_channel = REDUCTION_CHANNEL[self.version]
        self.upsampling_out_channel = UPSAMPLING_OUT_CHANNEL
        index = int(math.log2(self.downsample))
        if 2 ** index != self.downsample or not 1 <= index < len(self.reduction_channel) - 1:
            raise NotImplementedError("Encoder: DOWNSAMPLE must be 2, 4, 8 or 16")
        self.c_hi, self.c_lo = self.reduction_channel[index + 1], self.reduction_channel[index]
        self.backbone = backbone
        self.depth_layer_1 = DeepLabHead(self.c_hi, self.c_hi, hidden_channel=HIDDEN)
        self.depth_layer_2 = UpsamplingConcat(self.c_hi + self.c_lo, self.D)
        self.feature_layer_1 = DeepLabHead(self.c_hi, self.c_hi, hidden_channel=HIDDEN)
        self.feature_layer_2 = UpsamplingConcat(self.c_hi + self.c_lo, self.C)
        self.collapse = True      # tests pack the same head without the dead-branch collapse

    def __getstate__(self):
        return runtime.strip_runtime_state(self.__dict__)

    # ---- packing ----------------------------------------------------------------------------------------------------
    def _neck_parameters(self):
        for m in (self.feature_layer_1, self.feature_layer_2, self.depth_layer_1, self.depth_layer_2):
            yield from m.parameters()
            yield from m.buffers()

    def _pack(self, collapsed):
        if self.training:
            raise RuntimeError("streamingflow_amd is inference-only: call .eval() (BatchNorm uses running statistics)")
        f, d = self.feature_layer_1, self.depth_layer_1
        t = twin_head_tensors(f, d, collapsed)
        pk = packing.Pack(_lib.DeepLabW())
        s, C, hid = pk.struct, t["C"], t["hid"]
        fold2 = lambda a, b: [torch.cat(v) for v in zip(packing.bn_fold(a), packing.bn_fold(b))]
        for i in range(4):
            sc, bi = fold2(f[0].convs[i][1], d[0].convs[i][1])
            s.branch[i] = packing.conv_w(pk, t["branch_w"][i], C, scale=sc, bias=bi, act="relu", dil=t["branch_dil"][i])
        sc, bi = fold2(f[0].convs[4][2], d[0].convs[4][2])
        s.pool_w, s.pool_scale, s.pool_bias = pk.hold(t["pool_w"]), pk.hold(sc), pk.hold(bi)
        s.proj_pool_w = pk.hold(t["proj_pool_w"])
        sc, bi = fold2(f[0].project[1], d[0].project[1])
        s.project = packing.conv_w(pk, t["project_w"], 4 * hid, scale=sc, bias=bi, act="relu")
        sc, bi = fold2(f[2], d[2])
        s.conv3 = packing.conv_w(pk, t["conv3_w"], hid, scale=sc, bias=bi, act="relu")
        s.cls = packing.conv_w(pk, t["cls_w"], hid, bias=t["cls_b"])
        s.C, s.hid = C, hid
        pk.convs = (_lib.ConvW * 4)(*(self.feature_layer_2.pack(pk, self.c_lo) + self.depth_layer_2.pack(pk, self.c_lo)))
        return pk

    def packed(self, H, W):
        """The packed neck for an H x W /16 endpoint: re-packed when a parameter changed (as PackedModule), one copy per set of
        collapsed dilation rates."""
        sig = (packing.math_mode(), packing.winograd()) + tuple((p.data_ptr(), p._version, p.device) for p in self._neck_parameters())
        cache = self.__dict__.get("_sf_neck_packs")
        if cache is None or cache[0] != sig:
            self.__dict__["_sf_neck_packs"] = cache = (sig, {})
        key = dead_rates(self.feature_layer_1[0].rates, H, W) if self.collapse else ()
        if key not in cache[1]:
            runtime.require_cuda(self.feature_layer_1[1].weight)
            with torch.no_grad():
                cache[1][key] = self._pack(key)
        return cache[1][key]

    # ---- forward ----------------------------------------------------------------------------------------------------
    def neck_nhwc(self, reduction_hi, reduction_lo):
        """reduction_hi [N, c_hi, H, W], reduction_lo [N, c_lo, 2H, 2W] (NCHW, as a trunk returns them) ->
        (rays [N * 4HW, C] NHWC features, depth logits [N, D, 4HW] planar, depth probabilities [N, D, 4HW] planar)."""
        runtime.require_cuda(reduction_hi, reduction_lo)
        n, c_hi, H, W = reduction_hi.shape
        if c_hi != self.c_hi or tuple(reduction_lo.shape) != (n, self.c_lo, 2 * H, 2 * W):
            raise ValueError("neck: endpoints %s / %s, expected [N, %d, H, W] / [N, %d, 2H, 2W]"
                             % (tuple(reduction_hi.shape), tuple(reduction_lo.shape), self.c_hi, self.c_lo))
        return self.neck_from_nhwc(runtime.to_nhwc(reduction_hi), runtime.to_nhwc(reduction_lo))

    def neck_from_nhwc(self, hi, lo):
        """``neck_nhwc`` on endpoints that are NHWC already — hi [N, H, W, c_hi], lo [N, 2H, 2W, c_lo], contiguous fp32, as
        ``EfficientNetTrunk.endpoints_nhwc`` returns them: no layout conversion in front of the neck."""
        runtime.require_cuda(hi, lo)
        n, H, W, c_hi = hi.shape
        if c_hi != self.c_hi or tuple(lo.shape) != (n, 2 * H, 2 * W, self.c_lo) or not (hi.is_contiguous() and lo.is_contiguous()):
            raise ValueError("neck: NHWC endpoints %s / %s, expected contiguous [N, H, W, %d] / [N, 2H, 2W, %d]"
                             % (tuple(hi.shape), tuple(lo.shape), self.c_hi, self.c_lo))
        hi, lo = runtime.f32c(hi), runtime.f32c(lo)
        pk = self.packed(H, W)
        dev = hi.device
        rays = torch.empty((n * 4 * H * W, self.C), dtype=torch.float32, device=dev)
        logits = torch.empty((n, self.D, 4 * H * W), dtype=torch.float32, device=dev)
        prob = torch.empty_like(logits)
        runtime.call("camera_neck", pk.struct, pk.convs, ptr(hi), ptr(lo), ptr(rays), ptr(logits), ptr(prob), n, H, W, device=dev,
                     scratch=("camera_neck", self.c_hi, self.c_lo, self.C, self.D, 2 * HIDDEN, n, H, W))
        return rays, logits, prob

    def neck(self, reduction_hi, reduction_lo):
        """-> (feature [N, C, 2H, 2W], depth_logits [N, D, 2H, 2W]): ``Encoder.get_features_depth`` after its endpoint selection."""
        n, _, H, W = reduction_hi.shape
        rays, logits, _ = self.neck_nhwc(reduction_hi, reduction_lo)
        return runtime.to_nchw(rays.view(n, 2 * H, 2 * W, self.C)), logits.view(n, self.D, 2 * H, 2 * W)

    def _endpoints(self, x):
        if self.backbone is None:
            raise RuntimeError("Encoder has no backbone: construct it with backbone=EfficientNetTrunk(version) (models/efficientnet.py) "
                               "(or any module returning (reduction_hi, reduction_lo)), or call neck() on the two endpoints")
        return self.backbone(x)

    def forward_nhwc(self, x):
        if hasattr(self.backbone, "endpoints_nhwc"):      # EfficientNetTrunk: its endpoints are NHWC as they leave the device code
            return self.neck_from_nhwc(*self.backbone.endpoints_nhwc(x))
        return self.neck_nhwc(*self._endpoints(x))

    def forward(self, x):
        return self.neck(*self._endpoints(x))
