"""MI355X-native counterparts of mmdet3d/models/beverse/models/motion_modules.py:
``DistributionModule`` (:10-46), ``SpatialDistributionModule`` (:49-88), ``DistributionEncoder``
(:91-108), ``FuturePrediction`` (:111-146), ``ResFuturePrediction`` / ``ResFuturePredictionV2`` /
``ResFuturePredictionV1`` (:149-431) and ``warp_with_flow`` (:434-449).  Same signatures and state_dict keys; HIP execution."""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib, packing, runtime
from ..layers.convolutions import dist_head_nhwc
from ..runtime import PackedModule, ptr
from .basic_modules import (Bottleneck, ConvBlock, GRUCell, SpatialGRU, conv_block_torch, gru_cell_torch, require_eval, spatial_gru_torch,
                            use_torch_path)


class DistributionEncoder(nn.Module):
    def __init__(self, in_channels, out_channels, num_layer=2):
        super().__init__()
        layers = []
        for _ in range(num_layer):
            layers.append(Bottleneck(in_channels=in_channels, out_channels=out_channels, downsample=True))
            in_channels = out_channels
        self.model = nn.Sequential(*layers)

    def forward_nhwc(self, x):
        for blk in self.model:
            x = blk.forward_nhwc(x)
        return x

    def forward(self, s_t):
        return runtime.to_nchw(self.forward_nhwc(runtime.to_nhwc(s_t)))


class _DistBase(PackedModule):
    global_pool = False

    def __init__(self, in_channels, latent_dim, min_log_sigma, max_log_sigma):
        super().__init__()
        self.compress_dim, self.latent_dim = in_channels // 2, latent_dim
        self.min_log_sigma, self.max_log_sigma = min_log_sigma, max_log_sigma
        self.encoder = DistributionEncoder(in_channels, self.compress_dim)
        head = nn.Conv2d(self.compress_dim, out_channels=2 * latent_dim, kernel_size=1)
        self.last_conv = nn.Sequential(nn.AdaptiveAvgPool2d(1), head) if self.global_pool else nn.Sequential(head)

    def _pack(self):
        pk = packing.Pack(None)
        conv = self.last_conv[-1]
        pk.struct = packing.conv_w(pk, conv.weight, self.compress_dim, bias=conv.bias)
        return pk

    def _head(self, enc):
        return dist_head_nhwc(self.packed().struct, enc, self.global_pool, clamp=(self.min_log_sigma, self.max_log_sigma))


class DistributionModule(_DistBase):
    """Diagonal Gaussian over the whole BEV map: (mu, log_sigma) of shape (b, 1, latent_dim)."""
    global_pool = True

    def forward(self, s_t):
        b, s = s_t.shape[:2]
        assert s == 1
        runtime.require_cuda(s_t)
        out = self._head(self.encoder.forward_nhwc(runtime.to_nhwc(s_t[:, 0]))).view(b, 1, 2 * self.latent_dim)
        return out[:, :, :self.latent_dim], out[:, :, self.latent_dim:]


class SpatialDistributionModule(_DistBase):
    """Per-location Gaussian (no global pooling): (mu, log_sigma) of shape (b, latent_dim, h/4, w/4)."""
    global_pool = False

    def forward(self, s_t):
        b, s = s_t.shape[:2]
        assert s == 1
        runtime.require_cuda(s_t)
        out = runtime.to_nchw(self._head(self.encoder.forward_nhwc(runtime.to_nhwc(s_t[:, 0]))))
        return out[:, :self.latent_dim], out[:, self.latent_dim:]


class FuturePrediction(nn.Module):
    """[SpatialGRU -> n_res_layers x Bottleneck] x n_gru_blocks (motion_modules.py:111-146)."""

    def __init__(self, in_channels, latent_dim, n_gru_blocks=3, n_res_layers=3):
        super().__init__()
        self.n_gru_blocks = n_gru_blocks
        grus, blocks = [], []
        for i in range(n_gru_blocks):
            grus.append(SpatialGRU(latent_dim if i == 0 else in_channels, in_channels))
            blocks.append(nn.Sequential(*[Bottleneck(in_channels) for _ in range(n_res_layers)]))
        self.spatial_grus = nn.ModuleList(grus)
        self.res_blocks = nn.ModuleList(blocks)

    def forward(self, x, hidden_state):
        runtime.require_cuda(x, hidden_state)
        b, T, c, h, w = x.shape
        xn = runtime.frames_to_nhwc(x)
        hid = runtime.to_nhwc(hidden_state)
        for gru, blocks in zip(self.spatial_grus, self.res_blocks):
            xn = gru.forward_nhwc(xn, hid)                       # [T, b, h, w, C]
            y = xn.view(T * b, h, w, xn.shape[-1])
            for blk in blocks:
                y = blk.forward_nhwc(y)
            xn = y.view(T, b, h, w, y.shape[-1])
        return runtime.frames_to_nchw(xn)


# ---- ResFuturePrediction family (motion_modules.py:149-449): flow-warp GRU rollout ---------------------------------------------
def flow_warp_nhwc(state, out, out_cs, out_co, feat=None, w_off=None, b_off=None, flow=None, flow_out=None):
    """``sf_flow_warp_fwd``: state [B, h, w, C] resampled along a per-pixel flow into channels out_co .. out_co + C of out
    [B, h, w, out_cs].  The flow is `flow` [B, h, w, 2] (x, y) or the fused 1x1 head w_off [2, Cf] . feat [B, h, w, Cf] + b_off."""
    B, h, w, C = state.shape
    runtime.call("flow_warp", ptr(state), ptr(feat), ptr(w_off), ptr(b_off), ptr(flow), ptr(out), ptr(flow_out), B, h, w, C,
                 feat.shape[-1] if feat is not None else 0, out_cs, out_co, device=state.device)
    return out


def warp_with_flow(x, flow):
    """x (B, C, H, W) sampled at (row + flow[:, 1], column + flow[:, 0]): bilinear, zeros outside, align_corners=True
    (motion_modules.py:434-449).  Unlike the reference, which adds the pixel grid into the caller's ``flow`` and normalises it in
    place, this function leaves ``flow`` unchanged."""
    B, C, H, W = x.shape
    if use_torch_path(x, flow):
        xx = torch.arange(0, W, device=x.device).view(1, 1, 1, W).expand(B, 1, H, W)
        yy = torch.arange(0, H, device=x.device).view(1, 1, H, 1).expand(B, 1, H, W)
        g = (flow + torch.cat((xx, yy), dim=1).float().type_as(flow)).permute(0, 2, 3, 1)
        g = torch.stack((g[..., 0] / (W - 1) * 2 - 1.0, g[..., 1] / (H - 1) * 2 - 1.0), dim=-1)
        return F.grid_sample(x, g, mode='bilinear', align_corners=True)
    if C % 4:
        raise NotImplementedError("warp_with_flow: the channel count must be a multiple of 4 (the kernel moves channels in fours)")
    xn = runtime.to_nhwc(x)
    out = torch.empty_like(xn)
    flow_warp_nhwc(xn, out, C, 0, flow=runtime.to_nhwc(flow))
    return runtime.to_nchw(out)


def _pack_block(pk, blk, c0, c1=0):
    sc, bi = packing.bn_fold(blk.norm, blk.conv.bias)
    return packing.conv_w(pk, blk.conv.weight, c0, c1, scale=sc, bias=bi, act="relu")


def _pack_flow_head(pk, blk, head, L, C):
    """(offset ConvBlock on (sample, state), [2][C+L] weights and [2] bias of the 1x1 the warp kernel computes itself)."""
    w_off = head.weight.detach().to(torch.float32).reshape(2, L + C).clone()
    b_off = head.bias.detach().to(torch.float32).clone()
    pk.keep += [w_off, b_off]
    return _pack_block(pk, blk, L, C), w_off, b_off


def _check_channels(in_channels, latent_dim):
    if in_channels % 4 or latent_dim % 4:
        raise NotImplementedError("ResFuturePrediction: in_channels and latent_dim must be multiples of 4 (the kernels move channels in fours)")


class _ResFutureBase(PackedModule):
    """What ResFuturePrediction and ResFuturePredictionV2 share: per frame, [flow head -> warp ->] GRUCell chain -> ConvBlock."""
    sample_first_without_flow = True

    def _flow_modules(self, i):
        raise NotImplementedError

    def _spatial_block(self, i):
        raise NotImplementedError

    def _build_cells(self, in_channels, latent_dim, n_gru_blocks):
        self.gru_cells = nn.ModuleList()
        cin = in_channels + latent_dim
        for _ in range(n_gru_blocks):
            self.gru_cells.append(GRUCell(input_size=cin, hidden_size=in_channels))
            cin = in_channels

    def _pack(self):
        require_eval(self)
        pk = packing.Pack(None)
        C, L = self.in_channels, self.latent_dim
        done = {}      # V2 without state refinement lists ONE module n_future times: packed once
        pk.flow, pk.spatial = [], []
        for i in range(self.n_future):
            if self.flow_warp:
                blk, head = self._flow_modules(i)
                if id(blk) not in done:
                    done[id(blk)] = _pack_flow_head(pk, blk, head, L, C)
                pk.flow.append(done[id(blk)])
            sp = self._spatial_block(i)
            if id(sp) not in done:
                done[id(sp)] = _pack_block(pk, sp, C)
            pk.spatial.append(done[id(sp)])
        return pk

    def forward_nhwc(self, sn, hid):
        """sample [B, h, w, L], hidden state [B, h, w, C] -> frames [n_future, B, h, w, C].  Enqueues only."""
        B, h, w, L = sn.shape
        C = self.in_channels
        pk = self.packed()
        dev = sn.device
        # the GRU input: (warped, sample) with flow, else (sample, state) / V2 (state, sample); sample written once
        s_co, w_co = (C, 0) if self.flow_warp or not self.sample_first_without_flow else (0, L)
        xbuf = torch.empty((B, h, w, C + L), dtype=torch.float32, device=dev)
        xbuf[..., s_co:s_co + L].copy_(sn)
        feat = torch.empty((B, h, w, C + L), dtype=torch.float32, device=dev) if self.flow_warp else None
        frames = torch.empty((self.n_future, B, h, w, C), dtype=torch.float32, device=dev)
        cur = hid
        for i in range(self.n_future):
            if self.flow_warp:
                cw, w_off, b_off = pk.flow[i]
                runtime.conv2d_ex(cw, sn, L, 0, B, h, w, feat, C + L, 0, in1=cur, in1_cs=C)
                flow_warp_nhwc(cur, xbuf, C + L, w_co, feat=feat, w_off=w_off, b_off=b_off)
            else:
                xbuf[..., w_co:w_co + C].copy_(cur)
            y = xbuf
            for cell in self.gru_cells:
                y = cell.forward_nhwc(y, cur)
            runtime.conv2d_ex(pk.spatial[i], y, C, 0, B, h, w, frames[i], C, 0)
            cur = frames[i]
        return frames

    def _forward_torch(self, sample, hidden):
        res, cur = [], hidden
        for i in range(self.n_future):
            if self.flow_warp:
                blk, head = self._flow_modules(i)
                flow = F.conv2d(conv_block_torch(blk, torch.cat((sample, cur), dim=1)), head.weight, head.bias)
                x = torch.cat((warp_with_flow(cur, flow), sample), dim=1)
            elif self.sample_first_without_flow:
                x = torch.cat((sample, cur), dim=1)
            else:
                x = torch.cat((cur, sample), dim=1)
            for cell in self.gru_cells:
                x = gru_cell_torch(cell, x, cur)
            cur = conv_block_torch(self._spatial_block(i), x)
            res.append(cur)
        return torch.stack(res, dim=1)

    def forward(self, sample_distribution, hidden_state):
        """sample (b, latent_dim, h, w), hidden state (b, in_channels, h, w) -> (b, n_future, in_channels, h, w)."""
        require_eval(self)
        assert sample_distribution.shape[1] == self.latent_dim and hidden_state.shape[1] == self.in_channels
        if use_torch_path(sample_distribution, hidden_state, next(self.parameters())):
            with torch.no_grad():
                return self._forward_torch(sample_distribution, hidden_state)
        return runtime.frames_to_nchw_strided(self.forward_nhwc(runtime.to_nhwc(sample_distribution), runtime.to_nhwc(hidden_state)))


class ResFuturePrediction(_ResFutureBase):
    """Per frame: offset head on (sample, state) -> warp the state -> GRUCell chain on (warped, sample) with the frame's
    state -> 3x3 ConvBlock (motion_modules.py:149-227).  ``detach_state`` is accepted and has no effect (inference only)."""

    def __init__(self, in_channels, latent_dim, n_future, detach_state=True, n_gru_blocks=3, flow_warp=True, prob_each_future=False):
        super().__init__()
        _check_channels(in_channels, latent_dim)
        self.in_channels, self.latent_dim = in_channels, latent_dim
        self.n_future, self.detach_state, self.flow_warp, self.prob_each_future = n_future, detach_state, flow_warp, prob_each_future
        if self.flow_warp:
            self.offset_conv = ConvBlock(in_channels=latent_dim + in_channels)
            self.offset_pred = nn.Conv2d(latent_dim + in_channels, 2, kernel_size=1, padding=0)
        self._build_cells(in_channels, latent_dim, n_gru_blocks)
        self.spatial_conv = ConvBlock(in_channels=in_channels)
        self.init_weights()

    def init_weights(self):
        if self.flow_warp:
            self.offset_pred.weight.data.normal_(0.0, 0.02)
            self.offset_pred.bias.data.fill_(0)

    def _flow_modules(self, i):
        return self.offset_conv, self.offset_pred

    def _spatial_block(self, i):
        return self.spatial_conv


class ResFuturePredictionV2(_ResFutureBase):
    """ResFuturePrediction with a flow head and a ConvBlock per frame (``with_state_refine``), or ONE of each listed n_future
    times (motion_modules.py:230-325).  Without flow the cell input is (state, sample)."""
    sample_first_without_flow = False

    def __init__(self, in_channels, latent_dim, n_future, detach_state=True, n_gru_blocks=3, flow_warp=True, prob_each_future=False,
                 with_state_refine=True):
        super().__init__()
        _check_channels(in_channels, latent_dim)
        self.in_channels, self.latent_dim = in_channels, latent_dim
        self.n_future, self.detach_state, self.flow_warp, self.prob_each_future = n_future, detach_state, flow_warp, prob_each_future
        self.with_state_refine = with_state_refine
        if self.flow_warp:
            flow_pred = nn.Sequential(ConvBlock(in_channels=latent_dim + in_channels),
                                      nn.Conv2d(latent_dim + in_channels, 2, kernel_size=1, padding=0))
        self._build_cells(in_channels, latent_dim, n_gru_blocks)
        spatial_conv = ConvBlock(in_channels=in_channels)
        if self.with_state_refine:
            clones = lambda m: nn.ModuleList([copy.deepcopy(m) for _ in range(self.n_future)])
        else:
            clones = lambda m: nn.ModuleList([m for _ in range(self.n_future)])
        if self.flow_warp:
            self.flow_preds = clones(flow_pred)
        self.spatial_convs = clones(spatial_conv)
        self.init_weights()

    def init_weights(self):
        if self.flow_warp:
            for flow_pred in self.flow_preds:
                flow_pred[1].weight.data.normal_(0.0, 0.02)
                flow_pred[1].bias.data.fill_(0)

    def _flow_modules(self, i):
        return self.flow_preds[i][0], self.flow_preds[i][1]

    def _spatial_block(self, i):
        return self.spatial_convs[i]


class ResFuturePredictionV1(PackedModule):
    """One GRUCell rolled over the frames on (sample, warped state) from a zero state, the warp replacing the state itself;
    then n_gru_blocks x [ConvBlock + biased 1x1], blocks k >= 1 behind a SpatialGRU over the n_future + 1 frames
    (motion_modules.py:328-431).  Returns (b, n_future + 1, in_channels, h, w), the hidden state first."""

    def __init__(self, in_channels, latent_dim, n_future, n_gru_blocks=3, flow_warp=True, detach_state=False, prob_each_future=False):
        super().__init__()
        if not flow_warp:
            raise NotImplementedError("ResFuturePredictionV1(flow_warp=False): the reference's init_weights reads self.flow_pred "
                                      "unconditionally and cannot construct it either")
        _check_channels(in_channels, latent_dim)
        self.n_future, self.detach_state, self.flow_warp = n_future, detach_state, flow_warp
        self.latent_dim, self.hidden_size, self.n_gru_blocks, self.prob_each_future = latent_dim, in_channels, n_gru_blocks, prob_each_future
        self.flow_pred = nn.Sequential(ConvBlock(in_channels=latent_dim + in_channels),
                                       nn.Conv2d(latent_dim + in_channels, 2, kernel_size=1, padding=0))
        self.spatial_grus = nn.ModuleList()
        self.spatial_convs = nn.ModuleList()
        cin = in_channels + latent_dim
        for i in range(n_gru_blocks):
            self.spatial_grus.append((GRUCell if i == 0 else SpatialGRU)(input_size=cin, hidden_size=in_channels))
            cin = in_channels
            self.spatial_convs.append(nn.Sequential(ConvBlock(in_channels=in_channels),
                                                    nn.Conv2d(in_channels, in_channels, kernel_size=1, padding=0)))
        self.init_weights()

    def init_weights(self):
        self.flow_pred[1].weight.data.normal_(0.0, 0.02)
        self.flow_pred[1].bias.data.fill_(0)

    def _pack(self):
        require_eval(self)
        pk = packing.Pack(None)
        C, L = self.hidden_size, self.latent_dim
        pk.flow = _pack_flow_head(pk, self.flow_pred[0], self.flow_pred[1], L, C)
        pk.spatial = [(_pack_block(pk, sc[0], C), packing.conv_w(pk, sc[1].weight, C, bias=sc[1].bias)) for sc in self.spatial_convs]
        return pk

    def forward_nhwc(self, sn, hid):
        """sample [B, h, w, L (x n_future with prob_each_future)], hidden [B, h, w, C] -> [n_future + 1, B, h, w, C]."""
        B, h, w, Ls = sn.shape
        C, L, T = self.hidden_size, self.latent_dim, self.n_future + 1
        pk = self.packed()
        dev = sn.device
        n_x = self.n_future if self.prob_each_future else 1
        xbuf = torch.empty((n_x, B, h, w, L + C), dtype=torch.float32, device=dev)      # (sample, warped state), sample written once
        for k in range(n_x):
            xbuf[k][..., :L].copy_(sn[..., k * L:(k + 1) * L])
        feat = torch.empty((B, h, w, C + L), dtype=torch.float32, device=dev)
        states = torch.empty((T, B, h, w, C), dtype=torch.float32, device=dev)
        states[0].copy_(hid)
        zeros = torch.zeros((B, h, w, C), dtype=torch.float32, device=dev)
        cw, w_off, b_off = pk.flow
        for i in range(self.n_future):
            k = i if self.prob_each_future else 0
            runtime.conv2d_ex(cw, sn, Ls, k * L, B, h, w, feat, C + L, 0, in1=states[i], in1_cs=C)
            flow_warp_nhwc(states[i], xbuf[k], L + C, L, feat=feat, w_off=w_off, b_off=b_off)
            self.spatial_grus[0].forward_nhwc(xbuf[k], zeros if i == 0 else states[i], out=states[i + 1])
        y = states
        tmp = torch.empty((T * B, h, w, C), dtype=torch.float32, device=dev)
        for k in range(self.n_gru_blocks):
            if k:
                y = self.spatial_grus[k].forward_nhwc(y, zeros)
            blk, one = pk.spatial[k]
            runtime.conv2d_ex(blk, y, C, 0, T * B, h, w, tmp, C, 0)
            y = torch.empty((T, B, h, w, C), dtype=torch.float32, device=dev)
            runtime.conv2d_ex(one, tmp, C, 0, T * B, h, w, y, C, 0)
        return y

    def _forward_torch(self, sample, hidden):
        cur, states = hidden, [hidden]
        dists = torch.split(sample, self.latent_dim, dim=1) if self.prob_each_future else [sample] * self.n_future
        b, _, h, w = hidden.shape
        rnn = torch.zeros((b, self.hidden_size, h, w), dtype=hidden.dtype, device=hidden.device)
        for i in range(self.n_future):
            flow = F.conv2d(conv_block_torch(self.flow_pred[0], torch.cat((dists[i], cur), dim=1)), self.flow_pred[1].weight,
                            self.flow_pred[1].bias)
            cur = warp_with_flow(cur, flow)
            rnn = gru_cell_torch(self.spatial_grus[0], torch.cat((dists[i], cur), dim=1), rnn)
            cur = rnn
            states.append(rnn)
        y = torch.stack(states, dim=1)
        b, t, c, h, w = y.shape
        for k in range(self.n_gru_blocks):
            if k:
                y = spatial_gru_torch(self.spatial_grus[k], y)
            sc = self.spatial_convs[k]
            y = F.conv2d(conv_block_torch(sc[0], y.flatten(0, 1)), sc[1].weight, sc[1].bias).view(b, t, c, h, w)
        return y

    def forward(self, sample_distribution, hidden_state):
        require_eval(self)
        want = self.latent_dim * (self.n_future if self.prob_each_future else 1)
        assert sample_distribution.shape[1] == want and hidden_state.shape[1] == self.hidden_size
        if use_torch_path(sample_distribution, hidden_state, next(self.parameters())):
            with torch.no_grad():
                return self._forward_torch(sample_distribution, hidden_state)
        return runtime.frames_to_nchw_strided(self.forward_nhwc(runtime.to_nhwc(sample_distribution), runtime.to_nhwc(hidden_state)))
