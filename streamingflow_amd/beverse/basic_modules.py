"""MI355X-native counterparts of mmdet3d/models/beverse/models/basic_modules.py: ``ConvBlock``
(:11-64, parameter container), ``Bottleneck`` (:68-178), ``GRUCell`` (:192-222 — one step of the conv-GRU on separate
x and state tensors) and ``SpatialGRU`` (:225-284 — conv-GRU whose candidate is conv+BN+ReLU and whose output is the
state sequence itself, no 1x1 decoder)."""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib, packing, runtime
from ..layers.convolutions import Bottleneck  # noqa: F401  (same block, same state_dict keys)
from ..runtime import PackedModule, ptr


class ConvBlock(nn.Module):
    def __init__(self, in_channels, out_channels=None, kernel_size=3, stride=1, norm='bn', activation='relu',
                 bias=False, transpose=False):
        super().__init__()
        if transpose or norm != 'bn' or activation != 'relu' or stride != 1:
            raise NotImplementedError("BEVerse ConvBlock: conv + BatchNorm + ReLU form only")
        out_channels = out_channels or in_channels
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding=int((kernel_size - 1) / 2), bias=bias)
        self.norm = nn.BatchNorm2d(out_channels)
        self.activation = nn.ReLU(inplace=True)


def use_torch_path(*tensors):
    """The ResFuturePrediction family states its wiring a second time in plain torch ops: taken for CPU tensors or with
    SF_BEVERSE_TORCH=1 (the baseline tools/resfuturebench.py measures the device path against)."""
    return os.environ.get("SF_BEVERSE_TORCH") == "1" or not all(t.is_cuda for t in tensors)


def require_eval(mod):
    if mod.training:
        raise RuntimeError("streamingflow_amd is inference-only: call .eval()")


def conv_block_torch(blk, x):
    """ConvBlock.forward (basic_modules.py:58-65) in eval mode: conv + BatchNorm (running statistics) + ReLU."""
    n = blk.norm
    y = F.conv2d(x, blk.conv.weight, blk.conv.bias, padding=blk.conv.padding)
    return F.relu(F.batch_norm(y, n.running_mean, n.running_var, n.weight, n.bias, False, 0.0, n.eps))


def gru_cell_torch(cell, x, state):
    """GRUCell.forward / SpatialGRU.gru_cell (basic_modules.py:208-222, :270-284) on the parameters of `cell`."""
    xs = torch.cat([x, state], dim=1)
    update = torch.sigmoid(F.conv2d(xs, cell.conv_update.weight, cell.conv_update.bias, padding=1) + cell.gru_bias_init)
    reset = torch.sigmoid(F.conv2d(xs, cell.conv_reset.weight, cell.conv_reset.bias, padding=1) + cell.gru_bias_init)
    tilde = conv_block_torch(cell.conv_state_tilde, torch.cat([x, (1.0 - reset) * state], dim=1))
    return (1.0 - update) * state + update * tilde


def spatial_gru_torch(gru, x, state=None):
    """SpatialGRU.forward (basic_modules.py:244-268, flow=None): x [b, T, c, h, w] -> the states [b, T, C, h, w]."""
    b, T, _, h, w = x.shape
    s = torch.zeros((b, gru.hidden_size, h, w), dtype=x.dtype, device=x.device) if state is None else state
    out = []
    for t in range(T):
        s = gru_cell_torch(gru, x[:, t], s)
        out.append(s)
    return torch.stack(out, dim=1)


class SpatialGRU(PackedModule):
    def __init__(self, input_size, hidden_size, gru_bias_init=0.0, norm='bn', activation='relu'):
        super().__init__()
        self.input_size, self.hidden_size, self.gru_bias_init = input_size, hidden_size, gru_bias_init
        cat = input_size + hidden_size
        self.conv_update = nn.Conv2d(cat, hidden_size, kernel_size=3, bias=True, padding=1)
        self.conv_reset = nn.Conv2d(cat, hidden_size, kernel_size=3, bias=True, padding=1)
        self.conv_state_tilde = ConvBlock(cat, hidden_size, kernel_size=3, bias=False, norm=norm, activation=activation)

    def _pack(self):
        if self.training:
            raise RuntimeError("streamingflow_amd is inference-only: call .eval()")
        pk = packing.Pack(_lib.GruW())
        s = pk.struct
        wg = torch.cat([self.conv_update.weight, self.conv_reset.weight], 0)
        bg = torch.cat([self.conv_update.bias, self.conv_reset.bias], 0) + float(self.gru_bias_init)
        s.gates = packing.conv_w(pk, wg, self.input_size, self.hidden_size, bias=bg, act="sigmoid")
        sc, bi = packing.bn_fold(self.conv_state_tilde.norm)
        s.cand = packing.conv_w(pk, self.conv_state_tilde.conv.weight, self.input_size, self.hidden_size, scale=sc,
                                bias=bi, act="relu")
        return pk

    def forward_nhwc(self, x, state):
        """x [T, B, h, w, Cx], state [B, h, w, C] -> states [T, B, h, w, C]."""
        T, B, h, w, _ = x.shape
        L = _lib.lib()
        ws = runtime.workspace(L.sf_spatial_gru_ws_bytes(self.hidden_size, B, h, w), x.device)
        out = torch.empty((T, B, h, w, self.hidden_size), dtype=torch.float32, device=x.device)
        _lib.check(L.sf_spatial_gru_fwd(self.packed().struct, ptr(x), ptr(state), ptr(out), T, B, h, w, ptr(ws),
                                        ws.numel() * 4, runtime.stream_ptr(x.device)), "beverse_spatial_gru")
        return out

    def forward(self, x, state=None, flow=None, mode='bilinear'):
        assert len(x.size()) == 5, 'Input tensor must be BxTxCxHxW.'
        if flow is not None:
            raise NotImplementedError("flow warping is not on the StreamingFlow path")
        runtime.require_cuda(x, state)
        b, T, c, h, w = x.size()
        assert c == self.input_size, f'feature sizes must match, got input {c} for layer with size {self.input_size}'
        xn = runtime.to_nhwc(x.reshape(b * T, c, h, w)).view(b, T, h, w, c).permute(1, 0, 2, 3, 4).contiguous()
        s0 = (torch.zeros((b, h, w, self.hidden_size), dtype=torch.float32, device=x.device) if state is None
              else runtime.to_nhwc(state))
        out = self.forward_nhwc(xn, s0).permute(1, 0, 2, 3, 4).reshape(b * T, h, w, self.hidden_size)
        return runtime.to_nchw(out).view(b, T, self.hidden_size, h, w)


class GRUCell(PackedModule):
    """One conv-GRU step, ``forward(x, state)`` with x (b, input_size, h, w) and state (b, hidden_size, h, w): the cell
    ResFuturePrediction* chain per frame.  Same parameters as ``SpatialGRU``, packed the same way, run by ``sf_gru_cell_fwd``."""

    def __init__(self, input_size, hidden_size, gru_bias_init=0.0, norm='bn', activation='relu'):
        super().__init__()
        if input_size % 4 or hidden_size % 4:
            raise NotImplementedError("BEVerse GRUCell: channel counts must be multiples of 4 (the kernels move channels in fours)")
        self.input_size, self.hidden_size, self.gru_bias_init = input_size, hidden_size, gru_bias_init
        cat = input_size + hidden_size
        self.conv_update = nn.Conv2d(cat, hidden_size, kernel_size=3, bias=True, padding=1)
        self.conv_reset = nn.Conv2d(cat, hidden_size, kernel_size=3, bias=True, padding=1)
        self.conv_state_tilde = ConvBlock(cat, hidden_size, kernel_size=3, bias=False, norm=norm, activation=activation)

    _pack = SpatialGRU._pack

    def forward_nhwc(self, x, state, out=None):
        """x [n, h, w, input_size], state [n, h, w, hidden_size] -> [n, h, w, hidden_size] (into `out` when given)."""
        n, h, w, _ = x.shape
        L = _lib.lib()
        ws = runtime.workspace(L.sf_gru_cell_ws_bytes(self.hidden_size, n, h, w), x.device)
        if out is None:
            out = torch.empty((n, h, w, self.hidden_size), dtype=torch.float32, device=x.device)
        _lib.check(L.sf_gru_cell_fwd(self.packed().struct, ptr(x), ptr(state), ptr(out), n, h, w, ptr(ws), ws.numel() * 4,
                                     runtime.stream_ptr(x.device)), "beverse_gru_cell")
        return out

    def forward(self, x, state):
        require_eval(self)
        if use_torch_path(x, state, self.conv_update.weight):
            return gru_cell_torch(self, x, state)
        assert x.shape[1] == self.input_size and state.shape[1] == self.hidden_size, (x.shape, state.shape)
        return runtime.to_nchw(self.forward_nhwc(runtime.to_nhwc(x), runtime.to_nhwc(state)))
