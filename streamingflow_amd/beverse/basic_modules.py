"""MI355X-native counterparts of mmdet3d/models/beverse/models/basic_modules.py: ``ConvBlock``
(:11-64, parameter container), ``Bottleneck`` (:68-178), ``GRUCell`` (:192-222 — one step of the conv-GRU on separate
x and state tensors) and ``SpatialGRU`` (:225-284 — conv-GRU whose candidate is conv+BN+ReLU and whose output is the
state sequence itself, no 1x1 decoder)."""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import runtime
from ..layers.convolutions import Bottleneck  # noqa: F401  (same block, same state_dict keys)
from ..layers.temporal import gru_cell_nhwc, pack_gru_block, spatial_gru_nhwc
from ..runtime import PackedModule


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

    _pack = pack_gru_block

    def forward_nhwc(self, x, state):
        """x [T, B, h, w, Cx], state [B, h, w, C] -> states [T, B, h, w, C]."""
        return spatial_gru_nhwc(self.packed().struct, x, state, self.hidden_size, self.hidden_size)

    def forward(self, x, state=None, flow=None, mode='bilinear'):
        assert len(x.size()) == 5, 'Input tensor must be BxTxCxHxW.'
        if flow is not None:
            raise NotImplementedError("flow warping is not on the StreamingFlow path")
        runtime.require_cuda(x, state)
        b, T, c, h, w = x.size()
        assert c == self.input_size, f'feature sizes must match, got input {c} for layer with size {self.input_size}'
        xn = runtime.frames_to_nhwc(x)
        s0 = (torch.zeros((b, h, w, self.hidden_size), dtype=torch.float32, device=x.device) if state is None
              else runtime.to_nhwc(state))
        return runtime.frames_to_nchw(self.forward_nhwc(xn, s0))


class GRUCell(PackedModule):
    """One conv-GRU step, ``forward(x, state)`` with x (b, input_size, h, w) and state (b, hidden_size, h, w): the cell
    ResFuturePrediction* chain per frame.  Same parameters as ``SpatialGRU``, packed the same way, run by ``gru_cell_nhwc``."""

    def __init__(self, input_size, hidden_size, gru_bias_init=0.0, norm='bn', activation='relu'):
        super().__init__()
        if input_size % 4 or hidden_size % 4:
            raise NotImplementedError("BEVerse GRUCell: channel counts must be multiples of 4 (the kernels move channels in fours)")
        self.input_size, self.hidden_size, self.gru_bias_init = input_size, hidden_size, gru_bias_init
        cat = input_size + hidden_size
        self.conv_update = nn.Conv2d(cat, hidden_size, kernel_size=3, bias=True, padding=1)
        self.conv_reset = nn.Conv2d(cat, hidden_size, kernel_size=3, bias=True, padding=1)
        self.conv_state_tilde = ConvBlock(cat, hidden_size, kernel_size=3, bias=False, norm=norm, activation=activation)

    _pack = pack_gru_block

    def forward_nhwc(self, x, state, out=None):
        """x [n, h, w, input_size], state [n, h, w, hidden_size] -> [n, h, w, hidden_size] (into `out` when given)."""
        return gru_cell_nhwc(self.packed().struct, x, state, out)

    def forward(self, x, state):
        require_eval(self)
        if use_torch_path(x, state, self.conv_update.weight):
            return gru_cell_torch(self, x, state)
        assert x.shape[1] == self.input_size and state.shape[1] == self.hidden_size, (x.shape, state.shape)
        return runtime.to_nchw(self.forward_nhwc(runtime.to_nhwc(x), runtime.to_nhwc(state)))
