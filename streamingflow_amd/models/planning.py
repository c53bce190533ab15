"""``Planning`` — trajectory scoring, selection and refinement on the MI355X.

Drop-in for ``streamingflow/models/planning_model.py``: same constructor, the reference's attribute names (``cost_function``,
``reduce_channel``, ``GRU``, ``decoder``) and therefore its ``state_dict`` keys and shapes; ``forward`` returns ``(0, output_traj)``.
Inference only: ``loss`` is not built and ``forward`` in training mode raises.

How it is computed here.  The command slicing (a third of the samples, repeated three times) and the reduction of the HD-map logits
stay in torch.  Then three native steps: ``sf_plan_cost_fwd`` scores all B x N trajectories, the ``reduce_channel`` bottlenecks run
on the convolution kernels, and ``sf_plan_select_refine_fwd`` — one workgroup per sample — takes the arg-min over N (lowest index on
a tie; the reference's ``topk(k=1, largest=False)``), gathers the trajectory and runs the GRU refinement loop with the hidden state
in LDS.  Nothing is read back, so the sequence can be captured in a graph.

The plain-torch path (CPU inputs or ``SF_PLAN_TORCH=1``) states the same semantics with ``nn.GRUCell`` / ``nn.Linear`` themselves.
"""
import torch
import torch.nn as nn

from .. import runtime
from ..cost import Cost_Function, use_torch_path
from ..layers.convolutions import Bottleneck
from ..runtime import ptr

MAX_STATE = 256     # csrc/plan_kernels.hip keeps h, the gates and the hidden layer in LDS


def _bottleneck_torch(block, x):
    """convolutions.py:161-169 on the block's own torch layers."""
    residual = block.layers(x)
    if block.projection is None:
        return residual + x
    if block._downsample:
        x = nn.functional.pad(x, (0, x.shape[-1] % 2, 0, x.shape[-2] % 2), value=0)
    return residual + block.projection(x)


class Planning(nn.Module):
    def __init__(self, cfg, feature_channel, gru_input_size=6, gru_state_size=256):
        super().__init__()
        self.cost_function = Cost_Function(cfg)
        self.sample_num = cfg.PLANNING.SAMPLE_NUM
        self.commands = cfg.PLANNING.COMMAND
        assert self.sample_num % 3 == 0
        self.num = int(self.sample_num / 3)
        self.reduce_channel = nn.Sequential(
            Bottleneck(feature_channel, feature_channel, downsample=True),
            Bottleneck(feature_channel, int(feature_channel / 2), downsample=True),
            Bottleneck(int(feature_channel / 2), int(feature_channel / 2), downsample=True),
            Bottleneck(int(feature_channel / 2), int(feature_channel / 8)))
        self.GRU = nn.GRUCell(gru_input_size, gru_state_size)
        self.decoder = nn.Sequential(nn.Linear(gru_state_size, gru_state_size), nn.ReLU(inplace=True), nn.Linear(gru_state_size, 2))

    def loss(self, *args, **kwargs):
        raise NotImplementedError("streamingflow_amd is inference-only: the planner's training loss is not built")

    # ---- selection ------------------------------------------------------------------------------------------------------------
    def _pick(self, cs, trajs, target_points=None, h0=None):
        """cs [B, N], trajs [B, N, T, 3] -> (selected [B, T, 3], refined [B, T, 3] or None without h0): one launch."""
        B, N, T = trajs.shape[:3]
        S = 0 if h0 is None else h0.shape[1]
        if S > MAX_STATE or (S and self.GRU.input_size != 6):
            raise NotImplementedError("the refinement kernel holds a GRU state of at most %d and the reference's 6 inputs" % MAX_STATE)
        trajs = runtime.f32c(trajs)
        dev = trajs.device
        selected = torch.empty((B, T, 3), dtype=torch.float32, device=dev)
        refined = torch.empty((B, T, 3), dtype=torch.float32, device=dev) if S else None
        g, d = self.GRU, self.decoder
        w = [runtime.f32c(t) for t in (g.weight_ih, g.weight_hh, g.bias_ih, g.bias_hh, d[0].weight, d[0].bias, d[2].weight, d[2].bias)] if S else [None] * 8
        target = runtime.f32c(target_points) if S else None
        h0 = runtime.f32c(h0) if S else None
        runtime.call("plan_select_refine", ptr(cs), ptr(trajs), 3, ptr(target), ptr(h0), *[ptr(t) for t in w], B, N, T, S,
                     ptr(selected), ptr(refined), device=dev)
        return selected, refined

    def select(self, trajs, cost_volume, semantic_pred, lane_divider, drivable_area, target_points, k=1):
        """trajs [B, N, T, 3] -> the lowest-cost trajectory of every sample [B, T, 3]."""
        if k != 1:
            raise NotImplementedError("select: k = 1 only")
        if trajs.shape[-1] != 3:
            raise ValueError("trajs must be [B, N, T, 3]")
        with torch.no_grad():
            _, _, cs = self.cost_function.costs(cost_volume, trajs[:, :, :, :2], semantic_pred, lane_divider, drivable_area, target_points)
            if use_torch_path(cs, trajs):
                best = torch.argmin(cs, dim=-1)             # the first of equal minima
                return trajs[torch.arange(len(trajs), device=trajs.device), best]
            return self._pick(cs, trajs)[0]

    # ---- forward --------------------------------------------------------------------------------------------------------------
    def _command_trajs(self, trajs, commands):
        cur = []
        for traj, command in zip(trajs, commands):
            if command == "LEFT":
                cur.append(traj[:self.num].repeat(3, 1, 1))
            elif command == "FORWARD":
                cur.append(traj[self.num:self.num * 2].repeat(3, 1, 1))
            elif command == "RIGHT":
                cur.append(traj[self.num * 2:].repeat(3, 1, 1))
            else:
                cur.append(traj)
        return torch.stack(cur)

    def forward(self, cam_front, trajs, gt_trajs, cost_volume, semantic_pred, hd_map, commands, target_points):
        """cam_front [B, C, h, w]; trajs [B, N, T, 3]; gt_trajs unused (inference); cost_volume, semantic_pred [B, T, G, G];
        hd_map [B, 2 | 4, G, G]; commands: B strings; target_points [B, 2] -> (0, output_traj [B, T, 3])."""
        if self.training:
            raise RuntimeError("streamingflow_amd is inference-only: call .eval() (the planner's loss is not built)")
        if hd_map.shape[1] == 2:
            lane_divider, drivable_area = hd_map[:, 0:1], hd_map[:, 1:2]
        elif hd_map.shape[1] == 4:
            lane_divider, drivable_area = hd_map[:, 0:2], hd_map[:, 2:4]
        else:
            raise NotImplementedError
        with torch.no_grad():
            cur = self._command_trajs(trajs, commands)
            if use_torch_path(cam_front, cur, cost_volume, target_points, self.GRU.weight_hh):
                return 0, self._forward_torch(cam_front, cur, cost_volume, semantic_pred, lane_divider, drivable_area, target_points)
            if cam_front.shape[1] % 32:
                raise NotImplementedError("Planning on the device: feature_channel must be a multiple of 32 (the convolution kernels move "
                                          "channels in fours and the last bottleneck of reduce_channel has feature_channel / 8 of them)")
            _, _, cs = self.cost_function.costs(cost_volume, cur, semantic_pred, lane_divider, drivable_area, target_points)
            x = runtime.to_nhwc(cam_front)
            for block in self.reduce_channel:
                x = block.forward_nhwc(x)
            h0 = runtime.to_nchw(x).flatten(start_dim=1)
            if h0.shape[1] != self.GRU.hidden_size:
                raise ValueError("reduce_channel(cam_front) has %d features, the GRU state %d" % (h0.shape[1], self.GRU.hidden_size))
            return 0, self._pick(cs, cur, target_points, h0)[1]

    def _forward_torch(self, cam_front, cur, cost_volume, semantic_pred, lane_divider, drivable_area, target_points):
        x = cam_front
        for block in self.reduce_channel:
            x = _bottleneck_torch(block, x)
        h = x.flatten(start_dim=1)
        final = self.select(cur, cost_volume, semantic_pred, lane_divider, drivable_area, target_points)
        target_points = target_points.to(dtype=h.dtype)
        x = torch.zeros((final.shape[0], 2), device=h.device)
        out = []
        for i in range(final.shape[1]):
            x = torch.cat([x, final[:, i, :2], target_points], dim=-1)
            h = self.GRU(x, h)
            x = self.decoder(h)
            out.append(x)
        out = torch.stack(out, dim=1)
        return torch.cat([out, torch.zeros((*out.shape[:-1], 1), device=out.device)], dim=-1)
