"""The planner's cost function on the MI355X.

Drop-in for ``streamingflow/cost.py``: ``Cost_Function(cfg)`` with the reference's module tree (``safetycost``, ``headwaycost``,
``lrdividercost``, ``comfortcost``, ``progresscost``, ``rulecost``, ``costvolume``; each holds ``dx`` / ``bx`` — and ``SafetyCost``
``w`` — as frozen parameters, so the ``state_dict`` keys are the reference's) and ``forward(cost_volume, trajs, semantic_pred,
lane_divider, drivable_area, target_point) -> (cost_fc [B, N], cost_fo [B, N, T])``.

How it is computed here.  On the device all seven terms of all B x N trajectories come from ``sf_plan_cost_fwd``: one wavefront
per trajectory walks the T waypoints, its lanes stride over the footprint cells and a butterfly sum forms each area
(csrc/plan_kernels.hip).  The index arithmetic is the reference's operation for operation (mirror x, IEEE division by ``dx``, swap,
add the footprint offset, truncate towards zero, clamp).  What the reference does and this keeps:
  * the grown footprint of ``SafetyCost`` is grown by ``int(LAMBDA / dx[0])`` *metres*;
  * ``Progress`` drops its target term when ``target_points.sum() < 0.5`` over the whole batch (formed on the device);
  * ``LR_divider`` takes the nearest non-zero lane pixel and ignores distances above L = 1 m: only pixels within
    ``ceil(L / min(dx))`` cells of the waypoint's cell can count, so that window is scanned instead of every lane pixel.
The term classes below are the plain-torch statement of the same semantics (batched; no [N, T, n] distance tensor); they run when
the inputs are on the CPU or ``SF_PLAN_TORCH=1``.

Occupancy (``semantic_pred``) is a 0 / 1 mask: bool, integer or float maps are converted to uint8.  The footprint tables are the
integer cells strictly inside the ego rectangle (what ``skimage.draw.polygon`` fills when no corner lies on a lattice line;
a corner on one raises ``ValueError``, because there the two rules could differ).
"""
import ctypes
import math
import os

import numpy as np
import torch
import torch.nn as nn

from . import runtime
from .models.lift_splat import calculate_birds_eye_view_parameters
from .runtime import ptr

HEADWAY_L = 10      # metres kept to the vehicle ahead (cost.py:237)
DIVIDER_L = 1       # metres kept to a lane divider (cost.py:267)
RULE_FACTOR = 5     # cost.py:177


def use_torch_path(*tensors):
    return os.environ.get("SF_PLAN_TORCH") == "1" or not all(t.is_cuda for t in tensors)


def footprint(width, height, dx, bx, lambda_=0):
    """[n, 2] int64 (row, column) cells strictly inside the ego rectangle grown by ``lambda_`` metres, in the order
    ``skimage.draw.polygon`` lists them (rows, then columns ascending): cost.py:68-81 without skimage."""
    pts = np.array([[-height / 2. + 0.5 - lambda_, width / 2. + lambda_], [height / 2. + 0.5 + lambda_, width / 2. + lambda_],
                    [height / 2. + 0.5 + lambda_, -width / 2. - lambda_], [-height / 2. + 0.5 - lambda_, -width / 2. - lambda_]])
    pts = (pts - np.asarray(bx, dtype=np.float32)) / np.asarray(dx, dtype=np.float32)
    if np.any(pts == np.round(pts)):
        raise ValueError("a corner of the ego rectangle lies on an integer grid coordinate: %s" % pts.tolist())
    r0, r1, c0, c1 = pts[:, 0].min(), pts[:, 0].max(), pts[:, 1].min(), pts[:, 1].max()
    rr = np.arange(math.floor(r0) + 1, math.ceil(r1))
    cc = np.arange(math.floor(c0) + 1, math.ceil(c1))
    return torch.from_numpy(np.stack(np.meshgrid(rr, cc, indexing="ij"), -1).reshape(-1, 2).astype(np.int64))


def occupancy_u8(x):
    return x.detach().to(torch.uint8).contiguous()


def single_channel(m, drop_equal):
    """[B, 1 | 2, H, W] map -> [B, H, W]: two channels are logits (softmax, channel 1, values below — ``drop_equal``: not
    above — 0.5 zeroed, as the reference does it); one channel is taken as it is."""
    assert m.ndim == 4, "map ndim should be 4"
    if m.shape[1] == 2:
        p = torch.softmax(m, dim=1)[:, 1]
        return p.masked_fill((p <= 0.5) if drop_equal else (p < 0.5), 0)
    return m[:, 0]


class BaseCost(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        dx, bx, dim = calculate_birds_eye_view_parameters(cfg.LIFT.X_BOUND, cfg.LIFT.Y_BOUND, cfg.LIFT.Z_BOUND)
        self.dx = nn.Parameter(dx[:2].float(), requires_grad=False)
        self.bx = nn.Parameter(bx[:2].float(), requires_grad=False)
        self.bev_dimension = dim
        self.W, self.H = cfg.EGO.WIDTH, cfg.EGO.HEIGHT

    def get_origin_points(self, lambda_=0):
        return footprint(self.W, self.H, self.dx.detach().cpu().numpy(), self.bx.detach().cpu().numpy(), lambda_).to(self.bx.device)

    def _table(self, name, lambda_=0):
        """The footprint table as a non-persistent buffer, built once (it is not part of the reference's ``state_dict``)."""
        if name not in self._buffers:
            self.register_buffer(name, self.get_origin_points(lambda_), persistent=False)
        return self._buffers[name]

    def get_points(self, trajs, rc):
        q = trajs.unsqueeze(3) / self.dx
        q = q[..., [1, 0]] + rc
        rr = q[..., 0].long().clamp(0, int(self.bev_dimension[0]) - 1)
        cc = q[..., 1].long().clamp(0, int(self.bev_dimension[1]) - 1)
        return rr, cc

    def compute_area(self, maps, trajs, rc):
        """maps [B, T, G, G], trajs [B, N, T, 2] (mirrored) -> [B, N, T] sums of the maps over the footprint at every waypoint."""
        rr, cc = self.get_points(trajs, rc)
        B, T = maps.shape[:2]
        ii = torch.arange(B, device=maps.device)[:, None, None, None]
        kk = torch.arange(T, device=maps.device)[None, None, :, None]
        return maps[ii, kk, rr, cc].sum(dim=-1)

    def discretize(self, trajs):
        yi = ((trajs[..., 1] - self.bx[0]) / self.dx[0]).long().clamp(0, int(self.bev_dimension[0]) - 1)
        xi = ((trajs[..., 0] - self.bx[1]) / self.dx[1]).long().clamp(0, int(self.bev_dimension[1]) - 1)
        return yi, xi

    def evaluate(self, trajs, C):
        B, T = C.shape[:2]
        yi, xi = self.discretize(trajs)
        return C[torch.arange(B, device=C.device)[:, None, None], torch.arange(T, device=C.device)[None, None, :], yi, xi]


def _speed(trajs):
    """[B, N, T] distance between consecutive waypoints over 0.5 s; the waypoint before the first is the origin."""
    prev = torch.cat([torch.zeros_like(trajs[:, :, :1]), trajs[:, :, :-1]], dim=2)
    return torch.sqrt(((trajs - prev) ** 2).sum(dim=-1)) / 0.5


class Cost_Volume(BaseCost):
    def __init__(self, cfg):
        super().__init__(cfg)
        self.factor = cfg.COST_FUNCTION.VOLUME

    def forward(self, trajs, cost_volume):
        return self.evaluate(trajs, torch.clamp(cost_volume, 0, 1000)) * self.factor


class Rule(BaseCost):
    def __init__(self, cfg):
        super().__init__(cfg)
        self.factor = RULE_FACTOR

    def forward(self, trajs, drivable_area):
        """drivable_area [B, G, G] (one channel): cells of the footprint that are not drivable."""
        off_road = (drivable_area == 0).to(torch.uint8).unsqueeze(1).expand(-1, trajs.shape[2], -1, -1)
        return self.compute_area(off_road, trajs, self._table("rc0")).float() * self.factor


class SafetyCost(BaseCost):
    def __init__(self, cfg):
        super().__init__(cfg)
        self.w = nn.Parameter(torch.tensor([1., 1.]), requires_grad=False)
        self._lambda = cfg.COST_FUNCTION.LAMBDA
        self.factor = cfg.COST_FUNCTION.SAFETY

    def grown_table(self):
        return self._table("rc_lambda", int(self._lambda / float(self.dx[0])))       # metres, as the reference grows it

    def forward(self, trajs, occupancy):
        sub1 = self.compute_area(occupancy, trajs, self._table("rc0")).float()
        sub2 = self.compute_area(occupancy, trajs, self.grown_table()) * _speed(trajs)
        return (sub1 * self.w[0] + sub2 * self.w[1]) * self.factor


class HeadwayCost(BaseCost):
    def __init__(self, cfg):
        super().__init__(cfg)
        self.L = HEADWAY_L
        self.factor = cfg.COST_FUNCTION.HEADWAY

    def forward(self, trajs, occupancy, drivable_area):
        ahead = trajs.clone()
        ahead[..., 1] = ahead[..., 1] + self.L
        return self.compute_area(occupancy.float() * drivable_area.unsqueeze(1), ahead, self._table("rc0")) * self.factor


class LR_divider(BaseCost):
    def __init__(self, cfg):
        super().__init__(cfg)
        self.L = DIVIDER_L
        self.factor = cfg.COST_FUNCTION.LRDIVIDER
        self.reach = int(math.ceil(self.L / float(self.dx.min())))

    def forward(self, trajs, lane_divider):
        """lane_divider [B, G, G]: (L - d)^2 with d the distance to the nearest non-zero lane pixel, 0 where d > L.  Only the
        (2 reach + 1)^2 cells around a waypoint can be that near."""
        B, G = lane_divider.shape[0], lane_divider.shape[-1]
        yi, xi = self.discretize(trajs)
        bi = torch.arange(B, device=trajs.device)[:, None, None]
        dmin = torch.full(yi.shape, float("inf"), device=trajs.device)
        dxr = torch.flip(self.dx.detach(), dims=(0,))
        for dr in range(-self.reach, self.reach + 1):
            for dc in range(-self.reach, self.reach + 1):
                r, c = yi + dr, xi + dc
                ok = (r >= 0) & (r < G) & (c >= 0) & (c < G)
                on = ok & (lane_divider[bi, r.clamp(0, G - 1), c.clamp(0, G - 1)] != 0)
                d = torch.sqrt(((torch.tensor([dr, dc], device=trajs.device) * dxr) ** 2).sum())
                dmin = torch.where(on, torch.minimum(dmin, d), dmin)
        return ((self.L - dmin) ** 2).masked_fill(dmin > self.L, 0) * self.factor


class Comfort(BaseCost):
    def __init__(self, cfg):
        super().__init__(cfg)
        self.c_lat_acc, self.c_lon_acc, self.c_jerk = 3, 3, 1
        self.factor = cfg.COST_FUNCTION.COMFORT

    def forward(self, trajs):
        T = trajs.shape[2]
        prev = torch.cat([torch.zeros_like(trajs[:, :, :1]), trajs[:, :, :-1]], dim=2)
        vel = (trajs - prev) / 0.5                                   # lateral, longitudinal
        acc = torch.zeros_like(vel)
        if T > 1:
            acc[:, :, 1:] = (vel[:, :, 1:] - vel[:, :, :-1]) / 0.5
        lat = torch.abs(acc[..., 0]).max(dim=-1)[0]
        lon = torch.abs(acc[..., 1]).max(dim=-1)[0]
        ego_v = _speed(trajs)
        ego_acc = torch.zeros_like(ego_v)
        ego_jerk = torch.zeros_like(ego_v)
        if T > 1:
            ego_acc[:, :, 1:] = (ego_v[:, :, 1:] - ego_v[:, :, :-1]) / 0.5
        if T > 2:
            ego_jerk[:, :, 2:] = (ego_acc[:, :, 2:] - ego_acc[:, :, 1:-1]) / 0.5
        jerk = torch.abs(ego_jerk).max(dim=-1)[0]
        sub = torch.zeros_like(lat)
        sub += torch.clamp(lat - self.c_lat_acc, 0, 30) ** 2
        sub += torch.clamp(lon - self.c_lon_acc, 0, 30) ** 2
        sub += torch.clamp(jerk - self.c_jerk, 0, 20) ** 2
        return sub * self.factor


class Progress(BaseCost):
    def __init__(self, cfg):
        super().__init__(cfg)
        self.factor = cfg.COST_FUNCTION.PROGRESS

    def forward(self, trajs, target_points):
        ahead = trajs[..., 1].max(dim=-1)[0]
        to_target = ((trajs[:, :, -1] - target_points.unsqueeze(1)) ** 2).sum(dim=-1)
        drop = target_points.sum() < 0.5                            # over the whole batch; stays on the device
        return (torch.where(drop, torch.zeros_like(to_target), to_target) - ahead) * self.factor


class Cost_Function(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.safetycost = SafetyCost(cfg)
        self.headwaycost = HeadwayCost(cfg)
        self.lrdividercost = LR_divider(cfg)
        self.comfortcost = Comfort(cfg)
        self.progresscost = Progress(cfg)
        self.rulecost = Rule(cfg)
        self.costvolume = Cost_Volume(cfg)
        self.n_future = cfg.N_FUTURE_FRAMES
        self.safetycost._table("rc0")
        self.safetycost.grown_table()                               # raises ValueError for a corner on a lattice line
        for m in (self.headwaycost, self.rulecost):
            m._table("rc0")
        rc = torch.cat([self.safetycost.rc0, self.safetycost.rc_lambda]).to(torch.int32)
        self.register_buffer("_rc_i32", rc, persistent=False)      # both tables for the kernel: rc0, then the grown one
        c = cfg.COST_FUNCTION
        self._factors = tuple(float(v) for v in (c.SAFETY, c.HEADWAY, c.LRDIVIDER, c.COMFORT, c.PROGRESS, RULE_FACTOR, c.VOLUME))

    @staticmethod
    def _maps(cost_volume, semantic_pred, lane_divider, drivable_area):
        if cost_volume.shape[-1] != cost_volume.shape[-2]:
            raise NotImplementedError("non-square BEV grids: the reference's view(B, 1, W, H) scrambles them, there is nothing to match")
        return occupancy_u8(semantic_pred), single_channel(lane_divider, True), single_channel(drivable_area, False)

    def forward(self, cost_volume, trajs, semantic_pred, lane_divider, drivable_area, target_point):
        """cost_volume, semantic_pred [B, T, G, G]; trajs [B, N, T, 2]; lane_divider, drivable_area [B, 1 | 2, G, G];
        target_point [B, 2] -> (cost_fc [B, N], cost_fo [B, N, T])."""
        fc, fo, _ = self.costs(cost_volume, trajs, semantic_pred, lane_divider, drivable_area, target_point)
        return fc, fo

    def costs(self, cost_volume, trajs, semantic_pred, lane_divider, drivable_area, target_point):
        """-> (cost_fc, cost_fo, cs = cost_fc + cost_fo.sum(-1))."""
        occ, lane, drv = self._maps(cost_volume, semantic_pred, lane_divider, drivable_area)
        if use_torch_path(cost_volume, trajs, occ, lane, drv, target_point, self.safetycost.dx):
            return self._costs_torch(cost_volume, trajs[..., :2], occ, lane, drv, target_point)
        return self._costs_device(cost_volume, trajs, occ, lane, drv, target_point)

    def _costs_torch(self, cost_volume, trajs, occ, lane, drv, target_point):
        trajs = trajs * torch.tensor([-1, 1], device=trajs.device)
        safety = torch.clamp(self.safetycost(trajs, occ), 0, 100)
        headway = torch.clamp(self.headwaycost(trajs, occ, drv), 0, 100)
        divider = torch.clamp(self.lrdividercost(trajs, lane), 0, 100)
        comfort = torch.clamp(self.comfortcost(trajs), 0, 100)
        progress = torch.clamp(self.progresscost(trajs, target_point), -100, 100)
        rule = torch.clamp(self.rulecost(trajs, drv), 0, 100)
        volume = torch.clamp(self.costvolume(trajs, cost_volume), 0, 100)
        fo = safety + headway + divider + volume + rule
        fc = comfort + progress
        return fc, fo, fc + fo.sum(dim=-1)

    def _costs_device(self, cost_volume, trajs, occ, lane, drv, target_point):
        B, N, T = trajs.shape[:3]
        G = cost_volume.shape[-1]
        dev = trajs.device
        if tuple(cost_volume.shape) != (B, T, G, G) or tuple(occ.shape) != (B, T, G, G) or tuple(lane.shape) != (B, G, G) or \
                tuple(drv.shape) != (B, G, G) or tuple(target_point.shape) != (B, 2) or trajs.shape[-1] < 2:
            raise ValueError("Cost_Function: cost_volume / semantic_pred [B, T, G, G], maps [B, 1 | 2, G, G], trajs [B, N, T, >= 2], target [B, 2]")
        trajs = trajs.detach()
        if trajs.dtype != torch.float32:
            trajs = trajs.float()
        s = trajs.stride(2)
        if trajs.stride(3) != 1 or s < 2 or trajs.stride(1) != T * s or trajs.stride(0) != N * T * s:
            trajs, s = trajs[..., :2].contiguous(), 2                # anything but whole rows of a [B, N, T, s] tensor: pack
        sc = self.safetycost
        n0, nl = sc.rc0.shape[0], sc.rc_lambda.shape[0]
        rc = self._rc_i32
        fo = torch.empty((B, N, T), dtype=torch.float32, device=dev)
        fc = torch.empty((B, N), dtype=torch.float32, device=dev)
        cs = torch.empty((B, N), dtype=torch.float32, device=dev)
        runtime.call("plan_cost", ptr(trajs), s, ptr(runtime.f32c(cost_volume)), ptr(occ), ptr(runtime.f32c(lane)), ptr(runtime.f32c(drv)),
                     ptr(runtime.f32c(target_point)), ptr(rc), n0, ctypes.c_void_p(rc.data_ptr() + n0 * 8), nl, ptr(sc.dx), ptr(sc.bx),
                     ptr(sc.w), ctypes.byref((ctypes.c_float * 7)(*self._factors)), float(HEADWAY_L), float(DIVIDER_L), B, N, T, G, G, ptr(fo), ptr(fc),
                     ptr(cs), device=dev, scratch=("plan_cost",))
        return fc, fo, cs
