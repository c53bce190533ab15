"""IoU and panoptic-quality accumulators for StreamingFlow's evaluation on the MI355X.

Drop-in for ``streamingflow/metrics.py`` (``IntersectionOverUnion`` :15-71, ``PanopticMetric`` :74-261): same
constructor arguments, ``update`` / ``compute`` / ``__call__`` / ``reset`` and state names, no ``pytorch_lightning``.

How it is computed here.  Every statistic of both metrics is a function of joint label histograms:
  * IoU: tp / fp / fn / support of class c are the diagonal, column and row sums of the (target x prediction) histogram.
  * PQ: a frame's segments are the instance ids themselves (id 0 = background "stuff", ids > 0 = vehicle "things");
    the histogram of (ground-truth id, predicted id) gives every intersection, every segment area (its margins) and
    hence every IoU.  A pair is a match when IoU > 0.5; ground-truth / predicted things that are in no match are the
    false negatives / false positives; a matched vehicle whose ground-truth id was matched to a different predicted id
    in an earlier frame is an id switch and counts as one false negative plus one false positive (:190-197).
The histograms of a whole [batch, time] block come from ONE kernel launch (``sf_confusion_frames_fwd``, integer
atomics: exact) and one device -> host copy; the bookkeeping on the resulting few-dozen-entry matrices is numpy.  With a bound on the
ids (``PanopticMetric(max_instances=M)``) the bookkeeping is ``sf_panoptic_score_fwd`` on the device instead and nothing is copied.
"""
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib, runtime
from .runtime import ptr

THING_CLASS = 1     # PanopticMetric derives the semantic map as (instance > 0): every instance is of class 1


def _as_labels(t):
    return t.reshape(-1).to(torch.int64).contiguous()


def confusion(pred, target, K):
    """([K, K] int64 with entry [t, p] = number of positions labelled t in ``target`` and p in ``pred``, device flag
    that is non-zero when a label was outside [0, K))."""
    runtime.require_cuda(pred, target)
    a, b = _as_labels(pred), _as_labels(target)
    if a.numel() != b.numel():
        raise ValueError("prediction and target must have the same number of elements")
    hist = torch.empty((K, K), dtype=torch.int64, device=a.device)
    flag = torch.empty((1,), dtype=torch.int32, device=a.device)
    runtime.call("confusion", ptr(a), ptr(b), a.numel(), int(K), ptr(hist), ptr(flag), device=a.device)
    return hist, flag


def frame_confusions(pred, target, n_frames, K):
    """Per-frame joint histograms [n_frames, K, K] of two label tensors whose leading dims flatten to n_frames."""
    runtime.require_cuda(pred, target)
    a, b = _as_labels(pred), _as_labels(target)
    if a.numel() != b.numel() or a.numel() % n_frames:
        raise ValueError("prediction and target must hold n_frames equally sized maps")
    hist = torch.empty((n_frames, K, K), dtype=torch.int64, device=a.device)
    flag = torch.empty((1,), dtype=torch.int32, device=a.device)
    runtime.call("confusion_frames", ptr(a), ptr(b), a.numel() // n_frames, int(n_frames), int(K), ptr(hist), ptr(flag), device=a.device)
    return hist, flag


class _Accumulator(nn.Module):
    """Named float32 counters that follow the data to its device, reset to zero and sum over ranks."""

    def __init__(self, names, size):
        super().__init__()
        self._counter_names = tuple(names)
        for name in self._counter_names:
            self.register_buffer(name, torch.zeros(size), persistent=False)

    def _accumulate(self, name, increment):
        state = getattr(self, name)
        if state.device != increment.device:        # first update on another device: the state moves, not the data
            for n in self._counter_names:
                setattr(self, n, getattr(self, n).to(increment.device))
            state = getattr(self, name)
        state += increment.to(state.dtype)

    def reset(self):
        for name in self._counter_names:
            getattr(self, name).zero_()

    def forward(self, *args, **kwargs):
        self.update(*args, **kwargs)

    def sync(self):
        """Sum the counters over the ranks of the default process group (the reference's ``dist_reduce_fx='sum'``)."""
        from . import dist
        for name in self._counter_names:
            dist.reduce_counters(getattr(self, name))


class IntersectionOverUnion(_Accumulator):
    def __init__(self, n_classes: int, ignore_index: Optional[int] = None, absent_score: float = 0.0, reduction: str = "none",
                 compute_on_step: bool = False):
        super().__init__(("true_positive", "false_positive", "false_negative", "support"), n_classes)
        if reduction not in ("none", "sum", "elementwise_mean"):
            raise ValueError("Reduction parameter unknown.")
        self.n_classes, self.ignore_index, self.absent_score, self.reduction = n_classes, ignore_index, absent_score, reduction
        self._out_of_range = None       # device flag, OR-ed over every update since the last reset

    def update(self, prediction: torch.Tensor, target: torch.Tensor):
        if prediction.ndim == target.ndim + 1:      # class scores: the predicted label is the arg max over dim 1
            prediction = prediction.argmax(dim=1)
        n = self.n_classes
        hist, flag = confusion(prediction, target, n)          # any label outside [0, n) — n itself included — trips the flag (compute() raises)
        self._out_of_range = flag if self._out_of_range is None else torch.maximum(self._out_of_range, flag)
        hist = hist.to(torch.float32)                           # rows = target classes 0..n-1
        hit = hist.diagonal()
        self._accumulate("true_positive", hit)
        self._accumulate("false_positive", hist.sum(0) - hit)
        self._accumulate("false_negative", hist.sum(1) - hit)
        self._accumulate("support", hist.sum(1))

    def reset(self):
        super().reset()
        self._out_of_range = None

    def compute(self):
        if self._out_of_range is not None and int(self._out_of_range.item()):
            raise RuntimeError("IntersectionOverUnion: a label outside [0, n_classes) was seen")
        tp, fp, fn = self.true_positive, self.false_positive, self.false_negative
        seen = (self.support + tp + fp) > 0
        scores = torch.where(seen, tp / (tp + fp + fn).clamp(min=1), torch.full_like(tp, float(self.absent_score)))
        keep = torch.ones(self.n_classes, dtype=torch.bool, device=scores.device)
        if self.ignore_index is not None and 0 <= self.ignore_index < self.n_classes:
            keep[self.ignore_index] = False
        scores = scores[keep]
        return {"none": lambda s: s, "sum": torch.sum, "elementwise_mean": torch.mean}[self.reduction](scores)


class PanopticMetric(_Accumulator):
    """Panoptic quality of instance id maps (module docstring).  Two paths:

    ``max_instances=None`` (the default): ``update`` sizes its tables from the data — it copies three maxima and then every per-frame
    histogram to the host, scores them in numpy and raises at once on a negative id or a ground truth without background.

    ``max_instances=M`` (an int in 1 .. ``MAX_INSTANCES``): ``update`` only enqueues — the conversion of the maps to int64,
    ``sf_confusion_frames_fwd`` into a [batch * time, M + 1, M + 1] table and ``sf_panoptic_score_fwd``, which adds into the four
    counters in place — and returns; nothing is read back, so a whole evaluation step can be captured in a graph.  The counters are
    bitwise those of the default path.  M MUST bound every id of both maps: the ground-truth ids AND the predicted ids after tracking
    (tracking hands out new ids over a sequence, so a sequence's ids can exceed the 100 raw ids a frame is capped to).  Data errors
    cannot raise in ``update`` any more; they are OR-ed into a device int over the updates since the last ``reset()``: an id of either
    map outside [0, M] (negative ids included), or an update whose ``gt_instance`` holds no pixel of id 0.  Such an update adds nothing
    to the counters, and ``compute()`` — which reads the int once — raises ``ValueError`` naming the cause until ``reset()``.  Frames
    must have fewer than 2^23 pixels, and ``n_classes`` must be at least 2 (class 1 takes the vehicles)."""

    MAX_INSTANCES = _lib.SF_PANOPTIC_MAX_K - 1
    MAX_FRAME_PIXELS = 1 << 23

    def __init__(self, n_classes: int, temporally_consistent: bool = True, vehicles_id: int = 1, compute_on_step: bool = False,
                 max_instances: Optional[int] = None):
        super().__init__(("iou", "true_positive", "false_positive", "false_negative"), n_classes)
        self.keys = list(self._counter_names)
        self.n_classes, self.temporally_consistent, self.vehicles_id = n_classes, temporally_consistent, vehicles_id
        if max_instances is not None:
            if isinstance(max_instances, bool) or not isinstance(max_instances, int) or not 1 <= max_instances <= self.MAX_INSTANCES:
                raise ValueError("max_instances must be an int in 1 .. %d, got %r" % (self.MAX_INSTANCES, max_instances))
            if n_classes < THING_CLASS + 1:
                raise ValueError("max_instances needs n_classes >= 2: class 1 takes the vehicles")
            self.register_buffer("_errors", torch.zeros(1, dtype=torch.int32), persistent=False)      # SF_PANOPTIC_ERR_* bits since reset()
        self.max_instances = max_instances

    def _update_device(self, pred_instance, gt_instance):
        batch, steps, h, w = gt_instance.shape
        if batch * steps < 1 or not 1 <= h * w < self.MAX_FRAME_PIXELS:
            raise ValueError("max_instances: expected at least one frame of 1 .. 2^23 - 1 pixels")
        dev, K = pred_instance.device, self.max_instances + 1
        if self.iou.device != dev:                  # first update on another device: the state moves, not the data
            for n in self._counter_names + ("_errors",):
                setattr(self, n, getattr(self, n).to(dev))
        if any(getattr(self, n).dtype != torch.float32 for n in self._counter_names):
            raise RuntimeError("PanopticMetric: the counters must stay float32")
        hist, flag = frame_confusions(pred_instance, gt_instance, batch * steps, K)
        need = _lib.lib().sf_panoptic_score_ws_bytes(batch, steps, K)      # int32 / fp32 parts: a multiple of 4
        if need == 0:
            raise ValueError("max_instances: batch * time * (max_instances + 1) must stay below 2^31")
        ws = torch.empty(need // 4, dtype=torch.int32, device=dev)
        track = bool(self.temporally_consistent) and THING_CLASS == self.vehicles_id
        runtime.call("panoptic_score", ptr(hist), h * w, batch, steps, K, self.n_classes, int(track), ptr(flag), ptr(self.iou),
                     ptr(self.true_positive), ptr(self.false_positive), ptr(self.false_negative), ptr(self._errors), device=dev, scratch=ws)

    def reset(self):
        super().reset()
        if self.max_instances is not None:
            self._errors.zero_()

    def update(self, pred_instance, gt_instance):
        """pred_instance, gt_instance: [batch, time, H, W] instance ids (0 = background)."""
        runtime.require_cuda(pred_instance, gt_instance)
        if pred_instance.shape != gt_instance.shape or gt_instance.dim() != 4:
            raise ValueError("expected two [batch, time, H, W] id tensors of the same shape")
        if self.max_instances is not None:
            return self._update_device(pred_instance, gt_instance)
        batch, steps = gt_instance.shape[:2]
        top = torch.stack([pred_instance.max(), gt_instance.max(), -gt_instance.min()]).cpu()
        assert int(top[2]) == 0, "ID 0 of gt_instance must be background"
        K = int(max(top[0], top[1])) + 1
        hist, flag = frame_confusions(pred_instance, gt_instance, batch * steps, K)
        hist = hist.cpu().numpy().reshape(batch, steps, K, K)          # the one device -> host copy of this update
        if int(flag.item()):
            raise ValueError("negative instance id")
        tally = {k: np.zeros(self.n_classes, dtype=np.float64) for k in self.keys}
        for b in range(batch):
            partner = {}            # ground-truth vehicle id -> predicted id of its latest match (id switches)
            for t in range(steps):
                self._score_frame(hist[b, t], partner, tally)
        dev = pred_instance.device
        for k in self.keys:
            self._accumulate(k, torch.from_numpy(tally[k]).to(dev))

    def _score_frame(self, joint, partner, tally):
        """joint[g, p]: pixels with ground-truth id g and predicted id p in one frame."""
        area_gt, area_pred = joint.sum(1), joint.sum(0)
        union = (area_gt[:, None] + area_pred[None, :] - joint).astype(np.float32)
        iou = np.where(union > 0, (joint.astype(np.float32) + np.float32(1e-9)) / (union + np.float32(1e-9)), np.float32(0))
        hits = iou > 0.5
        if hits[0, 0]:                                   # the background segment is scored as a class-0 match only
            tally["true_positive"][0] += 1
            tally["iou"][0] += iou[0, 0]
        gt_ids, pred_ids = np.nonzero(hits[1:, 1:])      # thing <-> thing matches, ascending ground-truth id
        gt_ids, pred_ids = gt_ids + 1, pred_ids + 1
        track = self.temporally_consistent and THING_CLASS == self.vehicles_id
        for g, p in zip(gt_ids.tolist(), pred_ids.tolist()):
            switched = track and g in partner and partner[g] != p
            partner[g] = p
            if switched:
                tally["false_negative"][THING_CLASS] += 1
                tally["false_positive"][THING_CLASS] += 1
            else:
                tally["true_positive"][THING_CLASS] += 1
                tally["iou"][THING_CLASS] += iou[g, p]
        present_gt, present_pred = area_gt[1:] > 0, area_pred[1:] > 0
        matched_gt, matched_pred = hits[1:, 1:].any(1), hits[1:, 1:].any(0)
        tally["false_negative"][THING_CLASS] += int(np.count_nonzero(present_gt & ~matched_gt))
        tally["false_positive"][THING_CLASS] += int(np.count_nonzero(present_pred & ~matched_pred))

    def compute(self):
        if self.max_instances is not None:
            bits = int(self._errors.item())
            causes = [text for bit, text in ((_lib.SF_PANOPTIC_ERR_RANGE, "an instance id outside [0, max_instances = %d]" % self.max_instances),
                                             (_lib.SF_PANOPTIC_ERR_NO_BACKGROUND, "an update whose gt_instance has no pixel of id 0 (ID 0 of "
                                                                                  "gt_instance must be background)")) if bits & bit]
            if causes:
                raise ValueError("PanopticMetric: since the last reset() there was " + " and ".join(causes) + "; those updates were not counted")
        one = torch.ones_like(self.true_positive)
        denominator = torch.maximum(self.true_positive + 0.5 * self.false_positive + 0.5 * self.false_negative, one)
        return {"pq": self.iou / denominator, "sq": self.iou / torch.maximum(self.true_positive, one),
                "rq": self.true_positive / denominator}


class PlanningMetric(_Accumulator):
    """``PlanningMetric`` (streamingflow/metrics.py:263-396): per future frame the L2 distance to the ground-truth trajectory, the
    collisions of the planned point (``obj_col``) and of the ego rectangle (``obj_box_col``) with the ground-truth occupancy,
    counted only where the ground-truth trajectory's own rectangle is free.  ``update`` on device tensors is one launch of
    ``sf_plan_metric_fwd`` that adds into the counters; nothing is read back.  CPU tensors (or ``SF_PLAN_TORCH=1``) take the
    plain-torch statement of the same arithmetic."""

    def __init__(self, cfg, n_future=4, compute_on_step: bool = False):
        super().__init__(("obj_col", "obj_box_col", "L2"), n_future)
        from .cost import footprint
        from .models.lift_splat import calculate_birds_eye_view_parameters
        dx, bx, dim = calculate_birds_eye_view_parameters(cfg.LIFT.X_BOUND, cfg.LIFT.Y_BOUND, cfg.LIFT.Z_BOUND)
        self.dx = nn.Parameter(dx[:2].float(), requires_grad=False)
        self.bx = nn.Parameter(bx[:2].float(), requires_grad=False)
        self.bev_dimension = dim.numpy()
        self.W, self.H, self.n_future = cfg.EGO.WIDTH, cfg.EGO.HEIGHT, n_future
        self.register_buffer("total", torch.tensor(0), persistent=False)
        self.register_buffer("_rc", footprint(self.W, self.H, dx[:2].numpy(), bx[:2].numpy()).to(torch.int32), persistent=False)

    def reset(self):
        super().reset()
        self.total.zero_()

    def sync(self):
        """The reference declares ``total`` with ``dist_reduce_fx='sum'`` like the three sums: it is reduced with them."""
        super().sync()
        from . import dist
        dist.reduce_counters(self.total)

    def _box_hit(self, traj, segmentation):
        """traj [B, T, 2] (mirrored), segmentation [B, T, G, G] -> [B, T] bool: the ego rectangle touches an occupied cell.  The
        reference swaps, divides by dx in fp32 and adds the integer table in float64 (numpy) before it truncates."""
        G = segmentation.shape[-1]
        q = (traj[..., [1, 0]] / self.dx).double().unsqueeze(2) + self._rc.double()
        r, c = q[..., 0].long().clamp(0, G - 1), q[..., 1].long().clamp(0, G - 1)
        B, T = traj.shape[:2]
        ii = torch.arange(B, device=traj.device)[:, None, None]
        tt = torch.arange(T, device=traj.device)[None, :, None]
        return (segmentation[ii, tt, r, c] != 0).any(dim=-1)

    def _update_torch(self, trajs, gt_trajs, segmentation):
        G = segmentation.shape[-1]
        flip = torch.tensor([-1, 1], device=trajs.device)
        p, g = trajs[..., :2] * flip, gt_trajs[..., :2] * flip
        gt_hit = self._box_hit(g, segmentation)
        yi = ((p[..., 1] - self.bx[0]) / self.dx[0]).long()
        xi = ((p[..., 0] - self.bx[1]) / self.dx[1]).long()
        inside = (yi >= 0) & (yi < G) & (xi >= 0) & (xi < G) & ~gt_hit
        B, T = p.shape[:2]
        ii = torch.arange(B, device=p.device)[:, None]
        tt = torch.arange(T, device=p.device)[None, :]
        at = segmentation[ii, tt, yi.clamp(0, G - 1), xi.clamp(0, G - 1)].float()
        self.obj_col += torch.where(inside, at, torch.zeros_like(at)).sum(dim=0)
        self.obj_box_col += (self._box_hit(p, segmentation) & ~gt_hit).float().sum(dim=0)
        self.L2 += torch.sqrt(((trajs[..., :2] - gt_trajs[..., :2]) ** 2).sum(dim=-1)).sum(dim=0)
        self.total += len(trajs)

    def update(self, trajs, gt_trajs, segmentation):
        """trajs, gt_trajs [B, T, 3]; segmentation [B, T, G, G] (0 = free)."""
        assert trajs.shape == gt_trajs.shape
        from .cost import occupancy_u8, use_torch_path
        if segmentation.shape[-1] != segmentation.shape[-2]:
            raise NotImplementedError("non-square BEV grids")
        if self.L2.device != trajs.device:                  # first update on another device: the state moves, not the data
            self.to(trajs.device)
        seg = occupancy_u8(segmentation)
        trajs, gt_trajs = runtime.f32c(trajs), runtime.f32c(gt_trajs)
        if use_torch_path(trajs, gt_trajs, seg):
            return self._update_torch(trajs, gt_trajs, seg)
        B, T, s = trajs.shape
        if T != self.n_future or s < 2:
            raise ValueError("expected [B, %d, >= 2] trajectories" % self.n_future)
        runtime.call("plan_metric", ptr(trajs), ptr(gt_trajs), s, ptr(seg), ptr(self._rc), self._rc.shape[0], ptr(self.dx), ptr(self.bx),
                     B, T, seg.shape[-2], seg.shape[-1], ptr(self.obj_col), ptr(self.obj_box_col), ptr(self.L2), ptr(self.total),
                     device=trajs.device)

    def compute(self):
        return {"obj_col": self.obj_col / self.total, "obj_box_col": self.obj_box_col / self.total, "L2": self.L2 / self.total}
