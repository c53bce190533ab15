"""Label preparation of StreamingFlow's evaluation on the MI355X.

Drop-in for ``warp_features`` / ``cumulative_warp_features`` / ``cumulative_warp_features_reverse``
(``streamingflow/utils/geometry.py:196-297``), their helpers ``mat2pose_vec`` / ``invert_pose_matrix`` (:97-121, :175-193)
and ``prepare_future_labels`` (``streamingflow/trainer.py:283-394``; a function of (batch, cfg, receptive_field,
spatial_extent, encoder_downsample) here — the reference method lives on a pytorch_lightning module).

How it is computed here.  Warping a BEV map by an ego-motion is a planar rigid transform: yaw about z plus an (x, y)
shift.  For a sequence the ego-motions are chained as 4x4 matrices first (all samples at once, a handful of tiny
products), each chained matrix is reduced to its (yaw, shift) and turned into one 2x3 sampling matrix, and then ALL
frames of the sequence are resampled by a single launch of ``sf_warp_affine_fwd`` (affine grid + nearest / bilinear
sampling, zeros outside, ``align_corners=False``).  CUDA tensors only.

The labels themselves — ``convert_instance_mask_to_center_and_offset_label`` (``streamingflow/utils/instance.py:12-77``,
called by both data loaders) and its batched form ``instance_labels``: the centerness heat map, the centre offsets and the
future displacements of B sequences of T instance maps come from ``sf_instance_labels_fwd``, two launches for all B*T
frames (moments of every instance in the plain and the ego-motion-warped maps, then the per-pixel labels) instead of the
reference's Python loop over instances x frames.  ``prepare_future_labels`` derives them from ``batch["instance"]`` when
a batch does not carry them.
"""
import torch

from . import runtime
from .models.lift_splat import pose_vec2mat
from .runtime import ptr


def mat2pose_vec(matrix):
    """[..., 4, 4] rigid transform -> [..., 6] (x, y, z, rot_x, rot_y, rot_z), Euler angles of R = Rx Ry Rz."""
    r = matrix[..., :3, :3]
    rot_x = torch.atan2(-r[..., 1, 2], r[..., 2, 2])
    rot_y = torch.atan2(r[..., 0, 2], torch.sqrt(r[..., 1, 2] ** 2 + r[..., 2, 2] ** 2))
    rot_z = torch.atan2(-r[..., 0, 1], r[..., 0, 0])
    return torch.cat((matrix[..., :3, 3], torch.stack((rot_x, rot_y, rot_z), dim=-1)), dim=-1)


def invert_pose_matrix(x):
    """[n, 4, 4] rigid transforms -> their inverses ([R | t]^-1 = [R^T | -R^T t])."""
    assert x.dim() == 3 and x.shape[1:] == (4, 4), "Only works for batch of pose matrices."
    inv = torch.zeros_like(x)
    rt = x[:, :3, :3].transpose(1, 2)
    inv[:, :3, :3] = rt
    inv[:, :3, 3:] = -torch.bmm(rt, x[:, :3, 3:])
    inv[:, 3, 3] = 1.0
    return inv


def _sampling_matrices(pose, spatial_extent):
    """[n, 6] pose vectors -> [n, 6] row-major 2x3 matrices for F.affine_grid-style sampling: rotation by the yaw, the
    metric shift normalised by the half extents of the grid (x is mirrored: image rows grow towards -x)."""
    yaw = pose[:, 5]
    c, s = torch.cos(yaw), torch.sin(yaw)
    shift_rows = -(pose[:, 0] / spatial_extent[0])
    shift_cols = pose[:, 1] / spatial_extent[1]
    return torch.stack([c, -s, shift_cols, s, c, shift_rows], dim=-1).float().contiguous()


def _resample(maps, theta, mode):
    """maps [n, c, h, w], theta [n, 6] -> resampled maps, one launch for all n."""
    if mode not in ("nearest", "bilinear"):
        raise ValueError(mode)
    runtime.require_cuda(maps, theta)
    n, c, h, w = maps.shape
    src = runtime.f32c(maps)
    dst = torch.empty_like(src)
    runtime.call("warp_affine", ptr(src), ptr(theta), n, c, h, w, int(mode == "bilinear"), ptr(dst), device=maps.device)
    return dst.to(maps.dtype)


def warp_features(x, flow, mode="nearest", spatial_extent=None):
    """x [b, c, h, w] BEV maps, flow [b, 6] ego-motion pose vectors -> the maps seen from the moved ego frame."""
    if flow is None:
        return x
    return _resample(x, _sampling_matrices(flow, spatial_extent), mode)


def _warp_sequence(x, chained, keep, mode, spatial_extent):
    """x [b, T, c, h, w]; chained[t]: [b, 4, 4] transform of frame t (None for the frames listed in ``keep``, which are
    copied): every other frame is resampled, all of them in one launch."""
    b, T = x.shape[:2]
    moved = [t for t in range(T) if t not in keep]
    out = x.clone()
    if moved:
        poses = mat2pose_vec(torch.stack([chained[t] for t in moved], dim=1)).reshape(b * len(moved), 6)
        maps = x[:, moved].reshape((b * len(moved),) + tuple(x.shape[2:]))
        out[:, moved] = _resample(maps, _sampling_matrices(poses, spatial_extent), mode).view((b, len(moved)) + tuple(x.shape[2:]))
    return out


def cumulative_warp_features(x, flow, mode="nearest", spatial_extent=None):
    """Past frames into the LAST frame's ego frame: frame t is moved by flow[t] ... flow[T-2] chained (flow[t] takes frame
    t to frame t+1)."""
    T = x.shape[1]
    if T == 1:
        return x
    step = pose_vec2mat(flow)
    chained = {T - 2: step[:, T - 2]}
    for t in range(T - 3, -1, -1):
        chained[t] = step[:, t] @ chained[t + 1]
    return _warp_sequence(x, chained, {T - 1}, mode, spatial_extent)


def cumulative_warp_features_reverse(x, flow, mode="nearest", spatial_extent=None):
    """Future frames into the FIRST frame's ego frame: frame i is moved back by the inverses of flow[0] ... flow[i-1]."""
    T = x.shape[1]
    step = pose_vec2mat(flow)
    chained = {}
    for i in range(1, T):
        back = invert_pose_matrix(step[:, i - 1])
        chained[i] = back if i == 1 else chained[i - 1] @ back
    return _warp_sequence(x, chained, {0}, mode, spatial_extent)


def _label_moments(ws, frames, num_instances):
    """The moments ``sf_instance_labels_fwd`` left in its workspace (layout: include/sfnative.h), as copies: counts [F, K + 1]
    int32 and (row, col) sums [F, K + 1, 2] int64 of the plain maps, then the same of the warped maps."""
    n = frames * (num_instances + 1)
    raw = ws.view(torch.uint8)
    ac, asum = (n * 4 + 255) // 256 * 256, (n * 16 + 255) // 256 * 256
    out, at = [], 0
    for _ in range(2):
        out.append(raw[at:at + n * 4].view(torch.int32).view(frames, num_instances + 1).clone())
        out.append(raw[at + ac:at + ac + n * 16].view(torch.int64).view(frames, num_instances + 1, 2).clone())
        at += ac + asum
    return tuple(out)


def instance_labels(instance, future_egomotion, num_instances, ignore_index=255, subtract_egomotion=True, sigma=3, spatial_extent=None,
                    return_moments=False):
    """instance [B, T, H, W] integer ids (1..num_instances; anything else is background), future_egomotion [B, T, 6] ->
    (centerness [B, T, 1, H, W], offset [B, T, 2, H, W], flow [B, T, 2, H, W]) fp32 on the device: per sequence what the
    reference's ``convert_instance_mask_to_center_and_offset_label`` returns.  Two launches for all B*T frames; nothing is
    read back.  ``return_moments`` adds the per (frame, id) counts and sums of the plain and the warped maps (``_label_moments``)."""
    if not subtract_egomotion:
        raise NotImplementedError("subtract_egomotion=False is a NameError in the reference (instance.py:28): there is nothing to match")
    if spatial_extent is None:
        raise ValueError("spatial_extent (half extents of the grid in metres) is needed to warp the instance maps")
    if instance.dim() != 4 or tuple(future_egomotion.shape) != tuple(instance.shape[:2]) + (6,):
        raise AssertionError("instance must be [B, T, H, W] and future_egomotion [B, T, 6]")
    runtime.require_cuda(instance, future_egomotion)
    B, T, H, W = instance.shape
    K = int(num_instances)
    ids = instance.detach().to(torch.int64).contiguous()
    dev = ids.device
    # frame t is resampled by the inverse of ego-motion t - 1; frame 0 is never looked at warped: identity
    poses = torch.zeros((B, T, 6), dtype=torch.float32, device=dev)
    if T > 1:
        step = pose_vec2mat(future_egomotion[:, :-1].float()).reshape(B * (T - 1), 4, 4)
        poses[:, 1:] = mat2pose_vec(invert_pose_matrix(step)).view(B, T - 1, 6)
    theta = _sampling_matrices(poses.view(B * T, 6), spatial_extent)
    center = torch.empty((B, T, 1, H, W), dtype=torch.float32, device=dev)
    offset = torch.empty((B, T, 2, H, W), dtype=torch.float32, device=dev)
    flow = torch.empty((B, T, 2, H, W), dtype=torch.float32, device=dev)
    ws = runtime.call("instance_labels", ptr(ids), ptr(theta), B, T, H, W, K, float(sigma), float(ignore_index), ptr(center), ptr(offset),
                      ptr(flow), device=dev, scratch=("instance_labels", B, T, H, W, K))
    if return_moments:
        return center, offset, flow, _label_moments(ws, B * T, K)
    return center, offset, flow


def convert_instance_mask_to_center_and_offset_label(instance_img, future_egomotion, num_instances, ignore_index=255,
                                                     subtract_egomotion=True, sigma=3, spatial_extent=None):
    """instance_img [T, H, W], future_egomotion [T, 6] -> (centerness [T, 1, H, W], offset [T, 2, H, W], future displacement
    [T, 2, H, W]): the reference's function of the same name, on the device (``instance_labels`` with B = 1)."""
    if instance_img.dim() != 3:
        raise AssertionError("instance_img must be [T, H, W]")
    c, o, f = instance_labels(instance_img.unsqueeze(0), future_egomotion.unsqueeze(0), num_instances, ignore_index=ignore_index,
                              subtract_egomotion=subtract_egomotion, sigma=sigma, spatial_extent=spatial_extent)
    return c[0], o[0], f[0]


def prepare_future_labels(batch, cfg, receptive_field, spatial_extent, encoder_downsample=8, is_lyft=False):
    """Every label sequence of a batch in the PRESENT frame (index receptive_field - 1): the past is warped forward, the
    future backward, and the two halves are joined without repeating the present.  A batch without ``centerness``,
    ``offset`` or ``flow`` gets the missing ones from its ``instance`` maps (``instance_labels``, with the data loaders'
    arguments: every positive id an instance, cfg.DATASET.IGNORE_INDEX or 255, sigma 3)."""
    rf = receptive_field
    ego = batch["future_egomotion"]
    needed = (("centerness", "offset") if cfg.INSTANCE_SEG.ENABLED else ()) + (("flow",) if cfg.INSTANCE_FLOW.ENABLED else ())
    if any(k not in batch for k in needed):
        ignore = getattr(getattr(cfg, "DATASET", None), "IGNORE_INDEX", 255)
        made = instance_labels(batch["instance"], ego, max(int(batch["instance"].max().item()), 0), ignore_index=ignore, spatial_extent=spatial_extent)
        batch = {**dict(zip(("centerness", "offset", "flow"), made)), **batch}
    labels = {}
    if not is_lyft and "gt_trajectory" in batch:
        labels["gt_trajectory"] = batch["gt_trajectory"]
    if cfg.LIFT.GT_DEPTH and "depths" in batch:
        lo, hi = cfg.LIFT.D_BOUND[0], cfg.LIFT.D_BOUND[1]
        bins = batch["depths"][:, :rf, :, ::encoder_downsample, ::encoder_downsample].clamp(lo, hi - 1) - lo
        labels["depths"] = bins.long().contiguous()

    def to_present(seq, categorical, channel_less=False):
        maps = seq.float() if categorical else seq
        if channel_less:
            maps = maps.unsqueeze(2)
        past = cumulative_warp_features(maps[:, :rf], ego[:, :rf], mode="nearest", spatial_extent=spatial_extent)[:, :-1]
        future = cumulative_warp_features_reverse(maps[:, rf - 1:], ego[:, rf - 1:], mode="nearest", spatial_extent=spatial_extent)
        joined = torch.cat([past, future], dim=1)
        if categorical:
            joined = joined.long()
        return joined[:, :, 0].contiguous() if channel_less else joined.contiguous()

    labels["segmentation"] = to_present(batch["segmentation"], True)
    if cfg.SEMANTIC_SEG.PEDESTRIAN.ENABLED:
        labels["pedestrian"] = to_present(batch["pedestrian"], True)
    if cfg.INSTANCE_SEG.ENABLED:
        labels["instance"] = to_present(batch["instance"], True, channel_less=True)
        labels["centerness"] = to_present(batch["centerness"], False)
        labels["offset"] = to_present(batch["offset"], False)
    if cfg.INSTANCE_FLOW.ENABLED:
        labels["flow"] = to_present(batch["flow"], False)
    return labels
