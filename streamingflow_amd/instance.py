"""Instance post-processing of StreamingFlow's evaluation on the MI355X.

Drop-in for the functions of ``streamingflow/utils/instance.py`` that ``evaluate.py`` and ``evaluate_streaming.py`` reach
(``find_instance_centers`` :80-92, ``group_pixels`` :95-116, ``get_instance_segmentation_and_centers`` :119-140,
``update_instance_ids`` :143-160, ``make_instance_seg_consecutive`` :163-168, ``make_instance_id_temporally_consistent``
:171-263, ``make_instance_id_temporally_consistent_short_interval`` :272-368, ``predict_instance_segmentation_and_trajectories``
:370-428, ``predict_instance_segmentation_and_trajectories_short_interval`` :432-490): same names, arguments and results.

How it is computed here.
  * One frame — centres, pixel grouping: one kernel each (``sf_instance_centers_fwd``, ``sf_group_pixels_fwd``);
    relabelling is a look-up table gathered on the device; "make ids consecutive" is the inverse index of a sorted unique.
  * A sequence — ``instance_segmentation_sequence``: centres, grouping and consecutive ids of all B*T frames by
    ``sf_instance_seq_fwd`` (a fixed number of launches, nothing read back; ids are at most ``max_n_instance_centers``).
    Both ``predict_*`` functions go this way: one sequence call, one moments launch, one tracking call, one gather.
    Nothing is copied to the host (with ``compute_matched_centers``: one copy at the end), so a call only enqueues and
    can be captured in a graph behind the forward.
  * Temporal consistency.  The ids a frame ends up with are a relabelling of its own raw instances, so everything the
    matching needs — each raw instance's pixel count, centre, and centre displaced by the predicted flow — is computed
    for ALL frames by one launch (``sf_instance_moments_fwd``: integer atomics, order-independent) and stays on the
    device.  The frame-to-frame assignment (``sf_instance_track_fwd``: one workgroup per pair of frames solves the
    minimum-distance assignment by shortest augmenting paths, one wavefront per sample hands the ids down the frames)
    produces one small table per frame, and the whole sequence is relabelled by a single gather.  The regular matcher
    compares frame t+1 with the flow-displaced centres of frame t (closer than 3 pixels); the short-interval one
    ignores the flow and compares with the plain centres (closer than 10).
  * ``_consistent_tables`` is the statement of that matching on the host (Hungarian method, ``scipy``), the one the
    reference fixtures pin.  ``SF_TRACK_HOST=1`` (read at every call) selects it: one host copy of the moments, the
    matching per sample, one upload.  The device tables equal it wherever every pair of frames has one optimal
    assignment; where several are optimal the device returns one of them, the same on every run.  The stand-alone
    ``make_instance_id_temporally_consistent[_short_interval]`` take arbitrary ids: one ``max().item()`` sizes the
    tables, ids up to ``MAX_TRACK_ID`` go to the device call (its flag is read: ``ValueError`` where scipy raises),
    larger ones to the host path.
CUDA tensors only.
"""
import os
from typing import Tuple

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from . import runtime
from .runtime import ptr

MOMENT_SCALE = 1.0 / 1048576.0      # sf_instance_moments_fwd: flow-warped sums are 2^-20 fixed point
MAX_N_INSTANCE_CENTERS = 100        # the reference's default cut of a frame's centre list; raw ids of a frame are at most this
MAX_TRACK_ID = 128                  # sf_instance_track_fwd: the largest raw id of a frame (its cost matrix lives in LDS)


def find_instance_centers(center_prediction: torch.Tensor, conf_threshold: float = 0.1, nms_kernel_size: float = 3):
    """[1, H, W] centre heat map -> [n, 2] int64 (row, col) of its thresholded 3x3 local maxima, row-major order."""
    if center_prediction.dim() != 3:
        raise AssertionError("center_prediction must be [1, H, W]")
    if nms_kernel_size != 3:
        raise NotImplementedError("only the 3x3 non-maximum suppression the reference uses is built")
    runtime.require_cuda(center_prediction)
    H, W = center_prediction.shape[-2:]
    heat = runtime.f32c(center_prediction).view(H, W)
    found = torch.empty((H * W, 2), dtype=torch.int32, device=heat.device)
    count = torch.empty((), dtype=torch.int32, device=heat.device)
    runtime.call("instance_centers", ptr(heat), H, W, float(conf_threshold), ptr(found), H * W, ptr(count), device=heat.device,
                 scratch=("instance_centers", H, W))
    return found[: int(count.item())].long()


def group_pixels(centers: torch.Tensor, offset_predictions: torch.Tensor, foreground_mask: torch.Tensor = None) -> torch.Tensor:
    """Every pixel votes for the centre nearest to (pixel + predicted offset): [1, H, W] int64 ids from 1 (first centre
    wins ties); pixels outside ``foreground_mask`` (when given) get 0."""
    runtime.require_cuda(centers, offset_predictions)
    H, W = offset_predictions.shape[-2:]
    votes = runtime.f32c(offset_predictions).view(2, H, W)
    if foreground_mask is None:
        inside = torch.ones((H, W), dtype=torch.uint8, device=votes.device)
    else:
        inside = (foreground_mask.reshape(H, W) != 0).to(torch.uint8).contiguous()
    table = centers.to(torch.int32).contiguous()
    ids = torch.empty((1, H, W), dtype=torch.int64, device=votes.device)
    runtime.call("group_pixels", ptr(table), table.shape[0], ptr(votes), ptr(inside), H, W, ptr(ids), device=votes.device)
    return ids


def update_instance_ids(instance_seg, old_ids, new_ids):
    """Relabel: every id listed in ``old_ids`` becomes the matching entry of ``new_ids``, the others stay."""
    dev = instance_seg.device
    old = torch.as_tensor(old_ids, device=dev).long()
    table = torch.arange(int(old.max()) + 1, device=dev)
    table[old] = torch.as_tensor(new_ids, device=dev).long()
    return table[instance_seg].long()


def make_instance_seg_consecutive(instance_seg):
    """Ids become 0..n-1 in the order of their old values."""
    return torch.unique(instance_seg, return_inverse=True)[1].long()


def get_instance_segmentation_and_centers(center_predictions, offset_predictions, foreground_mask, conf_threshold: float = 0.1,
                                          nms_kernel_size: float = 3, max_n_instance_centers: int = MAX_N_INSTANCE_CENTERS) -> Tuple[torch.Tensor, torch.Tensor]:
    """One frame: ([1, H, W] int64 instance map with consecutive ids, [n, 2] centres)."""
    H, W = center_predictions.shape[-2:]
    heat = center_predictions.reshape(1, H, W)
    peaks = find_instance_centers(heat, conf_threshold=conf_threshold, nms_kernel_size=nms_kernel_size)
    if peaks.shape[0] == 0:
        return torch.zeros((1, H, W), dtype=torch.int64, device=heat.device), torch.zeros((0, 2), device=heat.device)
    peaks = peaks[:max_n_instance_centers].clone() if peaks.shape[0] > max_n_instance_centers else peaks
    ids = group_pixels(peaks, offset_predictions.reshape(2, H, W), foreground_mask.reshape(1, H, W))
    return make_instance_seg_consecutive(ids), peaks


def instance_segmentation_sequence(center, offset, foreground, conf_threshold: float = 0.1, nms_kernel_size: float = 3,
                                   max_n_instance_centers: int = MAX_N_INSTANCE_CENTERS, return_centers: bool = False):
    """``get_instance_segmentation_and_centers`` of F frames at once: center [F, 1, H, W] or [F, H, W], offset [F, 2, H, W],
    foreground [F, H, W] -> [F, H, W] int64 with consecutive ids per frame (at most ``max_n_instance_centers``).  Nothing is
    copied to the host, unless ``return_centers``: then also a list of the frames' [n, 2] int64 (row, col) centres."""
    if nms_kernel_size != 3:
        raise NotImplementedError("only the 3x3 non-maximum suppression the reference uses is built")
    runtime.require_cuda(center, offset, foreground)
    if center.dim() == 4:
        if center.shape[1] != 1:
            raise AssertionError("center must be [F, 1, H, W] or [F, H, W]")
        center = center[:, 0]
    F, H, W = center.shape
    if tuple(offset.shape) != (F, 2, H, W) or tuple(foreground.shape) != (F, H, W):
        raise AssertionError("offset must be [F, 2, H, W] and foreground [F, H, W]")
    cap = int(max_n_instance_centers)
    heat, votes = runtime.f32c(center), runtime.f32c(offset)
    inside = (foreground != 0).to(torch.uint8).contiguous()
    dev = heat.device
    found = torch.empty((F, cap, 2), dtype=torch.int32, device=dev)
    count = torch.empty((F,), dtype=torch.int32, device=dev)
    ids = torch.empty((F, H, W), dtype=torch.int64, device=dev)
    runtime.call("instance_seq", ptr(heat), ptr(votes), ptr(inside), F, H, W, float(conf_threshold), cap, ptr(found), ptr(count), ptr(ids),
                 device=dev, scratch=("instance_seq", F, H, W, cap))
    if not return_centers:
        return ids
    kept = count.cpu().clamp(max=cap).tolist()
    return ids, [found[f, :n].long() for f, n in enumerate(kept)]


def _moments_on_device(ids, flow, top, with_tables=False):
    """ids [F, H, W] int64 with values <= ``top``, flow [F, 2, H, W] or None -> ONE int64 device buffer, K = top + 1, n = F * K:
    position sums [n][2] | flow-warped sums [n][2] in 2^-20 fixed point (only with ``flow``) | room for the tables [n] (only
    ``with_tables``) | counts int32 [n].  One launch, nothing read back.  Returns (buffer, sums, warped or None, tables or None,
    counts): views of it."""
    F, H, W = ids.shape
    K = top + 1
    n = F * K
    fl = runtime.f32c(flow).view(F, 2, H, W) if flow is not None else None
    head = 2 * n * (2 if fl is not None else 1)
    tail = head + (n if with_tables else 0)
    buf = torch.empty((tail + (n + 1) // 2,), dtype=torch.int64, device=ids.device)
    pos = buf[:2 * n]
    moved = buf[2 * n:4 * n] if fl is not None else None
    tables = buf[head:tail] if with_tables else None
    cnt = buf[tail:].view(torch.int32)
    runtime.call("instance_moments", ptr(ids), ptr(fl), F, H, W, top, ptr(pos), ptr(moved), ptr(cnt), device=ids.device)
    return buf, pos, moved, tables, cnt


def _moments_to_host(ids, flow, top):
    """ids [F, H, W] int64 with values <= ``top``, flow [F, 2, H, W] or None -> numpy (counts [F, K] int32, position sums
    [F, K, 2] int64, flow-warped sums [F, K, 2] int64 in 2^-20 fixed point or None), K = top + 1: one launch, ONE copy.
    The host path only (``SF_TRACK_HOST=1``, ids above ``MAX_TRACK_ID``, ``instance_moments``)."""
    F, K = ids.shape[0], top + 1
    n = F * K
    buf, _, moved, _, _ = _moments_on_device(ids, flow, top)
    parts = 2 if moved is not None else 1
    host = buf.cpu().numpy()
    counts = host[2 * n * parts:].view(np.int32)[:n].reshape(F, K)
    sums = host[:2 * n].reshape(F, K, 2)
    warped = host[2 * n:4 * n].reshape(F, K, 2) if moved is not None else None
    return counts, sums, warped


def _track_on_device(counts, sums, warped, B, T, K, matching_threshold, tables=None):
    """``sf_instance_track_fwd`` on device moments of B samples of T frames (``warped`` None: the short-interval matcher) ->
    (tables [B*T, K] int64, flags [B] int32), both on the device.  Enqueues only."""
    dev = counts.device
    if tables is None:
        tables = torch.empty((B * T * K,), dtype=torch.int64, device=dev)
    flags = torch.empty((B,), dtype=torch.int32, device=dev)
    runtime.call("instance_track", ptr(counts), ptr(sums), ptr(warped), B, T, K, float(matching_threshold), ptr(tables), ptr(flags),
                 device=dev, scratch=("instance_track", B, T, K))
    return tables.view(B * T, K), flags


def _host_tracking():
    """``SF_TRACK_HOST=1``: the frame-to-frame matching on the host (scipy).  Read at every call."""
    return os.environ.get("SF_TRACK_HOST", "0") == "1"


def _means(counts, sums, scale=1.0):
    """Integer sums / pixel count in float64, then float32 (rows of absent ids are NaN)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return (sums * scale / counts[..., None].astype(np.float64)).astype(np.float32)


def instance_moments(instance_seq, flow_seq=None):
    """instance_seq [F, H, W] int64, flow_seq [F, 2, H, W] or None -> numpy (counts [F, K], centres [F, K, 2] float32,
    flow-displaced centres [F, K, 2] float32 or None), K = largest id + 1; rows of absent ids are NaN."""
    runtime.require_cuda(instance_seq)
    ids = instance_seq.to(torch.int64).contiguous()
    counts, sums, warped = _moments_to_host(ids, flow_seq, int(ids.max().item()))
    return counts, _means(counts, sums), _means(counts, warped, MOMENT_SCALE) if warped is not None else None


def _consistent_tables(counts, centres, anchors, matching_threshold):
    """The frame-to-frame matching of ONE sample, on the host.  counts [T, K] pixels of each raw id, centres [T, K, 2] of the
    raw instances, anchors [T, K, 2] the frame-t positions that the centres of frame t+1 are matched against (the
    flow-displaced centres for the regular matcher, the plain centres for the short-interval one) -> tables [T, K] int64,
    tables[t][raw id] = consistent id.  An instance of frame t+1 inherits the id of the frame-t instance it is assigned to
    (Hungarian method) when they are closer than ``matching_threshold``; otherwise it gets a new id."""
    T, K = counts.shape
    tables = np.tile(np.arange(K, dtype=np.int64), (T, 1))      # frame 0 keeps its ids
    next_new = int(np.flatnonzero(counts[0]).max(initial=0))      # largest id of the first frame
    for t in range(T - 1):
        raw_prev = np.flatnonzero(counts[t][1:]) + 1
        raw_next = np.flatnonzero(counts[t + 1][1:]) + 1
        if raw_prev.size == 0 or raw_next.size == 0:
            continue                                              # nothing to carry over: frame t+1 keeps its raw ids
        order = np.argsort(tables[t][raw_prev], kind="stable")    # previous instances by ascending consistent id
        raw_prev = raw_prev[order]
        carried = tables[t][raw_prev]
        n_next = int(raw_next.max())                              # raw ids are consecutive 1..n_next
        gap = np.linalg.norm(centres[t + 1, 1:n_next + 1][None, :, :] - anchors[t, raw_prev][:, None, :], axis=-1)
        rows, cols = linear_sum_assignment(gap)
        close = gap[rows, cols] < matching_threshold
        table = tables[t + 1]
        table[cols[close] + 1] = carried[rows[close]]
        unmatched = np.setdiff1d(raw_next, cols[close] + 1)       # ascending
        table[unmatched] = next_new + 1 + np.arange(unmatched.size)
        next_new += int(unmatched.size)
    return tables


def _relabel(frames, tables):
    """frames [F, h, w] raw ids, tables [F, K] (numpy) -> [F, h, w]: one gather."""
    lut = torch.from_numpy(tables).to(frames.device)
    return torch.gather(lut, 1, frames.reshape(frames.shape[0], -1).long()).view_as(frames)


def _consistent_sequence(frames, flow, matching_threshold):
    """One sample's [T, h, w] instance maps with arbitrary ids, flow [T, 2, h, w] or None (the short-interval matcher) -> the
    maps with consistent ids.  One ``max().item()`` sizes the tables; ids up to ``MAX_TRACK_ID`` are matched on the device
    (one more ``.item()`` reads the flag: ``ValueError`` where scipy raises), larger ones on the host."""
    ids = frames.to(torch.int64).contiguous()
    top = int(ids.max().item())
    if top > MAX_TRACK_ID or _host_tracking():
        counts, sums, warped = _moments_to_host(ids, flow, top)
        centres = _means(counts, sums)
        anchors = _means(counts, warped, MOMENT_SCALE) if warped is not None else centres
        return _relabel(frames, _consistent_tables(counts, centres, anchors, matching_threshold))
    _, sums, warped, _, counts = _moments_on_device(ids, flow, top)
    tables, flags = _track_on_device(counts, sums, warped, 1, ids.shape[0], top + 1, matching_threshold)
    if int(flags.item()):
        raise ValueError("matrix contains invalid numeric entries")      # scipy's, on the NaN centre of a missing raw id
    return torch.gather(tables, 1, ids.view(ids.shape[0], -1)).view_as(frames)


def make_instance_id_temporally_consistent(pred_inst, future_flow, matching_threshold=3.0):
    """pred_inst [1, T, h, w] per-frame instance maps, future_flow [1, T, 2, h, w] -> [1, T, h, w] with ids that follow the
    instances through time: an instance of frame t+1 inherits the id of the frame-t instance whose flow-displaced centre
    it is assigned to (Hungarian method) when they are closer than ``matching_threshold``; otherwise it gets a new id."""
    assert pred_inst.shape[0] == 1, "Assumes batch size = 1"
    runtime.require_cuda(pred_inst, future_flow)
    return _consistent_sequence(pred_inst[0], future_flow[0], matching_threshold).unsqueeze(0)


def make_instance_id_temporally_consistent_short_interval(pred_inst, future_flow=None, matching_threshold=10.0):
    """The matcher of the streaming evaluator: as ``make_instance_id_temporally_consistent``, but ``future_flow`` is
    ignored — an instance of frame t+1 is matched against the plain centres of the frame-t instances — and matches up
    to 10 pixels are accepted."""
    assert pred_inst.shape[0] == 1, "Assumes batch size = 1"
    runtime.require_cuda(pred_inst)
    return _consistent_sequence(pred_inst[0], None, matching_threshold).unsqueeze(0)


def _predict(output, compute_matched_centers, make_consistent, vehicles_id, short_interval):
    """Both ``predict_*`` functions: the sequence kernels on all B*T frames, one moments launch, the matching of all samples
    (``sf_instance_track_fwd``), one gather with the device tables: nothing is read back unless ``compute_matched_centers``,
    which copies tables and moments once at the end.  ``SF_TRACK_HOST=1``: one host copy of the moments and the host matching
    per sample instead."""
    vehicles = output["segmentation"].detach().argmax(dim=2) == vehicles_id
    B, T, H, W = vehicles.shape
    cap = MAX_N_INSTANCE_CENTERS                                    # the reference calls with the default
    raw = instance_segmentation_sequence(output["instance_center"].detach().reshape(B * T, H, W),
                                         output["instance_offset"].detach().reshape(B * T, 2, H, W), vehicles.reshape(B * T, H, W),
                                         max_n_instance_centers=cap)
    if make_consistent and output["instance_flow"] is None:
        output["instance_flow"] = torch.zeros_like(output["instance_offset"])
    if not make_consistent and not compute_matched_centers:
        return raw.view(B, T, H, W)
    flow = output["instance_flow"].detach().reshape(B * T, 2, H, W) if make_consistent and not short_interval else None
    thr = 10.0 if short_interval else 3.0
    if make_consistent and not _host_tracking():
        K = cap + 1                                                 # raw ids are <= cap by construction
        buf, d_sums, d_warped, d_tables, d_counts = _moments_on_device(raw, flow, cap, with_tables=compute_matched_centers)
        d_tables, _ = _track_on_device(d_counts, d_sums, d_warped, B, T, K, thr, d_tables)
        tracked = torch.gather(d_tables, 1, raw.view(B * T, -1)).view(B, T, H, W)
        if not compute_matched_centers:
            return tracked                                          # nothing was read back
        n = B * T * K
        host = buf.cpu().numpy()                                    # the ONE copy: sums, tables and counts together
        tail = host.size - (n + 1) // 2                             # _moments_on_device: sums | warped sums | tables | counts
        sums = host[:2 * n].reshape(B * T, K, 2)
        tables = host[tail - n:tail].reshape(B * T, K)
        counts = host[tail:].view(np.int32)[:n].reshape(B * T, K)
        return tracked, _tracks(tables, counts, sums, B, T, cap)
    counts, sums, warped = _moments_to_host(raw, flow, cap)        # raw ids are <= cap by construction
    if make_consistent:
        centres = _means(counts, sums)
        anchors = centres if short_interval else _means(counts, warped, MOMENT_SCALE)
        tables = np.concatenate([_consistent_tables(counts[b * T:(b + 1) * T], centres[b * T:(b + 1) * T], anchors[b * T:(b + 1) * T], thr)
                                 for b in range(B)])
        tracked = _relabel(raw, tables).view(B, T, H, W)
    else:
        tables = np.tile(np.arange(cap + 1, dtype=np.int64), (B * T, 1))
        tracked = raw.view(B, T, H, W)
    if not compute_matched_centers:
        return tracked
    return tracked, _tracks(tables, counts, sums, B, T, cap)


def _tracks(tables, counts, sums, B, T, cap):
    """{id: [n, 2] (x, y) centre track} of the instances of the first frame from the host copies of the tables [T, cap + 1] and
    the raw moments: moments of the consistent ids from those of the raw ids (integer sums: exact)."""
    assert B == 1
    top = int(tables.max())
    t_idx = np.repeat(np.arange(T), cap + 1)
    c_cnt = np.zeros((T, top + 1), dtype=np.int64)
    c_sum = np.zeros((T, top + 1, 2), dtype=np.int64)
    np.add.at(c_cnt, (t_idx, tables.ravel()), counts.ravel())
    np.add.at(c_sum, (t_idx, tables.ravel()), sums.reshape(-1, 2))
    centres = _means(c_cnt, c_sum)
    tracks = {}
    for ident in (np.flatnonzero(c_cnt[0][1:]) + 1).tolist():       # the instances of the first frame, wherever they reappear
        seen = c_cnt[:, ident] > 0
        tracks[ident] = centres[seen, ident][:, ::-1]               # (row, col) -> (x, y)
    return tracks


def predict_instance_segmentation_and_trajectories(output, compute_matched_centers=False, make_consistent=True, vehicles_id=1):
    """Decoder output dict (``segmentation`` [b, T, classes, H, W], ``instance_center`` [b, T, 1, H, W], ``instance_offset`` and
    ``instance_flow`` [b, T, 2, H, W]) -> [b, T, H, W] int64 instance ids (+ {id: [n, 2] (x, y) centre track} of the
    instances of the first frame when ``compute_matched_centers``, batch size 1)."""
    return _predict(output, compute_matched_centers, make_consistent, vehicles_id, short_interval=False)


def predict_instance_segmentation_and_trajectories_short_interval(output, compute_matched_centers=False, make_consistent=True,
                                                                  vehicles_id=1):
    """``predict_instance_segmentation_and_trajectories`` with the short-interval matcher (the streaming evaluator's
    post-processing): the flow is not used; a missing ``instance_flow`` is still replaced by zeros in the dict."""
    return _predict(output, compute_matched_centers, make_consistent, vehicles_id, short_interval=True)
