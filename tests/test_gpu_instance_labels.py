"""GPU: ground-truth centerness / offset / flow labels from instance maps (sf_instance_labels_fwd, streamingflow_amd.labels)
against the REFERENCE's convert_instance_mask_to_center_and_offset_label (tests/golden/instance_labels.npz,
tools/gen_instance_labels_golden.py).
  * offset and flow: equal on every pixel.  They are small integers or ignore_index, and the generator refused every scene whose
    labels move when the ego-motions are scaled by 1 +- 2e-7 (and 1 +- 1e-5), so none hangs on a nearest-neighbour rounding boundary;
  * centerness: within 2^-22 absolute.  The argument of exp is the reference's bit pattern (an exact integer squared distance, one
    fp32 division); the two expf implementations are each specified to 1 ulp, values lie in (0, 1] where an ulp is at most 2^-24,
    so two ulps with a 2x margin;
  * the warped half of the moments pass against sf_instance_moments_fwd on the sf_warp_affine_fwd(nearest) output: exactly;
  * batching, prepare_future_labels, the entry point's argument checks, run-to-run equality."""
import functools
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from util import ROOT, cases, gold

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_instance_labels_golden as GEN  # noqa: E402
from streamingflow_amd._lib import SF_ERR_INVALID, SF_ERR_WORKSPACE  # noqa: E402

pytestmark = pytest.mark.gpu
CENTER_TOL = 2.0 ** -22


@functools.lru_cache(maxsize=None)
def scene(tag):
    s = GEN.scene(tag)
    return s["instance"].cuda(), s["future_egomotion"].cuda(), s["num_instances"], s["kwargs"]


@functools.lru_cache(maxsize=None)
def labels_of(tag):
    from streamingflow_amd import labels as LB
    inst, ego, K, kw = scene(tag)
    return LB.convert_instance_mask_to_center_and_offset_label(inst, ego, K, **kw)


@pytest.mark.parametrize("tag", sorted(GEN.SCENES))
def test_labels_equal_the_reference(tag):
    G = gold("instance_labels.npz")
    inst, _, _, _ = scene(tag)
    T, H, W = inst.shape
    center, offset, flow = labels_of(tag)
    assert center.is_cuda and center.dtype == offset.dtype == flow.dtype == torch.float32
    assert tuple(center.shape) == (T, 1, H, W) and tuple(offset.shape) == tuple(flow.shape) == (T, 2, H, W)
    for name, got in (("offset", offset), ("flow", flow)):
        bad = int((got.cpu().numpy() != G[f"{tag}.{name}"]).sum())
        assert bad == 0, (name, bad)
    err = float(np.abs(center.cpu().numpy().astype(np.float64) - G[f"{tag}.centerness"].astype(np.float64)).max())
    print(f"{tag}: centerness max abs error {err:.3e} (bound {CENTER_TOL:.3e})")
    assert err <= CENTER_TOL, f"centerness max abs error {err:.3e} > {CENTER_TOL:.3e}"


def test_batched_call_equals_the_single_calls():
    from streamingflow_amd import labels as LB
    tags = ("a48", "c48")
    inst, ego, K, kw = GEN.stacked(tags)
    got = LB.instance_labels(inst.cuda(), ego.cuda(), K, **kw)
    assert tuple(got[0].shape) == (2, 6, 1, 48, 40) and tuple(got[1].shape) == tuple(got[2].shape) == (2, 6, 2, 48, 40)
    for b, tag in enumerate(tags):
        for name, one, many in zip(("centerness", "offset", "flow"), labels_of(tag), got):
            assert torch.equal(one, many[b]), (tag, name)


@pytest.mark.parametrize("tags", (("a48", "c48"), ("b96",), ("t1",)))
def test_moments_in_the_workspace_equal_the_warp_and_moments_kernels(tags):
    """Plain half: sf_instance_moments_fwd on the maps.  Warped half: the same on the sf_warp_affine_fwd(nearest) output of the maps
    under the sampling matrices the label call builds — the fused lookup has to pick the very pixel the warp kernel picks."""
    from streamingflow_amd import _lib, labels as LB, runtime
    from streamingflow_amd.models.lift_splat import pose_vec2mat
    from streamingflow_amd.runtime import ptr
    inst, ego, K, kw = GEN.stacked(tags)
    inst, ego = inst.cuda(), ego.cuda()
    B, T, H, W = inst.shape
    F = B * T
    cnt, sums, wcnt, wsums = LB.instance_labels(inst, ego, K, return_moments=True, **kw)[3]
    assert tuple(cnt.shape) == tuple(wcnt.shape) == (F, K + 1) and tuple(sums.shape) == tuple(wsums.shape) == (F, K + 1, 2)

    poses = torch.zeros((B, T, 6), device=inst.device)
    if T > 1:
        poses[:, 1:] = LB.mat2pose_vec(LB.invert_pose_matrix(pose_vec2mat(ego[:, :-1]).reshape(-1, 4, 4))).view(B, T - 1, 6)
    warped = LB.warp_features(inst.reshape(F, 1, H, W).float(), poses.view(F, 6), mode="nearest", spatial_extent=kw["spatial_extent"])
    assert torch.equal(warped[::T], inst.reshape(F, 1, H, W).float()[::T])       # frame 0 of a sequence: the identity
    if T > 1:
        assert not torch.equal(warped, inst.reshape(F, 1, H, W).float())

    def moments(maps):
        pos = torch.empty((F, K + 1, 2), dtype=torch.int64, device=maps.device)
        n = torch.empty((F, K + 1), dtype=torch.int32, device=maps.device)
        _lib.check(_lib.lib().sf_instance_moments_fwd(ptr(maps), None, F, H, W, K, ptr(pos), None, ptr(n), runtime.stream_ptr(maps.device)), "moments")
        return n, pos

    n, pos = moments(inst.reshape(F, H, W).contiguous())
    assert torch.equal(cnt, n) and torch.equal(sums, pos)
    n, pos = moments(warped.reshape(F, H, W).long().contiguous())
    assert torch.equal(wcnt, n) and torch.equal(wsums, pos)
    assert int(cnt.sum()) > 0 and int(wcnt.sum()) > 0
    assert not cnt[:, 0].any() and not wcnt[:, 0].any()


def test_prepare_future_labels_derives_missing_labels():
    from streamingflow_amd import labels as LB
    cfg = NS(LIFT=NS(GT_DEPTH=True, D_BOUND=[2.0, 50.0, 1.0]), SEMANTIC_SEG=NS(PEDESTRIAN=NS(ENABLED=False)),
             INSTANCE_SEG=NS(ENABLED=True), INSTANCE_FLOW=NS(ENABLED=True))
    extent = (50.0, 50.0)
    batch = {k: v.cuda() for k, v in cases.label_batch(0).items()}
    before = {k: v.clone() for k, v in batch.items()}
    G = gold("labels.npz")

    # an untouched batch: its own labels are used, exactly as before this path existed (the parent's outputs on this batch are
    # what tests/test_labels.py pins to labels.npz; here: the carried labels win over anything derived)
    carried = LB.prepare_future_labels(batch, cfg, 3, extent, 8)
    marked = dict(batch, centerness=batch["centerness"] * 2.0)
    assert torch.equal(LB.prepare_future_labels(marked, cfg, 3, extent, 8)["centerness"], carried["centerness"] * 2.0)
    assert carried["centerness"].shape == G["0.centerness"].shape
    assert all(torch.equal(batch[k], before[k]) for k in batch)

    own = LB.instance_labels(batch["instance"], batch["future_egomotion"], int(batch["instance"].max()), spatial_extent=extent)
    full = dict(batch, centerness=own[0], offset=own[1], flow=own[2])
    stripped = {k: v for k, v in batch.items() if k not in ("centerness", "offset", "flow")}
    want, got = LB.prepare_future_labels(full, cfg, 3, extent, 8), LB.prepare_future_labels(stripped, cfg, 3, extent, 8)
    assert sorted(want) == sorted(got) == sorted(carried)
    for k in want:
        assert torch.equal(want[k], got[k]), k
    assert "centerness" not in stripped                                            # the caller's dict is left alone
    assert not torch.equal(got["centerness"], carried["centerness"])               # label_batch's own maps are decoder-like fakes
    # one missing key only: that one is derived, the carried ones stay
    partial = {k: v for k, v in batch.items() if k != "flow"}
    mixed = LB.prepare_future_labels(partial, cfg, 3, extent, 8)
    assert torch.equal(mixed["flow"], got["flow"]) and torch.equal(mixed["centerness"], carried["centerness"])


def test_untouched_batch_is_bitwise_what_the_parent_path_gives():
    """prepare_future_labels on a batch that carries its labels never reaches the label kernels: the result is the plain warp of the
    carried maps (the code path before this feature), bit for bit."""
    from streamingflow_amd import labels as LB
    cfg = NS(LIFT=NS(GT_DEPTH=False, D_BOUND=[2.0, 50.0, 1.0]), SEMANTIC_SEG=NS(PEDESTRIAN=NS(ENABLED=False)),
             INSTANCE_SEG=NS(ENABLED=True), INSTANCE_FLOW=NS(ENABLED=True))
    extent, rf = (50.0, 50.0), 3
    batch = {k: v.cuda() for k, v in cases.label_batch(1).items()}
    lab = LB.prepare_future_labels(batch, cfg, rf, extent, 8)
    ego = batch["future_egomotion"]
    for k in ("centerness", "offset", "flow"):
        past = LB.cumulative_warp_features(batch[k][:, :rf], ego[:, :rf], mode="nearest", spatial_extent=extent)[:, :-1]
        future = LB.cumulative_warp_features_reverse(batch[k][:, rf - 1:], ego[:, rf - 1:], mode="nearest", spatial_extent=extent)
        assert torch.equal(lab[k], torch.cat([past, future], dim=1)), k


def test_entry_point_rejects_bad_arguments():
    from streamingflow_amd import _lib, runtime
    from streamingflow_amd.runtime import ptr
    L = _lib.lib()
    B, T, H, W, K = 2, 3, 6, 5, 4
    dev = torch.device("cuda", 0)
    inst = torch.randint(0, K + 2, (B * T, H, W), device=dev)
    theta = torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], device=dev).repeat(B * T, 1).contiguous()
    center = torch.empty((B * T, 1, H, W), device=dev)
    offset, flow = torch.empty((B * T, 2, H, W), device=dev), torch.empty((B * T, 2, H, W), device=dev)
    need = L.sf_instance_labels_ws_bytes(B, T, H, W, K)
    assert need >= 2 * B * T * (K + 1) * (4 + 16) and need % 256 == 0
    ws = torch.empty(need // 4 + 64, dtype=torch.float32, device=dev)
    st = runtime.stream_ptr(dev)
    args = [ptr(inst), ptr(theta), B, T, H, W, K, 3.0, 255.0, ptr(center), ptr(offset), ptr(flow), ptr(ws), ws.numel() * 4, st]
    assert L.sf_instance_labels_fwd(*args) == 0
    bad = list(args)
    bad[13] = need                                                  # exactly the size asked for is enough
    assert L.sf_instance_labels_fwd(*bad) == 0
    for k in (0, 1, 9, 10, 11, 12):                                 # NULL pointers
        bad = list(args)
        bad[k] = None
        assert L.sf_instance_labels_fwd(*bad) == SF_ERR_INVALID, k
    for k in (2, 3, 4, 5):                                          # B, T, H, W < 1
        bad = list(args)
        bad[k] = 0
        assert L.sf_instance_labels_fwd(*bad) == SF_ERR_INVALID, k
        sizes = [B, T, H, W, K]
        sizes[k - 2] = 0
        assert L.sf_instance_labels_ws_bytes(*sizes) == 0
    bad = list(args)
    bad[6] = -1                                                     # num_instances < 0 (0 is a valid call)
    assert L.sf_instance_labels_fwd(*bad) == SF_ERR_INVALID and L.sf_instance_labels_ws_bytes(B, T, H, W, -1) == 0
    assert L.sf_instance_labels_ws_bytes(B, T, H, W, 0) > 0
    bad = list(args)
    bad[7] = 0.0                                                    # sigma
    assert L.sf_instance_labels_fwd(*bad) == SF_ERR_INVALID
    bad = list(args)
    bad[2], bad[3], bad[4], bad[5] = 1 << 6, 1 << 5, 1 << 10, 1 << 10      # B * T * H * W = 2^31
    assert L.sf_instance_labels_fwd(*bad) == SF_ERR_INVALID
    assert L.sf_instance_labels_ws_bytes(1 << 6, 1 << 5, 1 << 10, 1 << 10, K) == 0
    bad = list(args)
    bad[13] = need - 256                                            # short workspace
    assert L.sf_instance_labels_fwd(*bad) == SF_ERR_WORKSPACE
    torch.cuda.synchronize()


def test_python_argument_checks():
    from streamingflow_amd import labels as LB
    inst, ego, K, kw = scene("t1")
    with pytest.raises(NotImplementedError):
        LB.convert_instance_mask_to_center_and_offset_label(inst, ego, K, subtract_egomotion=False, **kw)
    with pytest.raises(NotImplementedError):
        LB.instance_labels(inst[None], ego[None], K, subtract_egomotion=False, **kw)
    with pytest.raises(RuntimeError):
        LB.convert_instance_mask_to_center_and_offset_label(inst.cpu(), ego.cpu(), K, **kw)
    with pytest.raises(ValueError):
        LB.convert_instance_mask_to_center_and_offset_label(inst, ego, K)
    with pytest.raises(AssertionError):
        LB.instance_labels(inst, ego, K, **kw)


def test_two_runs_are_bitwise_equal_and_other_arguments_reach_the_kernel():
    from streamingflow_amd import labels as LB
    inst, ego, K, kw = scene("c48")
    again = LB.convert_instance_mask_to_center_and_offset_label(inst, ego, K, **kw)
    for a, b in zip(labels_of("c48"), again):
        assert torch.equal(a, b)
    # ignore_index and sigma: the same labels with another fill value, exp(-d^2 / 4) on the same distances
    c2, o2, f2 = LB.convert_instance_mask_to_center_and_offset_label(inst, ego, K, ignore_index=-7, sigma=2.0, spatial_extent=kw["spatial_extent"])
    c, o, f = labels_of("c48")
    assert torch.equal(o2 == -7, o == 255) and torch.equal(f2 == -7, f == 255)
    assert torch.equal(o2[o != 255], o[o != 255]) and torch.equal(f2[f != 255], f[f != 255])
    d2 = torch.round(-9.0 * torch.log(c.double()))                  # integer squared distances back from sigma = 3
    assert float((c2.double() - torch.exp(-d2 / 4.0)).abs().max()) <= CENTER_TOL
