"""GPU: the sequence path of the instance post-processing (sf_instance_seq_fwd, streamingflow_amd.instance) and the
short-interval tracking of the streaming evaluator.
  * instance_segmentation_sequence against the per-frame functions (find_instance_centers / get_instance_segmentation_and_centers,
    themselves pinned to the reference by test_eval_harness.py): ids and centre lists, exactly;
  * predict_instance_segmentation_and_trajectories(_short_interval) against the REFERENCE's results
    (tests/golden/instance_short_interval.npz, tools/gen_instance_seq_golden.py), exactly;
  * the entry point's argument checks.
Integer / index work: everything must match exactly (the tracks, float means, to 1e-4)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from util import ROOT, gold

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_instance_seq_golden as GEN  # noqa: E402
from streamingflow_amd._lib import SF_ERR_INVALID, SF_ERR_WORKSPACE  # noqa: E402

pytestmark = pytest.mark.gpu
THR = 0.1


def per_frame(center, offset, fg, cap):
    """The single-frame functions, frame by frame: ([F, H, W] ids, list of [n, 2] centres)."""
    from streamingflow_amd import instance as I
    ids, cents = [], []
    for f in range(center.shape[0]):
        i, c = I.get_instance_segmentation_and_centers(center[f], offset[f], fg[f], conf_threshold=THR, max_n_instance_centers=cap)
        ids.append(i[0])
        cents.append(c.long())
    return torch.stack(ids), cents


def check_sequence(center, offset, fg, cap):
    from streamingflow_amd import instance as I
    want_ids, want_c = per_frame(center, offset, fg, cap)
    ids, cents = I.instance_segmentation_sequence(center, offset, fg, conf_threshold=THR, max_n_instance_centers=cap, return_centers=True)
    assert ids.dtype == torch.int64 and ids.shape == want_ids.shape
    assert len(cents) == len(want_c)
    for f, (a, b) in enumerate(zip(cents, want_c)):
        assert a.dtype == torch.int64 and a.shape == b.shape and torch.equal(a, b), f
    bad = (ids != want_ids).flatten(1).any(1).nonzero().flatten().tolist()
    assert not bad, bad
    assert int(ids.max()) <= cap
    assert torch.equal(I.instance_segmentation_sequence(center, offset, fg, conf_threshold=THR, max_n_instance_centers=cap), ids)
    return ids, cents


def edge_frames():
    """9 frames of 24 x 20: random maps, zeros, corner peaks, last pixel then first pixel, a plateau, a value at the threshold."""
    g = torch.Generator().manual_seed(11)
    F, H, W = 9, 24, 20
    heat = torch.zeros(F, 1, H, W)
    heat[0, 0] = torch.rand(H, W, generator=g)
    heat[1, 0] = torch.rand(H, W, generator=g) * 0.3              # many values under the threshold
    # frame 2: zeros
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        heat[3, 0, y, x] = 0.9
    heat[4, 0, H - 1, W - 1] = 0.8                                 # the last pixel of a frame ...
    heat[5, 0, 0, 0] = 0.8                                         # ... next to the first pixel of the following one
    heat[6, 0, 10:12, 7:10] = 0.7                                  # a plateau: every pixel of it equals its 3x3 maximum
    heat[6, 0, 3, 3] = 0.5
    heat[7, 0, 5, 5] = torch.tensor(THR, dtype=torch.float32)      # exactly the threshold: not above it
    heat[7, 0, 15, 12] = 0.4
    heat[8, 0] = torch.rand(H, W, generator=g)
    offset = (torch.rand(F, 2, H, W, generator=g) - 0.5) * 10.0
    fg = torch.rand(F, H, W, generator=g) > 0.3
    fg[8] = True                                                   # a frame without background pixels
    return heat.cuda(), offset.cuda(), fg.cuda()


def test_sequence_equals_per_frame_on_edge_frames():
    heat, offset, fg = edge_frames()
    ids, cents = check_sequence(heat, offset, fg, 100)
    n = [len(c) for c in cents]
    assert n[2] == 0 and int(ids[2].max()) == 0                    # no centre: all zeros
    assert cents[3].tolist() == [[0, 0], [0, 19], [23, 0], [23, 19]]
    assert cents[4].tolist() == [[23, 19]] and cents[5].tolist() == [[0, 0]]
    assert n[6] == 7 and cents[7].tolist() == [[15, 12]]
    assert n[0] > 5 and n[1] > 5 and n[8] > 5
    assert int(ids[8].max()) == n[8] - 1                           # no background pixel: the first instance became 0


def test_sequence_equals_per_frame_when_frames_overflow_the_cap():
    heat, offset, fg = edge_frames()
    ids, cents = check_sequence(heat, offset, fg, 5)
    assert [len(c) for c in cents] == [5, 5, 0, 4, 1, 1, 5, 1, 5]


def test_sequence_keeps_the_first_hundred_of_188_centres():
    g = torch.Generator().manual_seed(7)
    heat = torch.rand((2, 1, 40, 40), generator=g)
    offset = (torch.rand((2, 2, 40, 40), generator=g) - 0.5) * 8.0
    fg = torch.ones((2, 40, 40), dtype=torch.bool)
    from streamingflow_amd import instance as I
    for f in range(2):
        assert I.find_instance_centers(heat[f].cuda(), conf_threshold=THR).shape[0] == 188
    ids, cents = check_sequence(heat.cuda(), offset.cuda(), fg.cuda(), 100)
    for f in range(2):
        assert cents[f].shape[0] == 100
        assert torch.unique(ids[f]).tolist() == list(range(100))   # no background pixel: the first instance becomes 0


def test_sequence_walks_more_centres_than_one_table_piece():
    """Cap 150 on the 188-centre frames: the grouping kernel takes its centre table in pieces of 128, here two of them; a
    second frame pair with cap 300 keeps all 188 (a full piece and a partial one, nothing cut)."""
    g = torch.Generator().manual_seed(7)
    heat = torch.rand((2, 1, 40, 40), generator=g)
    offset = (torch.rand((2, 2, 40, 40), generator=g) - 0.5) * 8.0
    fg = torch.rand((2, 40, 40), generator=g) > 0.1
    ids, cents = check_sequence(heat.cuda(), offset.cuda(), fg.cuda(), 150)
    assert [len(c) for c in cents] == [150, 150] and int(ids.max()) > 128
    ids, cents = check_sequence(heat.cuda(), offset.cuda(), fg.cuda(), 300)
    assert [len(c) for c in cents] == [188, 188] and int(ids.max()) > 150


def test_sequence_single_small_frame():
    g = torch.Generator().manual_seed(3)
    heat = torch.rand((1, 5, 7), generator=g)
    offset = (torch.rand((1, 2, 5, 7), generator=g) - 0.5) * 4.0
    fg = torch.rand((1, 5, 7), generator=g) > 0.2
    ids, cents = check_sequence(heat.cuda(), offset.cuda(), fg.cuda(), 100)
    assert len(cents[0]) >= 1


@functools.lru_cache(maxsize=None)
def scene(tag):
    return {k: v.cuda() for k, v in GEN.scene_output(tag).items()}


def fresh(tag, **replace):
    d = dict(scene(tag))
    d.update(replace)
    return d


@pytest.mark.parametrize("tag", sorted(GEN.SCENES))
def test_short_interval_equals_the_reference(tag):
    from streamingflow_amd.instance import predict_instance_segmentation_and_trajectories_short_interval as predict
    G = gold("instance_short_interval.npz")
    want = G[f"{tag}.short"].astype(np.int64)
    got = predict(fresh(tag))
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    o = fresh(tag)
    zero_flow = predict(fresh(tag, instance_flow=torch.zeros_like(o["instance_flow"])))
    assert torch.equal(zero_flow, got)
    o = fresh(tag, instance_flow=None)
    assert torch.equal(predict(o), got)
    assert o["instance_flow"].shape == o["instance_offset"].shape and not o["instance_flow"].any()
    raw = predict(fresh(tag), make_consistent=False)
    assert np.array_equal(raw.cpu().numpy(), G[f"{tag}.raw"].astype(np.int64))


@pytest.mark.parametrize("kind", ("short", "regular"))
def test_tracks_equal_the_reference(kind):
    from streamingflow_amd import instance as I
    predict = I.predict_instance_segmentation_and_trajectories_short_interval if kind == "short" else I.predict_instance_segmentation_and_trajectories
    G = gold("instance_short_interval.npz")
    tag = GEN.TRACK_SCENE
    got, tracks = predict(fresh(tag), compute_matched_centers=True)
    assert np.array_equal(got.cpu().numpy(), G[f"{tag}.{kind}"].astype(np.int64))
    names = [n for n in G.files if n.startswith(f"{tag}.track_{kind}.")]
    assert sorted(tracks) == sorted(int(n.rsplit(".", 1)[1]) for n in names) and len(names) == 5
    for n in names:
        mine = tracks[int(n.rsplit(".", 1)[1])]
        assert mine.shape == G[n].shape and np.allclose(mine, G[n], atol=1e-4), n


@pytest.mark.parametrize("tag", sorted(GEN.SCENES))
def test_regular_equals_the_reference_and_batches_like_single_samples(tag):
    from streamingflow_amd.instance import predict_instance_segmentation_and_trajectories as predict
    G = gold("instance_short_interval.npz")
    got = predict(fresh(tag))
    assert np.array_equal(got.cpu().numpy(), G[f"{tag}.regular"].astype(np.int64))
    if got.shape[0] > 1:
        for b in range(got.shape[0]):
            one = predict({k: v[b:b + 1] for k, v in scene(tag).items()})
            assert torch.equal(one[0], got[b]), b


def test_short_interval_matcher_on_given_maps():
    from streamingflow_amd import instance as I
    G = gold("instance_short_interval.npz")
    raw = torch.from_numpy(G["s3k6.raw"].astype(np.int64)).cuda()
    for b in range(raw.shape[0]):
        got = I.make_instance_id_temporally_consistent_short_interval(raw[b:b + 1], scene("s3k6")["instance_flow"][b:b + 1])
        assert np.array_equal(got[0].cpu().numpy(), G["s3k6.short"][b].astype(np.int64))
        assert torch.equal(I.make_instance_id_temporally_consistent_short_interval(raw[b:b + 1]), got)


def test_entry_point_rejects_bad_arguments():
    from streamingflow_amd import _lib, runtime
    from streamingflow_amd.runtime import ptr
    L = _lib.lib()
    F, H, W, cap = 2, 6, 5, 4
    dev = torch.device("cuda", 0)
    heat = torch.rand((F, H, W), device=dev)
    off = torch.zeros((F, 2, H, W), device=dev)
    fg = torch.ones((F, H, W), dtype=torch.uint8, device=dev)
    cents = torch.empty((F, cap, 2), dtype=torch.int32, device=dev)
    n = torch.empty((F,), dtype=torch.int32, device=dev)
    ids = torch.empty((F, H, W), dtype=torch.int64, device=dev)
    need = L.sf_instance_seq_ws_bytes(F, H, W, cap)
    assert need > 2 * F * H * W * 4
    ws = torch.empty(need // 4 + 64, dtype=torch.float32, device=dev)
    st = runtime.stream_ptr(dev)
    args = [ptr(heat), ptr(off), ptr(fg), F, H, W, THR, cap, ptr(cents), ptr(n), ptr(ids), ptr(ws), ws.numel() * 4, st]
    assert L.sf_instance_seq_fwd(*args) == 0
    for k in (0, 1, 2, 8, 9, 10, 11):                               # NULL pointers
        bad = list(args)
        bad[k] = None
        assert L.sf_instance_seq_fwd(*bad) == SF_ERR_INVALID, k
    for k in (3, 4, 5, 7):                                          # F, H, W, cap < 1
        bad = list(args)
        bad[k] = 0
        assert L.sf_instance_seq_fwd(*bad) == SF_ERR_INVALID, k
        size_args = [F, H, W, cap]
        size_args[{3: 0, 4: 1, 5: 2, 7: 3}[k]] = 0
        assert L.sf_instance_seq_ws_bytes(*size_args) == 0
    bad = list(args)
    bad[3], bad[4], bad[5] = 1 << 11, 1 << 10, 1 << 10              # F * H * W = 2^31
    assert L.sf_instance_seq_fwd(*bad) == SF_ERR_INVALID
    assert L.sf_instance_seq_ws_bytes(1 << 11, 1 << 10, 1 << 10, cap) == 0
    bad = list(args)
    bad[12] = need - 512                                            # short workspace
    assert L.sf_instance_seq_fwd(*bad) == SF_ERR_WORKSPACE
    torch.cuda.synchronize()


def test_cpu_tensors_and_other_nms_sizes_raise():
    from streamingflow_amd import instance as I
    heat, off, fg = torch.rand(1, 5, 7), torch.zeros(1, 2, 5, 7), torch.ones(1, 5, 7, dtype=torch.bool)
    with pytest.raises(RuntimeError):
        I.instance_segmentation_sequence(heat, off, fg)
    with pytest.raises(NotImplementedError):
        I.instance_segmentation_sequence(heat.cuda(), off.cuda(), fg.cuda(), nms_kernel_size=5)
    with pytest.raises(RuntimeError):
        I.predict_instance_segmentation_and_trajectories_short_interval(GEN.scene_output("s0k1"))
    with pytest.raises(RuntimeError):
        I.make_instance_id_temporally_consistent_short_interval(torch.zeros(1, 2, 5, 7, dtype=torch.long))


def test_two_runs_are_bitwise_equal():
    from streamingflow_amd import instance as I
    heat, offset, fg = edge_frames()
    a = I.instance_segmentation_sequence(heat, offset, fg, conf_threshold=THR, max_n_instance_centers=5, return_centers=True)
    b = I.instance_segmentation_sequence(heat, offset, fg, conf_threshold=THR, max_n_instance_centers=5, return_centers=True)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    p = I.predict_instance_segmentation_and_trajectories_short_interval(fresh("s3k6"))
    q = I.predict_instance_segmentation_and_trajectories_short_interval(fresh("s3k6"))
    assert torch.equal(p, q)
