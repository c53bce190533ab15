"""GPU: instance tracking on the device (sf_instance_track_fwd, csrc/instance_track.hip) and the public functions on top of it.
  * direct calls on the synthetic moment tables of tests/track_util.py against streamingflow_amd.instance._consistent_tables: whole
    tables, exactly (integer ids: no tolerance), both matchers, thresholds 3 and 10;
  * the entry point's argument checks and the flag of a sample with a missing raw id;
  * a cost matrix with two optimal assignments: one of them, the same on every run;
  * predict_* and make_instance_id_temporally_consistent*: the default (device) path against SF_TRACK_HOST=1, exactly;
  * predict_instance_segmentation_and_trajectories inside a captured graph (it may not wait on the host)."""
import functools

import numpy as np
import pytest
import torch

import track_util as TU
from streamingflow_amd._lib import SF_OK, SF_ERR_INVALID, SF_ERR_WORKSPACE

pytestmark = pytest.mark.gpu
POISON = -7


def track(case, threshold, K=None, B=None, T=None, ws_bytes=None, null=None):
    """sf_instance_track_fwd on a case -> (status, tables [B*T, K] numpy, flags [B] numpy); outputs start poisoned."""
    from streamingflow_amd import _lib, runtime
    from streamingflow_amd.runtime import ptr
    L = _lib.lib()
    B, T, K = B or case.B, T or case.T, K or case.K
    arg = {"counts": torch.from_numpy(case.counts).cuda(), "sums": torch.from_numpy(case.sums).cuda(),
           "warped": torch.from_numpy(case.warped).cuda() if case.warped is not None else None,
           "tables": torch.full((case.B * case.T, case.K), POISON, dtype=torch.int64, device="cuda"),
           "flags": torch.full((case.B,), POISON, dtype=torch.int32, device="cuda")}
    need = L.sf_instance_track_ws_bytes(case.B, case.T, case.K)
    assert need > 0
    arg["ws"] = torch.empty((need + 3) // 4, dtype=torch.int32, device="cuda")
    if null:
        arg[null] = None
    status = L.sf_instance_track_fwd(ptr(arg["counts"]), ptr(arg["sums"]), ptr(arg["warped"]), B, T, K, float(threshold), ptr(arg["tables"]),
                                     ptr(arg["flags"]), ptr(arg["ws"]), need if ws_bytes is None else ws_bytes,
                                     runtime.stream_ptr(torch.device("cuda")))
    torch.cuda.synchronize()
    return status, None if null == "tables" else arg["tables"].cpu().numpy(), None if null == "flags" else arg["flags"].cpu().numpy()


@pytest.mark.parametrize("threshold", TU.THRESHOLDS)
@pytest.mark.parametrize("warped", (False, True), ids=("plain", "warped"))
@pytest.mark.parametrize("name", sorted(TU.SPECS))
def test_tables_equal_the_host_statement(name, warped, threshold):
    case = TU.case(name, warped)
    status, tables, flags = track(case, threshold)
    assert status == SF_OK and not flags.any()
    want = TU.expected(name, warped, threshold)
    assert tables.dtype == np.int64 and tables.shape == want.shape
    bad = np.flatnonzero((tables != want).any(axis=1)).tolist()
    assert not bad, (bad, tables[bad[0]], want[bad[0]])


def test_single_frame_and_no_instances():
    one = TU.make_case([[6]], False, seed=3)
    status, tables, flags = track(one, 3.0)
    assert status == SF_OK and not flags.any() and np.array_equal(tables, np.arange(one.K)[None])
    none = TU.Case(np.zeros((3, 4), dtype=np.int32), np.zeros((3, 4, 2), dtype=np.int64), None, 1, 3)
    status, tables, flags = track(none, 3.0)
    assert status == SF_OK and not flags.any() and np.array_equal(tables, np.tile(np.arange(4), (3, 1)))
    bare = TU.Case(np.full((2, 1), 5, dtype=np.int32), np.zeros((2, 1, 2), dtype=np.int64), None, 1, 2)      # K = 1: background only
    status, tables, flags = track(bare, 3.0)
    assert status == SF_OK and not flags.any() and not tables.any()


def test_argument_checks():
    from streamingflow_amd import _lib
    L = _lib.lib()
    case = TU.case("5x1", True)
    assert L.sf_instance_track_ws_bytes(1, 2, 130) == 0 and L.sf_instance_track_ws_bytes(1, 2, 129) > 0
    assert L.sf_instance_track_ws_bytes(0, 2, 6) == 0 and L.sf_instance_track_ws_bytes(1, 0, 6) == 0 and L.sf_instance_track_ws_bytes(1, 2, 0) == 0
    assert track(case, 3.0, K=130)[0] == SF_ERR_INVALID      # K - 1 = 129 instances
    for kw in ({"B": -1}, {"T": -1}, {"K": -1}, {"null": "counts"}, {"null": "sums"}, {"null": "tables"}, {"null": "flags"}, {"null": "ws"}):
        assert track(case, 3.0, **kw)[0] == SF_ERR_INVALID, kw
    need = L.sf_instance_track_ws_bytes(case.B, case.T, case.K)
    status, tables, flags = track(case, 3.0, ws_bytes=need - 1)
    assert status == SF_ERR_WORKSPACE and (tables == POISON).all() and (flags == POISON).all()      # nothing was launched
    assert track(case, 3.0, ws_bytes=need)[0] == SF_OK


def test_a_missing_raw_id_sets_the_flag_of_its_sample_only():
    good = TU.case("B3_mixed", True)
    counts = good.counts.copy()
    T, K = good.T, good.K
    assert counts[T + 3, 1:7].all() and counts[T + 2, 1:5].all()      # sample 1: 4 instances, then 6
    counts[T + 3, 3] = 0                                              # ... of which id 3 goes missing
    status, tables, flags = track(TU.Case(counts, good.sums, good.warped, good.B, T), 3.0)
    assert status == SF_OK and flags.tolist() == [0, 1, 0]
    want = TU.expected("B3_mixed", True, 3.0)
    for b in (0, 2):
        assert np.array_equal(tables[b * T:(b + 1) * T], want[b * T:(b + 1) * T]), b
    assert np.array_equal(tables[T:T + 3], want[T:T + 3])             # the frames before the broken pair
    assert tables[T:2 * T].min() >= 0 and tables[T:2 * T].max() <= T * K


def test_one_of_two_optima_the_same_on_every_run():
    from scipy.optimize import linear_sum_assignment
    case = TU.two_optima_case()
    gap = TU.pair_costs(case)[0][2]
    rows, cols = linear_sum_assignment(gap)
    runs = [track(case, 10.0) for _ in range(2)]
    for status, tables, flags in runs:
        assert status == SF_OK and not flags.any()
        assert tables[0].tolist() == [0, 1, 2, 3, 4]
        partner = tables[1, 1:]                                       # every distance is under 10: all four inherit an id of frame 0
        assert sorted(partner.tolist()) == [1, 2, 3, 4]
        assert float(gap[partner - 1, np.arange(4)].astype(np.float64).sum()) == float(gap[rows, cols].astype(np.float64).sum()) == 16.0
    assert np.array_equal(runs[0][1], runs[1][1])


# ---- the public functions ------------------------------------------------------------------------------------------------------

def scene(frames, seed, h=64, w=64, n_obj=8, blank=()):
    """A decoder output of one sample in the style of tools/instbench.py's scene: moving 9 x 5 boxes with Gaussian centre heat, offsets
    pointing at the centres and a constant flow per object; the boxes start in cells of a 3 x 3 grid, so they stay apart.  Frames in
    `blank` hold no vehicle pixel."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float), torch.arange(w, dtype=torch.float), indexing="ij")
    seg, center = torch.zeros(1, frames, 2, h, w), torch.zeros(1, frames, 1, h, w)
    offset, flow = torch.zeros(1, frames, 2, h, w), torch.zeros(1, frames, 2, h, w)
    cells = torch.randperm(9, generator=g)[:n_obj]
    pos = torch.stack([(cells // 3) * 20.0 + 12.0, (cells % 3) * 20.0 + 12.0], 1) + (torch.rand(n_obj, 2, generator=g) - 0.5) * 5.0
    vel = (torch.rand(n_obj, 2, generator=g) - 0.5) * 1.6
    for t in range(frames):
        fg = torch.zeros(h, w, dtype=torch.bool)
        for k in range(n_obj if t not in blank else 0):
            cy, cx = pos[k] + vel[k] * t
            m = ((yy - cy).abs() <= 4.5) & ((xx - cx).abs() <= 2.5)
            fg |= m
            center[0, t, 0] = torch.maximum(center[0, t, 0], torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 12.0))
            offset[0, t, 0][m] = (cy.round() - yy)[m]
            offset[0, t, 1][m] = (cx.round() - xx)[m]
            flow[0, t, 0][m] = vel[k, 0]
            flow[0, t, 1][m] = vel[k, 1]
        seg[0, t, 1][fg] = 4.0
        seg[0, t, 0][~fg] = 4.0
    return {"segmentation": seg, "instance_center": center, "instance_offset": offset, "instance_flow": flow}


@functools.lru_cache(maxsize=None)
def batch(first_seed=21):
    """B = 3, T = 5; sample 1 has a blanked frame 2."""
    parts = [scene(5, first_seed + b, blank=(2,) if b == 1 else ()) for b in range(3)]
    return {k: torch.cat([p[k] for p in parts]).cuda() for k in parts[0]}


PREDICT = ("predict_instance_segmentation_and_trajectories", "predict_instance_segmentation_and_trajectories_short_interval")


@pytest.mark.parametrize("fn", PREDICT)
def test_predict_device_path_equals_host_path(fn, monkeypatch):
    from streamingflow_amd import instance as I
    out = dict(batch())
    monkeypatch.delenv("SF_TRACK_HOST", raising=False)
    got = getattr(I, fn)(out)
    monkeypatch.setenv("SF_TRACK_HOST", "1")
    want = getattr(I, fn)(out)
    assert got.dtype == torch.int64 and got.shape == (3, 5, 64, 64) and torch.equal(got, want)
    assert int(want[:, 0].max()) >= 6 and int(want[1, 2].max()) == 0 and int(want[1, 3].max()) >= 6
    one = {k: v[:1] for k, v in out.items()}
    host_ids, host_tracks = getattr(I, fn)(one, compute_matched_centers=True)
    monkeypatch.delenv("SF_TRACK_HOST")
    ids, tracks = getattr(I, fn)(one, compute_matched_centers=True)
    assert torch.equal(ids, host_ids) and torch.equal(ids, got[:1])
    assert sorted(tracks) == sorted(host_tracks) == list(range(1, int(ids[0, 0].max()) + 1))
    for k in tracks:
        assert tracks[k].shape == host_tracks[k].shape and np.array_equal(tracks[k], host_tracks[k]), k
    assert max(len(v) for v in tracks.values()) == 5


def id_maps(seed=4, T=4, h=24, w=24, n=6, scale=1):
    """[1, T, h, w] maps of n 3 x 3 blocks drifting one pixel per frame, ids scale * (1..n); flow pointing along the drift."""
    g = torch.Generator().manual_seed(seed)
    maps, flow = torch.zeros(1, T, h, w, dtype=torch.int64), torch.zeros(1, T, 2, h, w)
    for k in range(n):
        y, x = 3 + 6 * (k // 3) + int(torch.randint(0, 2, (1,), generator=g)), 2 + 7 * (k % 3)
        for t in range(T):
            ident = scale * (1 + (k + t) % n)                         # the raw ids rotate from frame to frame
            maps[0, t, y + t:y + t + 3, x:x + 3] = ident
            flow[0, t, 0, y + t:y + t + 3, x:x + 3] = 1.0
    return maps.cuda(), flow.cuda()


def test_stand_alone_functions_device_path_equals_host_path(monkeypatch):
    from streamingflow_amd import instance as I
    for scale in (1, 40):      # ids 1..6 on the device; 40..240 are past MAX_TRACK_ID: the host path either way
        maps, flow = id_maps(scale=scale)
        monkeypatch.delenv("SF_TRACK_HOST", raising=False)
        if scale == 1:
            a, s = I.make_instance_id_temporally_consistent(maps, flow), I.make_instance_id_temporally_consistent_short_interval(maps)
            monkeypatch.setenv("SF_TRACK_HOST", "1")
            assert torch.equal(a, I.make_instance_id_temporally_consistent(maps, flow))
            assert torch.equal(s, I.make_instance_id_temporally_consistent_short_interval(maps))
            for t in range(maps.shape[1]):                            # every block keeps the id it had in frame 0
                assert torch.equal((a[0, t] == 1).nonzero()[0], (maps[0, 0] == 1).nonzero()[0] + torch.tensor([t, 0], device="cuda"))
        else:
            with pytest.raises(ValueError):                           # ids 40, 80, ...: 1..39 are missing, scipy refuses the NaN centres
                I.make_instance_id_temporally_consistent(maps, flow)
    maps, flow = id_maps()
    maps[0, 2][maps[0, 2] == 3] = 0                                   # frame 2 loses raw id 3
    for host in ("0", "1"):
        monkeypatch.setenv("SF_TRACK_HOST", host)
        with pytest.raises(ValueError):
            I.make_instance_id_temporally_consistent(maps, flow)
        with pytest.raises(ValueError):
            I.make_instance_id_temporally_consistent_short_interval(maps)


def test_predict_is_captured_in_a_graph(monkeypatch):
    """No host round trip: the whole post-processing of a batch is recorded once and replayed on another scene."""
    from streamingflow_amd import instance as I
    monkeypatch.delenv("SF_TRACK_HOST", raising=False)
    first = batch()
    second = {k: torch.cat([scene(5, 31 + b, blank=(1,) if b == 2 else ())[k] for b in range(3)]).cuda() for k in first}
    static = {k: v.clone() for k, v in first.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        I.predict_instance_segmentation_and_trajectories(static)      # warm-up: workspaces, kernel attributes
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        result = I.predict_instance_segmentation_and_trajectories(static)
    for k in static:
        static[k].copy_(second[k])
    graph.replay()
    torch.cuda.synchronize()
    want = I.predict_instance_segmentation_and_trajectories(second)
    assert torch.equal(result, want)
    assert not torch.equal(want, I.predict_instance_segmentation_and_trajectories(first))
    assert int(want[2, 1].max()) == 0 and int(want[:, 0].max()) >= 6
