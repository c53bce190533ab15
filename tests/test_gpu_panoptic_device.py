"""GPU: PanopticMetric with ``max_instances`` — scoring on the device (sf_panoptic_score_fwd, csrc/panoptic_score.hip), no host copy.
  * the fixture scenes of tests/golden/panoptic_device.npz (the REFERENCE's own counters, tools/gen_panoptic_golden.py): the three
    integer counters exactly, ``iou`` within n * 2^-24 * sum (the textbook bound of the reference's sequential fp32 sum of n terms
    against an exact one; the device path adds one rounding per update, which the bound covers from n = 2 on, and n = 1 is exact
    on both sides), pq / sq / rq within 1e-5 (what tests/test_eval_harness.py asks of the host path);
  * bit equality with the host path (``max_instances=None``) of the same class, at several M, input dtypes and sizes past one pass of
    the tally workgroup;
  * the scenes of tests/golden/eval.npz behind predict_instance_segmentation_and_trajectories;
  * ``vehicles_id=2``: tracking off;
  * wrong labels: flagged on the device, the update adds nothing, ``compute()`` raises, ``reset()`` clears;
  * a whole evaluation step inside a captured graph (a synchronising call there is an error);
  * the entry point's argument checks."""
import numpy as np
import pytest
import torch

import panoptic_util as PU
from util import cases, gold
from streamingflow_amd._lib import SF_OK, SF_ERR_INVALID, SF_ERR_WORKSPACE

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def device_metric(M, **kw):
    from streamingflow_amd.metrics import PanopticMetric
    return PanopticMetric(2, max_instances=M, **kw)


def host_metric(**kw):
    from streamingflow_amd.metrics import PanopticMetric
    return PanopticMetric(2, **kw)


def maps(pair, dtype=torch.int64):
    return tuple(torch.from_numpy(a.astype(np.int64)).to(dtype).cuda() for a in pair)


def counters(m):
    return {k: getattr(m, k).clone() for k in PU.COUNTERS}


def assert_bitwise(a, b):
    for k in PU.COUNTERS:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype == torch.float32 and torch.equal(x, y), (k, x.tolist(), y.tolist())


def assert_reference(m, ref):
    """The metric's counters against one row of the fixture."""
    for k in ("true_positive", "false_positive", "false_negative"):
        assert np.array_equal(getattr(m, k).cpu().numpy(), ref[k]), (k, getattr(m, k).tolist(), ref[k].tolist())
    got, tp = m.iou.cpu().numpy().astype(np.float64), ref["true_positive"].astype(np.float64)
    want = ref["iou"].astype(np.float64)
    bound = tp * U * np.maximum(want, 1e-6)
    assert (np.abs(got - want) <= bound).all(), (got.tolist(), want.tolist(), bound.tolist())
    one = np.float32(1)
    den = np.maximum(ref["true_positive"] + ref["false_positive"] / 2 + ref["false_negative"] / 2, one)
    res = m.compute()
    for k, v in (("pq", ref["iou"] / den), ("sq", ref["iou"] / np.maximum(ref["true_positive"], one)), ("rq", ref["true_positive"] / den)):
        assert np.allclose(res[k].cpu().numpy(), v, rtol=0, atol=1e-5), k


@pytest.mark.parametrize("tc", (1, 0), ids=("tracking", "plain"))
@pytest.mark.parametrize("tag", sorted(PU.scenes()))
def test_fixture_scenes(tag, tc):
    sc = PU.scenes()[tag]
    m, host = device_metric(sc.M, temporally_consistent=bool(tc)), host_metric(temporally_consistent=bool(tc))
    for pair, ref in zip(sc.updates, sc.ref[tc]):
        m.update(*maps(pair))
        host.update(*maps(pair))
        assert_reference(m, ref)
        assert_bitwise(m, host)
    if tag == "hand":
        assert m.true_positive.tolist() == ([3.0, 2.0] if tc else [3.0, 3.0])      # the 0.5 pair and frame 2's background are no hits


@pytest.mark.parametrize("dtype", (torch.int32, torch.int64), ids=("int32", "int64"))
@pytest.mark.parametrize("M", (9, 200, 255))
def test_bitwise_equal_to_the_host_path(M, dtype):
    S = PU.scenes()
    m, host = device_metric(M), host_metric()
    for n, tag in enumerate(("rand0", "rand1", "rand2")):
        pred, gt = maps(S[tag].updates[0], dtype)
        m.update(pred, gt)
        host.update(pred, gt)
        assert_bitwise(m, host)      # after one update ... and after three
        if n == 0:
            assert_reference(m, S[tag].ref[1][0])
    assert float(m.true_positive[1]) == sum(float(S[t].ref[1][0]["true_positive"][1]) for t in ("rand0", "rand1", "rand2"))
    m(pred, gt)                      # forward() is update()
    host(pred, gt)
    assert_bitwise(m, host)


@pytest.mark.parametrize("reps,M", ((1, 255), (35, 9)), ids=("B6_K256", "B210"))
def test_more_items_and_frames_than_tally_threads(reps, M):
    """B * (K - 1) = 1530 and 1890 walks, and B * T = 1050 frames: more than one pass of the tally workgroup's 1024 threads."""
    S = PU.scenes()
    pred, gt = (torch.cat([maps(S[t].updates[0])[i] for t in ("rand0", "rand1")] * reps) for i in (0, 1))
    assert pred.shape[0] == 6 * reps
    m, host = device_metric(M), host_metric()
    m.update(pred, gt)
    host.update(pred, gt)
    assert_bitwise(m, host)
    want = sum(float(S[t].ref[1][0]["true_positive"][1]) for t in ("rand0", "rand1")) * reps
    assert float(m.true_positive[1]) == want and float(m.false_negative[1]) > 0


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_eval_golden_scenes(seed):
    from streamingflow_amd import instance as I
    G = gold("eval.npz")
    out, labels = cases.eval_scene(seed)
    cons = I.predict_instance_segmentation_and_trajectories({k: v.cuda() for k, v in out.items()}, compute_matched_centers=False, make_consistent=True)
    pq, host = device_metric(50).cuda(), host_metric().cuda()
    pq(cons, labels["instance"].cuda())
    host(cons, labels["instance"].cuda())
    res = pq.compute()
    for k in ("true_positive", "false_positive", "false_negative"):
        assert np.array_equal(getattr(pq, k).cpu().numpy(), G[f"pq_{k}_{seed}"]), k
    assert np.allclose(pq.iou.cpu().numpy(), G[f"pq_iou_{seed}"], atol=1e-5)
    assert np.allclose(res["pq"].cpu().numpy(), G[f"pq_{seed}"], atol=1e-5)
    assert_bitwise(pq, host)
    pq.reset()
    assert float(pq.true_positive.sum()) == 0.0


def test_vehicles_id_2_turns_tracking_off():
    for tag in ("rand0", "hand"):
        sc = PU.scenes()[tag]
        m, host = device_metric(sc.M, vehicles_id=2), host_metric(vehicles_id=2)
        m.update(*maps(sc.updates[0]))
        host.update(*maps(sc.updates[0]))
        assert_reference(m, sc.ref[0][0])
        assert_bitwise(m, host)
        assert not np.array_equal(sc.ref[0][0]["true_positive"], sc.ref[1][0]["true_positive"])


def _wrong(kind, pred, gt, M):
    pred, gt = pred.clone(), gt.clone()
    if kind == "pred_above":
        pred[1, 2, 3, 4] = M + 1
    elif kind == "gt_above":
        gt[0, 0, 0, 0] = M + 1
    elif kind == "negative":
        gt[2, 4, 5, 6] = -1
    else:
        gt = gt + 1      # ids 1 .. 6: no background pixel anywhere
        assert int(gt.min()) == 1 and int(gt.max()) <= M
    return pred, gt


@pytest.mark.parametrize("kind", ("pred_above", "gt_above", "negative", "no_background"))
def test_wrong_labels_add_nothing_and_compute_raises(kind):
    sc = PU.scenes()["rand3"]
    pred, gt = maps(sc.updates[0])
    m = device_metric(sc.M)
    m.update(pred, gt)
    before = counters(m)
    m.compute()                                      # clean so far
    m.update(*_wrong(kind, pred, gt, sc.M))          # does not raise: the data is not looked at on the host
    for k in PU.COUNTERS:
        assert torch.equal(getattr(m, k), before[k]), k
    with pytest.raises(ValueError, match="no pixel of id 0" if kind == "no_background" else "outside"):
        m.compute()
    m.update(pred, gt)                               # a later clean update counts, the flag stays until reset()
    with pytest.raises(ValueError):
        m.compute()
    m.reset()
    assert all(float(getattr(m, k).sum()) == 0.0 for k in PU.COUNTERS)
    m.update(pred, gt)
    assert_reference(m, sc.ref[1][0])


def test_constructor_and_shape_errors():
    from streamingflow_amd.metrics import PanopticMetric
    assert PanopticMetric.MAX_INSTANCES >= 255
    for bad in (0, -3, PanopticMetric.MAX_INSTANCES + 1, 2.0, True):
        with pytest.raises(ValueError):
            PanopticMetric(2, max_instances=bad)
    PanopticMetric(2, max_instances=PanopticMetric.MAX_INSTANCES)
    m = device_metric(9)
    z = torch.zeros(1, 2, 4, 4, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        m.update(z, z[:, :1])
    with pytest.raises(ValueError):
        m.update(z[0], z[0])
    with pytest.raises(RuntimeError):
        m.update(z.cpu(), z.cpu())


def test_evaluation_step_is_captured_in_a_graph():
    """argmax, IntersectionOverUnion.update, the instance post-processing and PanopticMetric.update recorded once and replayed on
    another scene: a call that waits on the host inside the capture is an error, so the capture itself is the check."""
    from streamingflow_amd import instance as I
    from streamingflow_amd.metrics import IntersectionOverUnion

    def load(seed):
        out, labels = cases.eval_scene(seed)
        return {**{k: v.cuda() for k, v in out.items()}, "gt_seg": labels["segmentation"].cuda(), "gt_inst": labels["instance"].cuda()}

    def step(data, iou, pq):
        seg = torch.argmax(data["segmentation"], dim=2, keepdim=True)
        iou.update(seg, data["gt_seg"])
        ids = I.predict_instance_segmentation_and_trajectories({k: data[k] for k in ("segmentation", "instance_center", "instance_offset",
                                                                                     "instance_flow")})
        pq.update(ids, data["gt_inst"])

    first, second = load(0), load(1)
    static = {k: v.clone() for k, v in first.items()}
    iou, pq = IntersectionOverUnion(2).cuda(), device_metric(50).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(static, iou, pq)                        # warm-up: workspaces, kernel attributes, the counters' device
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(static, iou, pq)
    for k in static:
        static[k].copy_(second[k])
    iou.reset()
    pq.reset()
    graph.replay()
    torch.cuda.synchronize()
    want_iou, want_pq = IntersectionOverUnion(2).cuda(), device_metric(50).cuda()
    step(second, want_iou, want_pq)
    for k in ("true_positive", "false_positive", "false_negative", "support"):
        assert torch.equal(getattr(iou, k), getattr(want_iou, k)), k
    assert_bitwise(pq, want_pq)
    other = device_metric(50).cuda()
    step(first, IntersectionOverUnion(2).cuda(), other)
    assert not torch.equal(other.iou, want_pq.iou)      # the two scenes do differ
    assert float(pq.true_positive[1]) >= 3 and torch.equal(pq.compute()["pq"], want_pq.compute()["pq"])


def _score(K=10, B=1, T=2, n=64, n_classes=2, ws_bytes=None, null=None):
    """sf_panoptic_score_fwd on zero histograms of K0 = 10 -> (status, counters and error int as numpy); the counters start at 7."""
    from streamingflow_amd import _lib, runtime
    from streamingflow_amd.runtime import ptr
    L = _lib.lib()
    K0, B0, T0 = 10, 1, 2
    arg = {"hist": torch.zeros((B0 * T0, K0, K0), dtype=torch.int64, device="cuda"), "bad": torch.zeros(1, dtype=torch.int32, device="cuda"),
           "errors": torch.zeros(1, dtype=torch.int32, device="cuda")}
    arg["hist"][:, 0, 0] = 64
    for k in PU.COUNTERS:
        arg[k] = torch.full((2,), 7.0, device="cuda")
    need = L.sf_panoptic_score_ws_bytes(B0, T0, K0)
    assert need > 0
    arg["ws"] = torch.empty((need + 3) // 4, dtype=torch.int32, device="cuda")
    if null:
        arg[null] = None
    status = L.sf_panoptic_score_fwd(ptr(arg["hist"]), n, B, T, K, n_classes, 1, ptr(arg["bad"]), ptr(arg["iou"]), ptr(arg["true_positive"]),
                                     ptr(arg["false_positive"]), ptr(arg["false_negative"]), ptr(arg["errors"]), ptr(arg["ws"]),
                                     need if ws_bytes is None else ws_bytes, runtime.stream_ptr(torch.device("cuda")))
    torch.cuda.synchronize()
    return status, {k: v.cpu().numpy() for k, v in arg.items() if v is not None and k not in ("hist", "ws")}


def test_argument_checks():
    from streamingflow_amd import _lib
    L = _lib.lib()
    assert _lib.SF_PANOPTIC_MAX_K >= 256
    assert L.sf_panoptic_score_ws_bytes(1, 2, _lib.SF_PANOPTIC_MAX_K) > 0 and L.sf_panoptic_score_ws_bytes(1, 2, _lib.SF_PANOPTIC_MAX_K + 1) == 0
    assert L.sf_panoptic_score_ws_bytes(0, 2, 6) == 0 and L.sf_panoptic_score_ws_bytes(1, 0, 6) == 0 and L.sf_panoptic_score_ws_bytes(1, 2, 0) == 0
    refused = [{"K": 0}, {"K": -1}, {"K": _lib.SF_PANOPTIC_MAX_K + 1}, {"B": 0}, {"T": 0}, {"n": 0}, {"n": 1 << 23}, {"n_classes": 1}]
    refused += [{"null": k} for k in ("hist", "bad", "errors", "ws") + PU.COUNTERS]
    for kw in refused:
        status, left = _score(**kw)
        assert status == SF_ERR_INVALID, kw
        assert all((left[k] == 7.0).all() for k in PU.COUNTERS if k in left), kw      # nothing was launched
    need = L.sf_panoptic_score_ws_bytes(1, 2, 10)
    status, left = _score(ws_bytes=need - 1)
    assert status == SF_ERR_WORKSPACE and all((left[k] == 7.0).all() for k in PU.COUNTERS)
    status, left = _score(ws_bytes=need)             # two all-background frames: two class-0 true positives of IoU 1, added in place
    assert status == SF_OK and left["errors"].tolist() == [0]
    assert left["true_positive"].tolist() == [9.0, 7.0] and left["iou"].tolist() == [9.0, 7.0]
    assert left["false_positive"].tolist() == [7.0, 7.0] and left["false_negative"].tolist() == [7.0, 7.0]
