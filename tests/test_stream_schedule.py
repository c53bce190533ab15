"""CPU: the incremental scheduler (streamingflow_amd.schedule.StreamSchedule) yields, observation by observation, the ops of the
one-shot schedule — pinned on all reference-captured schedules of tests/golden/schedules.json."""
import copy
import json
import os

import pytest

from util import GOLD
from streamingflow_amd import schedule as S
from streamingflow_amd._lib import OP_JUMP, OP_STEP


def _golden():
    with open(os.path.join(GOLD, "schedules.json")) as f:
        return json.load(f)


def _trunk_state(ss):
    return (ss.current_time, ss.n_ops, ss.n_draws, ss.n_obs, list(ss.path_t), list(ss.path_n), ss.evicted, ss.evicted_tmax)


def _concat(segments):
    """Segments (each numbering its steps / its observation from 0) -> ops and dts in the one-shot numbering."""
    ops, dts, n_obs = [], [], 0
    for seg in segments:
        for k, a in seg.ops:
            if k == OP_JUMP:
                assert a == 0
                ops.append((OP_JUMP, n_obs))
                n_obs += 1
            else:
                assert k == OP_STEP
                ops.append((OP_STEP, len(dts)))
                dts.append(seg.dts[a])
    return ops, dts


def test_fixture_has_all_cases():
    assert len(_golden()) == 44


@pytest.mark.parametrize("name", sorted(_golden()))
def test_stream_schedule_matches_one_shot_and_reference(name):
    e = _golden()[name]
    times, _ = S.merge_observations(e["camera_ts"], e["lidar_ts"])
    ref = S.build_schedule(times, e["target_ts"], e["delta_t"], e["variable"])
    ss = S.StreamSchedule(e["delta_t"], e["variable"])
    segs = []
    for i, t in enumerate(times):
        segs.append(ss.observe(t))
        # a predict after every prefix leaves the trunk as it was, and answers like the one-shot schedule of that prefix
        before = _trunk_state(ss)
        br = ss.predict(e["target_ts"])
        assert _trunk_state(ss) == before
        pre = S.build_schedule(times[:i + 1], e["target_ts"], e["delta_t"], e["variable"])
        ops, dts = _concat(segs + [br.seg])
        assert ops == pre.ops and dts == pre.dts and br.sel_nops == pre.sel_nops
        assert br.base_ops == ss.n_ops and br.base_draws == ss.n_draws
    br = ss.predict(e["target_ts"])
    ops, dts = _concat(segs + [br.seg])
    assert ops == ref.ops
    assert dts == ref.dts                               # float64, bit-exact
    assert br.sel_nops == ref.sel_nops == e["select_nops"]
    assert [["jump", None] if k == OP_JUMP else ["step", dts[a]] for k, a in ops] == e["ops"]
    assert ss.n_draws + br.seg.n_draws == ref.n_draws
    # where each answer comes from: a kept trunk entry (an observation's state) or a row of the branch's own outputs
    for n, (src, j) in zip(br.sel_nops, br.source):
        if src == "trunk":
            assert n <= ss.n_ops and ss.path_n[j] == n
        else:
            assert n > ss.n_ops and br.seg.sel_nops[j] == n - ss.n_ops


@pytest.mark.parametrize("solver,per", [("euler", 1), ("midpoint", 2), ("rk4", 4)])
def test_draw_numbering(solver, per):
    times, _ = S.merge_observations([-1, -.5, 0], [-.8, -.6, -.4, -.2, 0])
    targets = [-1, -.5, 0, .5, 1, 1.5, 2]
    ref = S.build_schedule(times, targets, 0.05, True, solver)
    ss = S.StreamSchedule(0.05, True, solver)
    base = 0
    for t in times:
        seg = ss.observe(t)
        assert seg.n_draws == seg.n_jumps + per * seg.n_steps
        base += seg.n_draws
        assert ss.n_draws == base
    br = ss.predict(targets)
    assert br.base_draws == base and base + br.seg.n_draws == ref.n_draws
    assert ss.predict(targets).base_draws == base        # a branch does not advance the trunk's counter


def test_out_of_order_and_predict_before_observe_raise():
    ss = S.StreamSchedule(0.05, True)
    with pytest.raises(RuntimeError):
        ss.predict([0.5])
    ss.observe(-0.5)
    ss.observe(-0.5)          # equal times are an order the caller chose (camera before LiDAR in the reference)
    before = _trunk_state(ss)
    with pytest.raises(ValueError):
        ss.observe(-0.6)
    assert _trunk_state(ss) == before
    ss.reset()
    with pytest.raises(RuntimeError):
        ss.predict([0.5])


def test_history_eviction_raises_only_where_the_answer_could_change():
    cam, lid = [-1, -.5, 0], [-.8, -.6, -.4, -.2, 0]
    times, _ = S.merge_observations(cam, lid)
    full = S.StreamSchedule(0.05, True)
    short = S.StreamSchedule(0.05, True, history=3)
    for t in times:
        full.observe(t)
        short.observe(t)
    assert short.evicted == len(times) - 3 and len(short.path_t) == 3
    future = [0, .5, 1, 1.5, 2]
    assert short.predict(future).sel_nops == full.predict(future).sel_nops
    kept_past = [-.2, 0, 1]
    assert short.predict(kept_past).sel_nops == full.predict(kept_past).sel_nops
    for gone in ([-1.0], [-.5, 1.0], [-.4]):     # the entries at -1, -.5 and -.4 were evicted
        with pytest.raises(ValueError):
            short.predict(gone)
    assert short.predict([-.29]).sel_nops == full.predict([-.29]).sel_nops      # nearest entry of the whole path is the kept -.2
    # an exact tie between an evicted and a kept entry (binary-exact times): the reference's argmin takes the first, the evicted one
    full, short = S.StreamSchedule(0.05, True), S.StreamSchedule(0.05, True, history=2)
    for t in (-1.0, -0.75, -0.5, -0.25):
        full.observe(t)
        short.observe(t)
    assert full.predict([-0.625]).source == [("trunk", 1)]
    with pytest.raises(ValueError):
        short.predict([-0.625])
    assert short.predict([-0.5625]).sel_nops == full.predict([-0.5625]).sel_nops
    full, short = S.StreamSchedule(0.05, True), S.StreamSchedule(0.05, True, history=3)
    for t in times:
        full.observe(t)
        short.observe(t)
    with pytest.raises(ValueError):
        S.StreamSchedule(0.05, True, history=0)
    assert copy.deepcopy(short).predict(future).sel_nops == full.predict(future).sel_nops


def test_plan_observe_does_not_advance_until_committed():
    ss = S.StreamSchedule(0.05, True, history=2)
    for t in (-1.0, -0.8):
        ss.observe(t)
    before = _trunk_state(ss)
    seg = ss.plan_observe(-0.5)
    assert _trunk_state(ss) == before and ss.last_time == -0.8
    assert [k for k, _ in seg.ops] == [OP_STEP, OP_JUMP] and seg.n_draws == 2
    with pytest.raises(ValueError):
        ss.plan_observe(-0.9)
    ss.commit_observe(seg)
    twin = S.StreamSchedule(0.05, True, history=2)
    for t in (-1.0, -0.8, -0.5):
        twin.observe(t)
    assert _trunk_state(ss) == _trunk_state(twin) and ss.last_time == -0.5 and ss.evicted == 1
