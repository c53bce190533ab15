"""Host-side step scheduler of the GRU-ODE rollout.

The reference decides, inside ``NNFOwithBayesianJumps.forward`` (streamingflow/layers/
temporal_ode_bayes.py:508-620), when to propagate the ODE, when to apply an observation jump and
which visited state answers each target timestamp — interleaved with device work and with one
device->host sync per comparison.  The schedule is a pure float64 function of
``(observation times, target times, delta_t, USE_VARIABLE_ODE_STEP)``; this module computes it up
front so that the whole rollout can be enqueued (and hipGraph-captured) without host syncs.
Python floats are IEEE doubles, i.e. the same arithmetic as the reference's 0-d float64 tensors.
"""
from dataclasses import dataclass, field
from typing import List, Tuple

import numpy as np

from ._lib import OP_JUMP, OP_STEP, SF_COEF_STRIDE

DRAWS_PER_STEP = {"euler": 1, "midpoint": 2, "rk4": 4}


@dataclass
class Schedule:
    ops: List[Tuple[int, int]] = field(default_factory=list)   # (OP_JUMP, obs index) | (OP_STEP, step index)
    dts: List[float] = field(default_factory=list)             # float64 dt of every step
    sel_nops: List[int] = field(default_factory=list)          # per target: number of ops applied to the chosen state
    n_draws: int = 0                                           # eps draws consumed (reference order)
    path_t: List[float] = field(default_factory=list)

    @property
    def n_steps(self):
        return len(self.dts)

    @property
    def n_jumps(self):
        return sum(1 for k, _ in self.ops if k == OP_JUMP)

    def key(self):
        """Structure of the rollout (what a captured hipGraph depends on; dt values do not)."""
        return (tuple(self.ops), tuple(self.sel_nops))

    def ops_array(self):
        return np.asarray(self.ops, dtype=np.int32).reshape(-1)

    def coef_array(self):
        """fp32 coefficient records (SF_COEF_STRIDE per step), each rounded once from float64 —
        the reference multiplies fp32 tensors by float64 scalars, i.e. by fp32(dt), fp32(dt/2)."""
        out = np.zeros((max(1, len(self.dts)), SF_COEF_STRIDE), dtype=np.float32)
        for i, dt in enumerate(self.dts):
            out[i] = [dt, dt / 2, dt / 6, dt / 3, dt / 2, dt / 6, dt / 2, dt / 3, dt, dt / 3, dt / 6, 0.0]
        return out


def merge_observations(camera_ts, lidar_ts):
    """models/future_prediction_ode.py:37-49 for one sample: the dict is keyed by 0-d tensors
    (hashed by identity, so equal times are NOT merged) and sorted by time with a stable sort =>
    camera before lidar on ties.  Returns (times, [(source, index)]) with source 0=camera, 1=lidar."""
    items = [(float(t), 0, i) for i, t in enumerate(camera_ts)] + [(float(t), 1, i) for i, t in enumerate(lidar_ts)]
    items.sort(key=lambda v: v[0])
    return [v[0] for v in items], [(v[1], v[2]) for v in items]


def build_schedule(times, targets, delta_t, variable, solver="euler") -> Schedule:
    """Restates temporal_ode_bayes.py:508-620.  ``times``: sorted observation times (float64),
    ``targets``: target times in the order given (not necessarily sorted)."""
    if len(times) == 0:
        raise ValueError("at least one observation is required (reference: times.min() of an empty tensor)")
    delta_t = float(delta_t)
    sch = Schedule()
    per_step = DRAWS_PER_STEP[solver]
    current_time = float(min(times))                                       # :508
    path_t, path_n = [], []

    def step(dt):
        nonlocal current_time
        sch.ops.append((OP_STEP, len(sch.dts)))
        sch.dts.append(dt)
        sch.n_draws += per_step
        current_time = current_time + dt                                   # :458

    for i, obs_time in enumerate(times):                                   # :539
        obs_time = float(obs_time)
        while current_time <= (obs_time - delta_t):                        # :541
            step((obs_time - current_time) if variable else delta_t)       # :546-549
        sch.ops.append((OP_JUMP, i))                                       # :565
        sch.n_draws += 1                                                   # :574
        path_t.append(obs_time)
        path_n.append(len(sch.ops))                                        # :578-581

    for predict_time in targets:                                           # :585
        predict_time = float(predict_time)
        while current_time < predict_time:                                 # :586
            step((predict_time - current_time) if variable else delta_t)   # :590-593
            if predict_time - 0.5 * delta_t < current_time < predict_time + 0.5 * delta_t:
                path_t.append(current_time)                                # :601-604
                path_n.append(len(sch.ops))

    pt = np.array(path_t)
    for time_stamp in targets:                                             # :610-620
        time_stamp = float(time_stamp)
        A = np.where(pt > time_stamp - 0.5 * delta_t)[0]
        B = np.where(pt < time_stamp + 0.5 * delta_t)[0]
        both = A[np.isin(A, B)]
        idx = int(np.max(both)) if both.size else int(np.argmin(np.abs(pt - time_stamp)))
        sch.sel_nops.append(path_n[idx])
    sch.path_t = path_t
    return sch


@dataclass
class Branch:
    """What ``StreamSchedule.predict`` returns: the steps of the target loop as a segment (``seg.sel_nops`` counts the ops of
    the segment, one entry per target the branch itself answers) and, per target in the order given, where its state comes from."""
    seg: Schedule
    sel_nops: List[int]          # per target: ops applied since reset() — the one-shot schedule's ``sel_nops``
    source: List[Tuple[str, int]]  # per target: ("trunk", index into the kept path entries) | ("branch", row of the segment's out_states)
    base_ops: int                # ops / draws of the trunk the branch forks from
    base_draws: int


class StreamSchedule:
    """``build_schedule`` in incremental form, for a caller that learns one observation per call (StreamSession).

    ``observe(t)`` returns the segment the observation loop (temporal_ode_bayes.py:539-581) appends for an observation at ``t``:
    the steps of :541-549 from the carried ``current_time``, then the jump.  ``predict(targets)`` runs the target loop (:585-604)
    and the selection (:606-620) on a COPY of ``current_time``: the trunk is not advanced, so any number of predicts may lie
    between two observes.  Concatenating the segments of every ``observe`` and of a final ``predict`` gives exactly the ops, the
    float64 step sizes and the selection of ``build_schedule(times, targets, ...)`` — the observation loop never looks at the
    targets (tests/test_stream_schedule.py pins this on the 44 reference-captured schedules).

    The selection runs over the path entries the trunk recorded (one per observation) plus the ones the branch adds.  Only the
    last ``history`` trunk entries are kept (None: all); ``predict`` raises ValueError when an evicted entry could be the answer:
    when no kept or branch entry lies within half a delta_t of the target (the reference then takes the nearest entry of the WHOLE
    path, the first one on ties) and an evicted entry may be as near as the nearest kept one.  Evicted entries are older than every
    kept one and a window match takes the LATEST entry, so a target with a kept entry in its window never depends on them.

    A segment numbers its steps and its single observation from 0; ``n_ops`` / ``n_draws`` are the totals since ``reset()``.
    """

    def __init__(self, delta_t, variable, solver="euler", history=None):
        if history is not None and int(history) < 1:
            raise ValueError("history must be at least 1 path entry (or None for all)")
        self.delta_t, self.variable, self.per_step = float(delta_t), bool(variable), DRAWS_PER_STEP[solver]
        self.history = None if history is None else int(history)
        self.reset()

    def reset(self):
        self.current_time = None
        self.n_ops = self.n_draws = self.n_obs = 0
        self.path_t, self.path_n = [], []        # kept trunk path entries
        self.evicted, self.evicted_tmax = 0, None

    @property
    def last_time(self):
        """Time of the latest observation (None before the first): the next one must not be earlier."""
        return self.path_t[-1] if self.path_t else None

    def plan_observe(self, t) -> Schedule:
        """The segment an observation at ``t`` appends, WITHOUT advancing the trunk: a caller that may fail while enqueuing it
        (StreamSession) commits afterwards.  The segment carries the advanced time in ``path_t``."""
        t = float(t)
        if self.path_t and t < self.path_t[-1]:
            raise ValueError(f"observation at {t} after one at {self.path_t[-1]}: a stream cannot be sorted afterwards "
                             "(the reference sorts the whole window); feed observations in time order")
        seg = Schedule()
        ct = t if self.current_time is None else self.current_time             # :508, times.min() of a sorted stream
        while ct <= (t - self.delta_t):                                        # :541
            dt = (t - ct) if self.variable else self.delta_t                   # :546-549
            seg.ops.append((OP_STEP, len(seg.dts)))
            seg.dts.append(dt)
            seg.n_draws += self.per_step
            ct = ct + dt                                                       # :458
        seg.ops.append((OP_JUMP, 0))                                           # :565
        seg.n_draws += 1                                                       # :574
        seg.path_t = [t, ct]
        return seg

    def commit_observe(self, seg):
        """Advance the trunk by a segment ``plan_observe`` returned (for the trunk as it was then)."""
        t, ct = seg.path_t
        self.current_time = ct
        self.n_ops += len(seg.ops)
        self.n_draws += seg.n_draws
        self.n_obs += 1
        self.path_t.append(t)                                                  # :578-581
        self.path_n.append(self.n_ops)
        seg.path_t = [t]
        while self.history is not None and len(self.path_t) > self.history:
            self.evicted_tmax = self.path_t.pop(0)
            self.path_n.pop(0)
            self.evicted += 1

    def observe(self, t) -> Schedule:
        seg = self.plan_observe(t)
        self.commit_observe(seg)
        return seg

    def predict(self, targets) -> Branch:
        if self.current_time is None:
            raise RuntimeError("predict before any observation: the rollout starts at the first observation's time")
        targets = [float(x) for x in targets]
        dt_, seg = self.delta_t, Schedule()
        ct = self.current_time                                                 # a copy: the trunk is not advanced
        bt, bn = [], []
        for predict_time in targets:                                           # :585
            while ct < predict_time:                                           # :586
                dt = (predict_time - ct) if self.variable else dt_             # :590-593
                seg.ops.append((OP_STEP, len(seg.dts)))
                seg.dts.append(dt)
                seg.n_draws += self.per_step
                ct = ct + dt
                if predict_time - 0.5 * dt_ < ct < predict_time + 0.5 * dt_:
                    bt.append(ct)                                              # :601-604
                    bn.append(self.n_ops + len(seg.ops))
        n_trunk = len(self.path_t)
        pt = np.array(self.path_t + bt)
        pn = self.path_n + bn
        sel, source, rows = [], [], {}
        for ts in targets:                                                     # :610-620
            A = np.where(pt > ts - 0.5 * dt_)[0]
            B = np.where(pt < ts + 0.5 * dt_)[0]
            both = A[np.isin(A, B)]
            if both.size:
                idx = int(np.max(both))
            else:
                dist = np.abs(pt - ts)
                idx = int(np.argmin(dist))
                if self.evicted and not (ts > self.evicted_tmax and ts - self.evicted_tmax > float(dist[idx])):
                    raise ValueError(f"target {ts}: no kept path entry within delta_t/2 and an evicted observation state (the last one "
                                     f"at t={self.evicted_tmax}) may be the nearest: raise `history` (now {self.history})")
            sel.append(pn[idx])
            if idx < n_trunk:
                source.append(("trunk", idx))
            else:
                local = pn[idx] - self.n_ops
                if local not in rows:
                    rows[local] = len(seg.sel_nops)
                    seg.sel_nops.append(local)
                source.append(("branch", rows[local]))
        seg.path_t = bt
        return Branch(seg, sel, source, self.n_ops, self.n_draws)
