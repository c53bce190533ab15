"""Streaming sessions: the GRU-ODE state of ONE sensor stream carried across calls.

``FuturePredictionODE.forward`` starts from ``state = zeros`` and re-encodes / re-propagates every observation of its window.  A
session ingests observations one at a time (``observe``: the ODE steps up to the observation, the Bayesian jump, ``infer_state``)
and answers prediction requests from a fork of the carried state (``predict``: the target loop on a copy; the trunk is untouched).
The segments are the ops of the one-shot rollout over "all observations since ``reset()``", enqueued through the resumable entry
points ``sf_nnfo_rollout_resume_*_fwd`` (include/sfnative.h) — same kernels, same order, same noise numbering — so a session
reproduces the one-shot call on the same observations (bitwise at the latent level with fed noise).

``StreamSession``        latent level (``NNFOwithBayesianJumps.stream``): encoded observations in, latent states out.
``FutureStreamSession``  model level (``FuturePredictionODE.stream``): BEV frames in, ``forward(...)[0]``-shaped predictions out.
"""
import collections

import torch

from . import _lib, runtime, schedule as sched

_MODULE_NOISE = object()


class StreamSession:
    """Carried latent state of one stream on a ``NNFOwithBayesianJumps`` module (one sample; open one session per stream — any
    number may be open on a module, each with its own state, path, draw counter, static buffers and graphs).

    Noise.  The trunk consumes draws in reference order (one per jump, ``DRAWS_PER_STEP[solver]`` per step); a branch continues
    from the trunk's counter WITHOUT advancing it — the numbering the one-shot call gives the same ops.  Consequence: two
    ``predict`` calls from the same trunk state see the same noise, and the draws a branch used are the ones the next ``observe``
    uses (``fresh_noise=True`` gives a branch draws of its own).  Sources: ``noise`` = a callable ``(shape, dtype, device) ->
    NCHW eps`` called once per draw number in increasing order (default: the module's ``noise`` at creation); without one, either
    the in-kernel Philox noise (the module's ``in_kernel_noise`` rule; one ``call`` number of the module's counter per epoch,
    taken when the session is created / ``reset()``, and the trunk counter as ``draw_base``) or ``torch.randn`` rows on the device.

    Failures.  ``observe`` advances the host schedule only after its segment was enqueued.  If enqueuing fails half-way (a noise
    source that raises, a workspace or capture error) the carried buffers may be partly written: the session then refuses
    ``observe`` / ``predict`` with RuntimeError until ``reset()``.

    Path history.  Every observation's state is a path entry the selection (temporal_ode_bayes.py:606-620) may pick; the last
    ``history`` of them are kept (640 KB each at C = 64, 50x50).  ``predict`` raises ValueError when an evicted entry could be the
    answer (schedule.StreamSchedule) — it never returns anything but what the one-shot call over the same observations returns.

    Graphs.  Under the module's auto rule (h*w < 4096, not inside a capture) segments replay captured graphs from a cache the
    session owns (``GRAPH_CACHE_MAX`` structures, least recently used out).  The draw number is a kernel argument of the Philox
    epilogue, so a captured Philox segment is tied to its ``draw_base``: with in-kernel noise segments run eagerly unless
    ``use_graph=True`` (then the key includes ``draw_base``); fed noise has no such tie.

    Weights.  A re-pack of the module's weights (load_state_dict, .to(), in-place update) between two calls makes the carried state
    meaningless and the captured pointers stale: the next ``observe`` / ``predict`` raises RuntimeError until ``reset()``."""

    GRAPH_CACHE_MAX = 8

    def __init__(self, ode, delta_t, history=16, noise=_MODULE_NOISE, use_graph=None):
        if ode.training:
            raise RuntimeError("streamingflow_amd is inference-only: call .eval() before opening a session")
        self.ode, self.delta_t, self.history = ode, float(delta_t), history
        self.noise = ode.noise if noise is _MODULE_NOISE else noise
        self.use_graph = use_graph
        self._sched = sched.StreamSchedule(delta_t, ode.use_variable_ode_step, ode.solver, history)
        self._graphs = runtime.GraphCache()
        self._bufs = None            # (state, p, carry): the trunk's static device buffers, updated in place
        self._hist = collections.deque()
        self._gens = None
        self._broken = None
        self.reset()

    # ---- bookkeeping --------------------------------------------------------------------------
    @property
    def current_time(self):
        return self._sched.current_time

    @property
    def last_time(self):
        """Time of the latest observation (None before the first): ``observe`` refuses an earlier one."""
        return self._sched.last_time

    @property
    def n_draws(self):
        """Noise draws the trunk has consumed since ``reset()`` (= ``draw_base`` of the next segment)."""
        return self._sched.n_draws

    @property
    def n_observations(self):
        return self._sched.n_obs

    @property
    def state(self):
        """The carried latent state [h, w, C] (a copy)."""
        if self._bufs is None:
            raise RuntimeError("no observation yet")
        return self._bufs[0][0].clone()

    def __getstate__(self):
        raise TypeError("a StreamSession holds device buffers and captured graphs of this process: open a new one instead of copying")

    def drop_graphs(self):
        self._graphs.drop()

    def reset(self):
        """State and imputed input to zeros, draw counter to 0, path emptied, new noise epoch."""
        self._sched.reset()
        self._hist.clear()
        self._rows = {}              # fed noise: draw number -> [1, h, w, C] row (rows below the trunk counter are dropped)
        self._pulled = 0             # draws taken from the noise source so far
        self._broken = None
        # Philox `call` number of this epoch: taken here, so that one-shot calls on the module between now and the first observe do
        # not shift it (None: fed noise now — taken at the first segment should the session be switched to in-kernel noise later)
        self._call = None
        if self._in_kernel():
            self.ode._noise_calls += 1
            self._call = self.ode._noise_calls
        if self._bufs is not None:
            for t in self._bufs:
                t.zero_()
        gens = self.ode._pack_generations() if self._gens is not None else None
        if gens != self._gens:
            self.drop_graphs()
            self._gens = None

    def _check(self, *tensors):
        if self.ode.training:
            raise RuntimeError("streamingflow_amd is inference-only: the module was put into .train() mode")
        if self._broken is not None:
            raise RuntimeError(f"an observe of this session failed while its segment was being enqueued ({self._broken}): the carried "
                               "state may be partly written — call reset() and feed the stream again")
        runtime.require_cuda(*tensors)
        runtime.require_no_grad(*tensors)
        gens = self.ode._pack_generations()
        if self._gens is None:
            self.drop_graphs()
            self._gens = gens
        elif gens != self._gens:
            raise RuntimeError("the module's weights were re-packed (load_state_dict / .to() / in-place update) since this session's "
                               "state was computed: call reset() and feed the stream again")

    def _in_kernel(self):
        return self.ode._in_kernel(self.noise)

    # ---- noise ------------------------------------------------------------------------------------
    def _eps(self, base, n, shape, dev, fresh=False):
        """[max(n, 1), 1, h, w, C]: the draws numbered base .. base + n - 1 (cached: a branch and the trunk segment after it read
        the same rows)."""
        if n == 0:
            return torch.zeros((1, 1) + tuple(shape), dtype=torch.float32, device=dev)
        if fresh:
            if self.noise is not None:
                raise ValueError("fresh_noise with an injected noise source: the source defines the draws (inject another one)")
            return torch.randn((n, 1) + tuple(shape), dtype=torch.float32, device=dev)
        while self._pulled < base + n:
            self._rows[self._pulled] = (torch.randn((1,) + tuple(shape), dtype=torch.float32, device=dev) if self.noise is None
                                        else self.ode._draw_eps(self.noise, 1, 1, *shape[:2], dev)[0])
            self._pulled += 1
        return torch.stack([self._rows[k] for k in range(base, base + n)], 0)

    # ---- one segment ------------------------------------------------------------------------------
    def _enqueue(self, seg, trunk, hx, eps, philox, coef, out, ws, base, shape):
        """One segment from the carried (state, p, carry): the trunk writes all three back in place, a branch only reads them."""
        h, w, C = shape
        state, p, carry = self._bufs
        state_out, p_out, carry_out = (state, p, carry) if trunk else (None, None, None)
        self.ode._enqueue(seg, hx, eps, philox, coef, 0, out, state_out, 1, h, w, ws, state.device,
                          resume=(state, p, carry, base, p_out, carry_out))

    def _segment_noise(self, seg, base, shape, dev, fresh):
        """(eps, philox) of one segment: the {seed, call} record of this epoch (of its own for a fresh branch), or the fed rows."""
        if not self._in_kernel():
            return self._eps(base, seg.n_draws, shape, dev, fresh), None
        o = self.ode
        call = self._call
        if call is None or fresh:
            call = o._noise_calls = o._noise_calls + 1
            if not fresh:
                self._call = call
        return None, torch.tensor([o._philox_seed(), call], dtype=torch.int64, device=dev)

    def _run(self, seg, trunk, hx, base, shape, dev, fresh=False):
        """Enqueue one segment from the carried (state, p, carry).  trunk: they are updated in place and nothing is returned;
        branch: they are only read and the selected states [n_sel, 1, h, w, C] are returned (None when the branch selects none)."""
        h, w, C = shape
        n_sel = len(seg.sel_nops)
        if not seg.ops:
            return None
        eps, philox = self._segment_noise(seg, base, shape, dev, fresh)
        coef = torch.from_numpy(seg.coef_array()).to(dev)
        nbytes = _lib.lib().sf_nnfo_rollout_ws_bytes(C, 1, h, w)
        graph = self.use_graph
        if graph is None:
            graph = h * w < 4096 and philox is None and not torch.cuda.is_current_stream_capturing()
        if not graph:
            out = torch.empty((n_sel, 1, h, w, C), dtype=torch.float32, device=dev) if n_sel else None
            self._enqueue(seg, trunk, hx, eps, philox, coef, out, runtime.workspace(nbytes, dev), base, shape)
            return out
        # (the key says whether p_out is produced — trunk — and, for the Philox form, which draw numbers the kernels were captured with)
        key = (bool(trunk), seg.key(), int(base) if philox is not None else None, shape) + self.ode._graph_key_tail(dev, philox is not None)
        feeds = {"hx": hx.reshape(1, 1, h, w, C) if trunk else None, "eps": eps, "philox": philox, "coef": coef}
        g = self._graphs.get(key)
        if g is not None:
            for k, v in feeds.items():
                if v is not None:
                    g[k].copy_(v)
            self._graphs.replay(g, dev)
        else:
            g = {k: v.clone() if v is not None else None for k, v in feeds.items()}
            g["out"] = torch.empty((n_sel, 1, h, w, C), dtype=torch.float32, device=dev) if n_sel else None
            g["ws"] = runtime.static_workspace(nbytes, dev)
            # The first run of a structure is the real one, eager; the capture that follows only records the same calls — a trunk
            # segment updates the carried state in place and must run exactly once, so nothing is replayed here.
            self._graphs.capture(key, g, lambda: self._enqueue(seg, trunk, g["hx"], g["eps"], g["philox"], g["coef"], g["out"], g["ws"],
                                                               base, shape), dev, self.GRAPH_CACHE_MAX)
        return g["out"]      # the graph's static buffer (valid until its next replay): predict() copies the rows it returns out of it

    # ---- public -----------------------------------------------------------------------------------
    def observe(self, t, hx):
        """Ingest the observation at time ``t``: ``hx`` [h, w, C] (or [1, h, w, C]) NHWC fp32, already encoded.  Enqueues the ODE
        steps from the carried time up to ``t``, the jump and its ``infer_state``; the state after the jump becomes a path entry.
        Times must not decrease (ValueError); on equal times the order of the calls is the order of the jumps."""
        self._check(hx)
        if hx.dim() == 4 and hx.shape[0] == 1:
            hx = hx[0]
        C = self.ode.hidden_size
        if hx.dim() != 3 or hx.shape[-1] != C or hx.dtype != torch.float32:
            raise ValueError(f"hx must be an encoded observation [h, w, {C}] fp32 (NHWC), got {tuple(hx.shape)} {hx.dtype}")
        shape, dev = tuple(hx.shape), hx.device
        if self._bufs is None or tuple(self._bufs[0].shape[1:]) != shape or self._bufs[0].device != dev:
            if self._sched.n_obs:
                raise ValueError(f"observation shape / device changed mid-stream: {shape} on {dev}")
            h, w, _ = shape
            carry = _lib.lib().sf_nnfo_rollout_carry_bytes(C, 1, h, w) // 4
            self._bufs = (torch.zeros((1,) + shape, dtype=torch.float32, device=dev),
                          torch.zeros((1,) + shape, dtype=torch.float32, device=dev),
                          torch.zeros(carry, dtype=torch.float32, device=dev))
            self.drop_graphs()
        base = self._sched.n_draws
        seg = self._sched.plan_observe(t)     # raises on a time earlier than the previous one; the trunk is not advanced yet
        try:
            self._run(seg, True, hx.contiguous(), base, shape, dev)
        except Exception as ex:               # buffers possibly half-updated: no later call may answer from them
            self._broken = f"{type(ex).__name__}: {ex}"
            raise
        self._sched.commit_observe(seg)
        for k in [k for k in self._rows if k < self._sched.n_draws]:
            del self._rows[k]
        self._hist.append(self._bufs[0][0].clone())
        while len(self._hist) > len(self._sched.path_t):
            self._hist.popleft()

    def predict(self, targets, fresh_noise=False):
        """Latent states [n_T, h, w, C] for the target times (any order, as ``forward``'s T), computed on a fork of the carried
        (state, imputed input, time, draw counter): the trunk is untouched.  ``fresh_noise``: this branch draws noise of its
        own instead of the draws the one-shot call would give its ops."""
        self._check()
        if torch.is_tensor(targets):
            targets = targets.reshape(-1).tolist()
        br = self._sched.predict(targets)     # RuntimeError before any observation, ValueError for an evicted path entry
        state = self._bufs[0]
        shape, dev = tuple(state.shape[1:]), state.device
        out = self._run(br.seg, False, None, br.base_draws, shape, dev, fresh_noise)
        rows = [self._hist[j] if src == "trunk" else out[j, 0] for src, j in br.source]
        if not rows:
            return torch.empty((0,) + shape, dtype=torch.float32, device=dev)
        return torch.stack(rows, 0)


class FutureStreamSession:
    """Streaming form of ``FuturePredictionODE.forward`` for one stream (batch 1).

    ``observe(t, frame, source)`` encodes that frame alone (one SmallEncoder pass) and ingests it; ``predict(target_timestamp)``
    returns ``[1, T, C, H, W]`` with the layout and meaning of ``forward(...)[0]`` for the observations ingested since
    ``reset()``: latent predict, SmallDecoder, then the module's unchanged head.  ``forward`` merges camera and LiDAR frames by
    time with camera first on equal times (schedule.merge_observations); a session takes them in the order of the calls, so a
    caller that wants ``forward``'s result feeds the camera frame first on a tie.  Everything else: ``StreamSession``."""

    def __init__(self, net, history=16, noise=_MODULE_NOISE, use_graph=None):
        self.net = net
        self.latent = StreamSession(net.gru_ode, net.delta_t, history=history,
                                    noise=net.gru_ode.noise if noise is _MODULE_NOISE else noise, use_graph=use_graph)

    def __getstate__(self):
        raise TypeError("a FutureStreamSession holds device buffers of this process: open a new one instead of copying")

    def reset(self):
        self.latent.reset()

    @property
    def current_time(self):
        return self.latent.current_time

    def observe(self, t, frame, source="camera"):
        """``frame``: [C, H, W] or [1, C, H, W] NCHW BEV features of the camera or LiDAR branch at time ``t``."""
        if source not in ("camera", "lidar"):
            raise ValueError("source must be 'camera' or 'lidar'")
        if self.net.training:
            raise RuntimeError("streamingflow_amd is inference-only: call .eval()")
        runtime.require_cuda(frame)
        runtime.require_no_grad(frame)
        if frame.dim() == 3:
            frame = frame[None]
        if frame.dim() != 4 or frame.shape[0] != 1:
            raise ValueError(f"frame must be [C, H, W] or [1, C, H, W], got {tuple(frame.shape)}")
        if self.latent.last_time is not None and float(t) < self.latent.last_time:      # before paying for the encoder pass
            raise ValueError(f"observation at {float(t)} after one at {self.latent.last_time}: feed the stream in time order")
        self.latent._check(frame)
        hx = self.net.gru_ode.srvp_encoder.forward_nhwc(runtime.to_nhwc(frame))
        self.latent.observe(t, hx[0])

    def predict(self, target_timestamp, fresh_noise=False):
        if self.net.training:
            raise RuntimeError("streamingflow_amd is inference-only: call .eval()")
        if torch.is_tensor(target_timestamp):
            if target_timestamp.dim() == 2 and target_timestamp.shape[0] != 1:
                raise ValueError("one stream per session: target_timestamp must be [T] or [1, T]")
            target_timestamp = target_timestamp.reshape(-1).tolist()
        states = self.latent.predict(target_timestamp, fresh_noise)
        if states.shape[0] == 0:
            raise ValueError("predict needs at least one target time")
        x = self.net.gru_ode.srvp_decoder.forward_nhwc(states)
        return self.net._head_to_nchw(x.view(x.shape[0], 1, *x.shape[1:]), True)
