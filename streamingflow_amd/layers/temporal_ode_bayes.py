"""MI355X-native GRU-ODE with Bayesian jumps (streamingflow/layers/temporal_ode_bayes.py).

``DualGRUODECell`` (:64-161), ``DualGRUCell`` (:211-305), ``GRUObservationCell`` (:308-344) and
``NNFOwithBayesianJumps`` (:355-627) with the reference constructor/forward signatures and
``state_dict`` keys; the arithmetic runs on libsfnative (HIP, gfx950).

Differences a caller can observe (all documented in DESIGN.md):
  * the step schedule is computed on the host up front (streamingflow_amd.schedule) — no
    device->host sync inside the rollout, which is enqueued as one C call / one hipGraph;
  * the Gaussian noise of ``infer_state`` is drawn for the whole rollout in one call
    (``torch.randn`` on the device) or supplied through ``self.noise`` (parity tests);
  * ``solver='rk4'`` is accepted in addition to the reference's 'euler' / 'midpoint';
  * inference only (no autograd), batch 1 per call as in the reference.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import _lib, packing, runtime, schedule as sched
from ..runtime import PackedModule, ptr
from .convolutions import Bottleblock
from .res_models import ConvNet, SmallDecoder, SmallEncoder
from .temporal import conv_nhwc, gru_cell_nhwc, pack_gru, pack_gru_block, pack_trust_gate, trust_mix_nhwc


class _SingleGRU(PackedModule):
    """Single-branch conv-GRU cells of temporal_ode_bayes.py (``SpatialGRUODECell`` :14-61,
    ``SpatialGRUCell`` :165-208): gates = conv3x3 + bias + sigmoid, candidate = ConvBlock (conv3x3,
    BatchNorm, ReLU).  Defined by the reference but not instantiated on the shipped path."""
    ode = False

    def __init__(self, input_size, hidden_size, gru_bias_init=0.0, norm='bn', activation='relu', bias=True):
        super().__init__()
        if norm != 'bn' or activation != 'relu':
            raise NotImplementedError("conv + BatchNorm + ReLU candidate only")
        from ..beverse.basic_modules import ConvBlock
        self.input_size, self.hidden_size, self.bias, self.gru_bias_init = input_size, hidden_size, bias, gru_bias_init
        cat = input_size + hidden_size
        self.conv_update = nn.Conv2d(cat, hidden_size, kernel_size=3, bias=True, padding=1)
        self.conv_reset = nn.Conv2d(cat, hidden_size, kernel_size=3, bias=True, padding=1)
        self.conv_state_tilde = ConvBlock(cat, hidden_size, kernel_size=3, bias=False, norm=norm, activation=activation)

    _pack = pack_gru_block

    def forward(self, x, state):
        runtime.require_cuda(x, state)
        return runtime.to_nchw(gru_cell_nhwc(self.packed().struct, runtime.to_nhwc(x), runtime.to_nhwc(state), ode=self.ode))


class SpatialGRUODECell(_SingleGRU):
    """dh = u * (h~ - s) (temporal_ode_bayes.py:35-61)."""
    ode = True


class SpatialGRUCell(_SingleGRU):
    """(1 - u) * s + u * h~ (temporal_ode_bayes.py:184-208)."""
    ode = False


class _DualCell(PackedModule):
    """Two conv-GRU branches mixed by a soft 'trusting gate'; 6 fused launches per evaluation."""
    derivative = False

    def __init__(self, input_size, hidden_size, gru_bias_init=0.0, norm='bn', activation='relu', bias=True):
        super().__init__()
        if input_size != hidden_size or hidden_size % 8 or hidden_size > 128:
            raise NotImplementedError("dual GRU cell: input_size == hidden_size, multiple of 8, <= 128")
        self.input_size, self.hidden_size, self.gru_bias_init = input_size, hidden_size, gru_bias_init
        c2 = input_size + hidden_size
        for tag in ("1", "2"):
            for name in ("conv_update_", "conv_reset_", "conv_state_tilde_"):
                setattr(self, name + tag, nn.Conv2d(c2 if tag == "1" else 2 * hidden_size, hidden_size, 3, padding=1))
        self.conv_decoder_2 = nn.Conv2d(hidden_size, hidden_size, kernel_size=3, bias=True, padding=1)
        self.trusting_gate = nn.Sequential(Bottleblock(2 * hidden_size, hidden_size),
                                           nn.Conv2d(hidden_size, 2, kernel_size=1, bias=False))

    def _pack(self):
        C = self.hidden_size
        pk = packing.Pack(_lib.DualW())
        s = pk.struct
        gb = self.gru_bias_init       # added to the gate pre-activations of both cells (:139-140, :154-155)
        g1 = pack_gru(pk, self.conv_update_1, self.conv_reset_1, self.conv_state_tilde_1, C, C, gate_bias=gb)
        # gru_cell_2 is called as gru_cell_2(s, s): its gates see cat[s, s] -> duplicate input folded
        g2 = pack_gru(pk, self.conv_update_2, self.conv_reset_2, self.conv_state_tilde_2, C, C, fold_dup=True, gate_bias=gb)
        s.gates1, s.cand1, s.gates2, s.cand2 = g1.gates, g1.cand, g2.gates, g2.cand
        # the two input halves of gates1 on their own (rollout: the state half is accumulated beside the previous infer_state)
        wg = torch.cat([self.conv_update_1.weight, self.conv_reset_1.weight], 0)
        bg = torch.cat([self.conv_update_1.bias, self.conv_reset_1.bias], 0) + float(gb)
        s.gates1_x = packing.conv_w(pk, wg[:, :C], C, bias=bg, act="sigmoid")
        s.gates1_s = packing.conv_w(pk, wg[:, C:], C)
        s.dec2 = packing.conv_w(pk, self.conv_decoder_2.weight, C, bias=self.conv_decoder_2.bias)
        pack_trust_gate(pk, s, self.trusting_gate, C)
        return pk

    def run_nhwc(self, x, s, out, derivative, base=None, coef=None):
        """x, s, out: [B, h, w, C] (B samples processed as one pixel space)."""
        B, h, w, C = s.shape
        runtime.call("dual_cell", self.packed().struct, ptr(x), ptr(s), ptr(out), int(derivative), ptr(base), ptr(coef), None, 0,
                     B, h, w, device=s.device, scratch=("dual_cell", C, B, h, w))
        return out

    def _general_pack(self):
        """Second packed copy for calls with several present frames: cell 2 then sees two different tensors, so its gate
        convolution keeps both input halves (the main copy folds them, `_pack`)."""
        sig = self._param_signature()
        cache = self.__dict__.get("_sf_general")
        if cache is None or cache[0] != sig:
            C, gb = self.hidden_size, self.gru_bias_init
            pk = packing.Pack(None)
            with torch.no_grad():
                g1 = pack_gru(pk, self.conv_update_1, self.conv_reset_1, self.conv_state_tilde_1, C, C, gate_bias=gb)
                g2 = pack_gru(pk, self.conv_update_2, self.conv_reset_2, self.conv_state_tilde_2, C, C, gate_bias=gb)
                dec2 = packing.conv_w(pk, self.conv_decoder_2.weight, C, bias=self.conv_decoder_2.bias)
            pk.struct = (g1, g2, dec2)
            self.__dict__["_sf_general"] = cache = (sig, pk)
        return cache[1].struct

    def _forward_frames(self, x, state):
        """state [b, n_present > 1, C, h, w] (temporal_ode_bayes.py:101-131 / :248-275): branch 2's hidden state starts from
        the first frame (the ODE cell warms it up over the present frames), both branches start from the last one.
        Unused by the reference's forward path."""
        g1, g2, dec2 = self._general_pack()
        n = state.shape[1]
        frames = [runtime.to_nhwc(state[:, t]) for t in range(n)]
        hid = frames[0]
        if self.derivative:               # only the ODE cell warms branch 2 up (:106-109); the observation cell keeps state[:, 0] (:252)
            for t in range(n - 1):
                hid = gru_cell_nhwc(g2, frames[t], hid)
        r1 = gru_cell_nhwc(g1, runtime.to_nhwc(x[:, 0]), frames[-1])
        hid = gru_cell_nhwc(g2, frames[-1], hid)
        r2 = conv_nhwc(dec2, hid)
        cur = runtime.to_nchw(trust_mix_nhwc(self.packed().struct, r1, r2))
        if not self.derivative:
            return cur
        # the reference returns `cur_state - state.squeeze(1)`: with several frames the squeeze is a no-op and the
        # difference broadcasts over them (one sample)
        if state.shape[0] != 1:
            raise ValueError("DualGRUODECell with n_present > 1: one sample per call (the reference's broadcast)")
        return cur[:, None] - state

    def forward(self, x, state):
        runtime.require_cuda(x, state)
        if x.dim() == 5:
            assert x.shape[2] == self.input_size, f'feature sizes must match, got input {x.shape[2]} for layer with size {self.input_size}'
            if state.shape[1] != 1:
                return self._forward_frames(x, state)
            x, state = x[:, 0], state[:, 0]
        assert x.shape[1] == self.input_size, f'feature sizes must match, got input {x.shape[1]} for layer with size {self.input_size}'
        # note: the reference mis-broadcasts for batch > 1; here every sample of the
        # batch gets the batch-1 semantics
        xn, sn = runtime.to_nhwc(x), runtime.to_nhwc(state)
        out = torch.empty_like(sn)
        if self.derivative:   # cur - s  ==  0 + 1*(cur - s)
            base = torch.zeros_like(sn)
            one = torch.ones(1, dtype=torch.float32, device=sn.device)
            self.run_nhwc(xn, sn, out, True, base, one)
        else:
            self.run_nhwc(xn, sn, out, False)
        return runtime.to_nchw(out)


class DualGRUODECell(_DualCell):
    """ODE derivative f(x, s) = cur - s (temporal_ode_bayes.py:92-131)."""
    derivative = True


class DualGRUCell(_DualCell):
    """Observation update, returns cur (temporal_ode_bayes.py:239-275)."""
    derivative = False


class GRUObservationCell(nn.Module):
    """temporal_ode_bayes.py:308-344: discrete update at an observation; `p` is ignored, loss None."""

    def __init__(self, input_size, hidden_size, min_log_sigma=-5.0, max_log_sigma=5.0, bias=True):
        super().__init__()
        self.gru_d = DualGRUCell(input_size, hidden_size, bias=bias)
        self.input_size, self.prep_hidden, self.var_eps = input_size, hidden_size, 1e-6
        self.min_log_sigma, self.max_log_sigma = min_log_sigma, max_log_sigma

    def forward(self, state, p, X_obs):
        return self.gru_d(X_obs, state), None


class RolloutFeed:
    """The operands a rollout builds on the host — the per-sample step sizes ``coef`` and the noise: the in-kernel record
    {seed, call} or the injected source's eps rows — as device buffers their owner fills, for a caller that records the whole forward
    into a graph of its own (model_graph.ModelGraphSession).  One slot per rollout of a forward, in call order.  Installed as
    ``NNFOwithBayesianJumps.feed``: outside a capture the rollout fills the slot as it goes (making it on first use), inside one it
    copies nothing and only hands the buffers to the kernels; before a replay the owner calls ``fill_feed_slot`` per slot.  ``ops`` and
    ``sel`` stay host arrays read at enqueue: they are the structure such a graph is keyed by."""

    def __init__(self):
        self.slots, self.cursor = [], 0

    def begin(self):
        """Before every pass over the forward (eager, capture): the next rollout takes slot 0."""
        self.cursor = 0


def init_weights(m):
    if type(m) == torch.nn.Linear:
        torch.nn.init.xavier_uniform_(m.weight)
        if m.bias is not None:
            m.bias.data.fill_(0.05)


class NNFOwithBayesianJumps(nn.Module):
    """Neural negative-feedback ODE with Bayesian jumps over BEV latents."""

    def __init__(self, input_size, hidden_size, cfg, bias=True, logvar=True, mixing=1, solver="euler",
                 min_log_sigma=-5.0, max_log_sigma=5.0, impute=False):
        super().__init__()
        self.impute = cfg.MODEL.IMPUTE          # ctor `impute` / `solver` are ignored, as in the reference (:365,:384)
        self.cfg = cfg
        self.min_log_sigma, self.max_log_sigma = min_log_sigma, max_log_sigma
        self.p_model = ConvNet(hidden_size, hidden_size * 2)
        self.gru_c = DualGRUODECell(input_size, hidden_size, bias=bias)
        self.gru_obs = GRUObservationCell(input_size, hidden_size, min_log_sigma=min_log_sigma,
                                          max_log_sigma=max_log_sigma, bias=bias)
        self.skipco = cfg.MODEL.SMALL_ENCODER.SKIPCO
        if self.skipco:      # res_models.py:98-109, :134-147 — not on the shipped path; never silently ignored
            raise NotImplementedError("MODEL.SMALL_ENCODER.SKIPCO=True (encoder -> decoder skip connections) is not built")
        oc, fs = cfg.MODEL.ENCODER.OUT_CHANNELS, cfg.MODEL.SMALL_ENCODER.FILTER_SIZE
        self.srvp_encoder = SmallEncoder(oc, oc, fs)
        self.srvp_decoder = SmallDecoder(oc, oc, fs, self.skipco)
        self.solver = cfg.MODEL.SOLVER
        self.use_variable_ode_step = cfg.MODEL.FUTURE_PRED.USE_VARIABLE_ODE_STEP
        assert self.solver in ["euler", "midpoint", "rk4"], "Solver must be 'euler', 'midpoint' (reference) or 'rk4' (build-defined)."
        self.input_size, self.hidden_size, self.logvar, self.mixing = input_size, hidden_size, logvar, mixing
        self.noise = None    # None: torch.randn on the device; else callable(shape, dtype, device) -> NCHW eps per draw
        # throughput mode: the noise of infer_state is generated inside the sampling epilogue (Philox4x32-10 keyed by
        # (noise_seed, call counter)); no eps tensor exists.  Same distribution, its own stream; ignored when eps is given
        # None = auto: on whenever no `noise` source was injected (nothing to replay), True / False force it
        self.in_kernel_noise = None
        # None = derived at the first draw from torch's global seed (torch.manual_seed reaches the in-kernel noise as it reaches the
        # reference's torch.randn) mixed with the distributed rank and a per-module serial number: ranks and module instances draw
        # different streams.  `seed_noise(seed)` pins it (and restarts the call counter); neither is part of state_dict.
        self.noise_seed = None
        self._noise_calls = 0
        NNFOwithBayesianJumps._serial = getattr(NNFOwithBayesianJumps, "_serial", 0) + 1
        self._noise_serial = NNFOwithBayesianJumps._serial
        # capture the rollout of each schedule structure into a hipGraph and replay it.  None = auto: on for rollouts that
        # run on the launch-bound single-latent kernels (B*h*w < 4096), where ~9 short launches per step are replayed from one
        # graph; the results are cloned out of the graph's static buffers.  True: always, and the returned tensors ARE the
        # static buffers (valid until the next replay); False: never
        self.use_graph = None
        # at most GRAPH_CACHE_MAX captured rollouts are kept, least recently used first out (a stream of variable timestamps produces a
        # new schedule structure per call: each entry pins its own buffers and a rollout workspace); when auto mode sees more than
        # GRAPH_AUTO_MAX_STRUCTURES distinct structures it stops capturing and runs eagerly
        self._graphs = runtime.GraphCache()
        self._graph_structures_seen = set()
        self._graph_gens = None
        # a RolloutFeed while somebody else records the forward into a graph (ModelGraphSession): coef and the noise come from its
        # buffers, this module's own graph cache steps aside
        self.feed = None
        self.apply(init_weights)

    # ---- noise --------------------------------------------------------------------------------
    def _draw_eps(self, noise, n_draws, B, h, w, device):
        """[n_draws, B, h, w, C] fp32 on `device`, one row per infer_state call in reference order, from torch.randn or from the
        injected source `noise` (this module's or a session's): a callable (shape, dtype, device) -> NCHW eps."""
        C = self.hidden_size
        if noise is None:
            return torch.randn((max(1, n_draws), B, h, w, C), dtype=torch.float32, device=device)
        rows = [noise((B, C, h, w), torch.float32, "cpu") for _ in range(n_draws)]
        if not rows:
            return torch.zeros((1, B, h, w, C), dtype=torch.float32, device=device)
        return torch.stack(rows, 0).permute(0, 1, 3, 4, 2).contiguous().to(device=device, dtype=torch.float32)

    def _in_kernel(self, noise):
        """Whether an owner whose injected source is `noise` (this module, a session) draws inside the sampling epilogue."""
        return noise is None and (True if self.in_kernel_noise is None else bool(self.in_kernel_noise))

    # ---- reference API on NCHW tensors ------------------------------------------------------------
    def srvp_encode(self, x):
        b, t, c, h, w = x.shape
        hx = self.srvp_encoder(x.reshape(b * t, c, h, w))
        return hx.view(b, t, *hx.shape[1:]), None

    def srvp_decode(self, x, skip=None):
        b, t, c, h, w = x.shape
        out = self.srvp_decoder(x.reshape(b * t, c, h, w), skip=skip)
        return out.view(b, t, *out.shape[1:])

    def infer_state(self, x, deterministic=False):
        """(:463-477) returns (sample, raw p_model output).  `deterministic` is ignored as in the reference."""
        runtime.require_cuda(x)
        sn = runtime.to_nhwc(x)
        B, h, w, C = sn.shape
        eps = self._draw_eps(self.noise, 1, B, h, w, x.device)
        p = torch.empty_like(sn)
        q = torch.empty((B, h, w, 2 * C), dtype=torch.float32, device=x.device)
        runtime.call("infer_state", self.p_model.packed().struct, ptr(sn), ptr(eps), ptr(p), ptr(q), B, h, w, device=x.device,
                     scratch=("infer_state", C, B, h, w))
        return runtime.to_nchw(p), runtime.to_nchw(q)

    def ode_step(self, state, input, delta_t, current_time):
        """(:436-461) one Euler / midpoint / RK4 step; returns the reference's 5-tuple."""
        runtime.require_cuda(state, input)
        dev = state.device
        sn, pn = runtime.to_nhwc(state), runtime.to_nhwc(input)
        B, h, w, C = sn.shape
        sc = sched.Schedule(dts=[float(delta_t)])
        coef = torch.from_numpy(sc.coef_array()).to(dev)
        eps = self._draw_eps(self.noise, sched.DRAWS_PER_STEP[self.solver], B, h, w, dev)
        s_out, p_out = torch.empty_like(sn), torch.empty_like(pn)
        runtime.call("ode_step", self.gru_c.packed().struct, self.p_model.packed().struct, _lib.SOLVER[self.solver],
                     int(bool(self.impute)), ptr(sn), ptr(pn), ptr(coef), ptr(eps), ptr(s_out), ptr(p_out), B, h, w, device=dev,
                     scratch=("ode_step", C, B, h, w))
        current_time = current_time + delta_t
        return (runtime.to_nchw(s_out), runtime.to_nchw(p_out), current_time,
                torch.tensor([0], device=dev, dtype=torch.float64), torch.tensor([0], device=dev, dtype=torch.float32))

    # ---- the rollout ----------------------------------------------------------------------------
    def _enqueue(self, sc, hx, eps, philox, coef, per_image, out, final, B, h, w, ws, device, resume=None):
        """The C call of a whole rollout (`resume` None) or of one segment of a session (`resume` = state_in, p_in, carry_in,
        draw_base, p_out, carry_out: include/sfnative.h).  The noise is the `philox` record when there is one, else the `eps` rows;
        `ws` is the scratch as ``runtime.call`` takes it: the size query (eager) or a graph's static buffer."""
        L = _lib.lib()
        if resume is None:
            fn, block = (L.sf_nnfo_rollout_fwd if philox is None else L.sf_nnfo_rollout_philox_fwd), ()
        else:
            fn = L.sf_nnfo_rollout_resume_fwd if philox is None else L.sf_nnfo_rollout_resume_philox_fwd
            state_in, p_in, carry_in, draw_base, p_out, carry_out = resume
            block = (ptr(state_in), ptr(p_in), ptr(carry_in), int(draw_base), ptr(p_out), ptr(carry_out))
        ops = sc.ops_array()
        sel = np.asarray(sc.sel_nops, dtype=np.int32)
        runtime.call(fn, self.gru_c.packed().struct, self.gru_obs.gru_d.packed().struct, self.p_model.packed().struct,
                     _lib.SOLVER[self.solver], int(bool(self.impute)), ops.ctypes.data_as(_lib.i32p), len(sc.ops), ptr(hx),
                     ptr(eps if philox is None else philox), ptr(coef), int(per_image), sel.ctypes.data_as(_lib.i32p), len(sel),
                     ptr(out), ptr(final), *block, B, h, w, device=device, scratch=ws)

    def _pack_generations(self):
        """The packed copies a captured graph holds raw pointers into: a graph is stale once any of the three was rebuilt."""
        return (self.gru_c.pack_generation(), self.p_model.pack_generation(), self.gru_obs.gru_d.pack_generation())

    def _graph_key_tail(self, device, philox):
        # (a graph keeps the form, launch per layer / persistent flow, it was captured in)
        return (str(device), self.solver, bool(self.impute), bool(philox), packing._FLOW[0])

    GRAPH_CACHE_MAX = 4
    GRAPH_AUTO_MAX_STRUCTURES = 16

    def seed_noise(self, seed):
        """Pin the seed of the in-kernel (Philox) noise and restart its call counter."""
        self.noise_seed = int(seed) & 0x7FFFFFFFFFFFFFFF
        self._noise_calls = 0
        self._noise_pinned = True

    def _philox_seed(self):
        if self.noise_seed is None:
            rank = torch.distributed.get_rank() if torch.distributed.is_available() and torch.distributed.is_initialized() else 0
            x = (int(torch.initial_seed()) * 0x9E3779B97F4A7C15 + rank * 0xBF58476D1CE4E5B9 + self._noise_serial * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
            x ^= x >> 31
            self.noise_seed = x & 0x7FFFFFFFFFFFFFFF
        return self.noise_seed

    def __getstate__(self):
        # captured graphs (hipGraphExec handles + their static buffers) belong to this object alone: a copy starts without them
        d = runtime.strip_runtime_state(self.__dict__)
        d["_graphs"] = runtime.GraphCache()
        d["_graph_structures_seen"] = set()
        d["_graph_gens"] = None
        d["feed"] = None
        # a copy (copy.deepcopy, an EMA twin, torch.save / load) draws its OWN Philox stream: new instance serial, seed derived again on
        # first use, call counter restarted — unless seed_noise() pinned the seed, which a copy keeps on purpose
        if not d.get("_noise_pinned", False):
            NNFOwithBayesianJumps._serial += 1
            d["_noise_serial"] = NNFOwithBayesianJumps._serial
            d["noise_seed"] = None
            d["_noise_calls"] = 0
        return d

    def drop_graphs(self):
        """Destroy every captured rollout graph of this module and release its static buffers."""
        self._graphs.drop()
        self._graph_structures_seen.clear()

    def _rollout_noise(self, eps, need, B, h, w, device):
        """(eps, philox) of one rollout: the in-kernel record {seed, call} beside an empty eps, or `need` rows, fed or drawn."""
        C = self.hidden_size
        if eps is None and self._in_kernel(self.noise):
            self._noise_calls += 1
            philox = torch.tensor([self._philox_seed(), self._noise_calls], dtype=torch.int64, device=device)
            return torch.empty((0, B, h, w, C), dtype=torch.float32, device=device), philox      # placeholder (shape key of the graph cache)
        if eps is None:
            eps = self._draw_eps(self.noise, need, B, h, w, device)
        elif eps.dim() == 4:
            eps = eps[:, None]
        if eps.shape[0] < need or tuple(eps.shape[1:]) != (B, h, w, C):
            raise ValueError(f"eps must be [{need}, {B}, {h}, {w}, {C}] for solver {self.solver!r}, got {tuple(eps.shape)}")
        return eps, None

    # ---- operands as fed data (RolloutFeed) -------------------------------------------------------------
    @staticmethod
    def _coef_host(scs, per_image):
        """The fp32 step-size records of a rollout, on the host: [steps, SF_COEF_STRIDE], or [steps, B, SF_COEF_STRIDE] per image."""
        return np.ascontiguousarray(np.stack([x.coef_array() for x in scs], axis=1) if per_image else scs[0].coef_array())

    def _feed_mode(self):
        return "philox" if self._in_kernel(self.noise) else ("randn" if self.noise is None else "fed")

    def fill_feed_slot(self, slot, scs):
        """Write one rollout's host-built operands into its slot, as an eager call would have made them: the step sizes of ``scs``
        (schedules of the slot's structure), the next {seed, call} record — ``_noise_calls`` advances, as it does per eager call — or
        the injected source's next eps rows.  Ordinary copies on the current stream: never called inside a capture."""
        s0 = scs[0]
        per_image = len(scs) > 1 and any(x.dts != s0.dts for x in scs)
        if (s0.key(), per_image, len(scs), self._feed_mode()) != slot["sig"][:4] or any(x.key() != s0.key() for x in scs):
            raise ValueError("RolloutFeed: the schedules do not have the structure, grouping and noise mode the slot was made for")
        slot["coef"].copy_(torch.from_numpy(self._coef_host(scs, per_image)))
        if slot["philox"] is not None:
            self._noise_calls += 1
            slot["philox"].copy_(torch.tensor([self._philox_seed(), self._noise_calls], dtype=torch.int64))
        elif slot["sig"][3] == "fed":
            need, B, h, w, _ = slot["eps"].shape
            slot["eps"].copy_(self._draw_eps(self.noise, need, B, h, w, "cpu"))

    def _fed_operands(self, feed, scs, per_image, need, B, h, w, device):
        """(eps, philox, coef) of the feed's next slot.  Outside a capture the slot is (made and) filled here, so an eager forward under
        a feed computes what one without it computes; inside a capture nothing is copied and no counter moves."""
        i = feed.cursor
        feed.cursor += 1
        capturing = torch.cuda.is_current_stream_capturing()
        mode = self._feed_mode()
        C = self.hidden_size
        rows = need if mode == "fed" else 0      # (a schedule has at least one jump: need >= 1)
        sig = (scs[0].key(), per_image, len(scs), mode, rows, B, h, w, str(device))
        if i == len(feed.slots):
            if capturing:
                raise RuntimeError("RolloutFeed: rollout %d has no buffers yet: run the forward once outside the capture first" % i)
            shape = self._coef_host(scs, per_image).shape
            feed.slots.append({"sig": sig, "coef": torch.empty(shape, dtype=torch.float32, device=device),
                               "philox": torch.empty((2,), dtype=torch.int64, device=device) if mode == "philox" else None,
                               "eps": torch.empty((rows, B, h, w, C), dtype=torch.float32, device=device)})
        slot = feed.slots[i]
        if slot["sig"] != sig:
            raise RuntimeError("RolloutFeed: rollout %d changed its structure, shape or noise mode since its buffers were made" % i)
        if not capturing:
            self.fill_feed_slot(slot, scs)
        eps = torch.randn((need, B, h, w, C), dtype=torch.float32, device=device) if mode == "randn" else slot["eps"]
        return eps, slot["philox"], slot["coef"]

    def _auto_graph(self, structure, pixels):
        """`use_graph` None: graphs for the launch-bound single-latent kernels, but not from inside somebody else's capture
        (warm-up, synchronize and a nested capture would break it) and not for an endless variety of schedule structures: the
        set stops growing at the cap, a stream of ever new timestamp structures then runs eagerly, while structures whose graph
        is still cached keep replaying it."""
        if self.use_graph is not None or pixels >= 4096:
            return False
        seen = self._graph_structures_seen
        if len(seen) <= self.GRAPH_AUTO_MAX_STRUCTURES:
            seen.add(structure)
        if torch.cuda.is_current_stream_capturing():
            return False
        return len(seen) <= self.GRAPH_AUTO_MAX_STRUCTURES or any(k[0] == structure for k in self._graphs)

    def _run_eager(self, s0, per_image, hx_obs, eps, philox, coef):
        _, B, h, w, C = hx_obs.shape
        dev = hx_obs.device
        out = torch.empty((len(s0.sel_nops), B, h, w, C), dtype=torch.float32, device=dev)
        final = torch.empty((B, h, w, C), dtype=torch.float32, device=dev)
        self._enqueue(s0, hx_obs, eps, philox, coef, per_image, out, final, B, h, w, ("nnfo_rollout", C, B, h, w), dev)
        return out, final

    def _run_graph(self, s0, per_image, hx_obs, eps, philox, coef):
        """Replay the rollout from the graph of its (structure, shapes); the first call of one warms up eagerly on the static
        buffers and captures, then replays like every later one.  Returns the static buffers (valid until the next replay)."""
        _, B, h, w, C = hx_obs.shape
        dev = hx_obs.device
        # when any of the three packs was rebuilt (load_state_dict, .to(), in-place update) every cached graph is stale
        gens = self._pack_generations()
        if self._graph_gens != gens:
            self.drop_graphs()
            self._graph_gens = gens
        feeds = {"hx": hx_obs, "eps": eps, "coef": coef, "philox": philox}
        key = (s0.key(), per_image, tuple(hx_obs.shape), tuple(eps.shape)) + self._graph_key_tail(dev, philox is not None)
        g = self._graphs.get(key)
        if g is None:
            g = {k: v.clone() if v is not None else None for k, v in feeds.items()}
            g["out"] = torch.empty((len(s0.sel_nops), B, h, w, C), dtype=torch.float32, device=dev)
            g["final"] = torch.empty((B, h, w, C), dtype=torch.float32, device=dev)
            g["ws"] = runtime.static_workspace(_lib.lib().sf_nnfo_rollout_ws_bytes(C, B, h, w), dev)
            self._graphs.capture(key, g, lambda: self._enqueue(s0, g["hx"], g["eps"], g["philox"], g["coef"], per_image, g["out"],
                                                               g["final"], B, h, w, g["ws"], dev), dev, self.GRAPH_CACHE_MAX)
        for k, v in feeds.items():
            if v is not None:
                g[k].copy_(v)
        self._graphs.replay(g, dev)
        return g["out"], g["final"]

    def _flow_checked(self, result, s0, per_image, hx_obs, eps, philox, coef):
        """Persistent flow kernel: a dependency wait that gave up (device shared with another stream / process) must cost time, not
        a result — the same rollout again on the launch-per-layer path, in this process, counted.  Whether it gave up is read from
        THIS rollout's own output (the poison kernel turns every element into NaN), not from sf_flow_errors, whose "most recent
        rollout of the thread" is the most recent one ENQUEUED, not the graph that was just replayed."""
        if not (packing.flow_active() and packing.flow_checked()) or torch.cuda.is_current_stream_capturing():
            return result
        if not bool(torch.isnan(result[1].reshape(-1)[:1]).item()):
            return result
        packing.FLOW_FALLBACKS[0] += 1
        L = _lib.lib()
        was = L.sf_set_flow_mode(0)
        try:
            return self._run_eager(s0, per_image, hx_obs.contiguous(), eps.contiguous(), philox, coef)
        finally:
            L.sf_set_flow_mode(int(bool(was)) if packing._FLOW[0] is not None else -1)

    def rollout_nhwc(self, hx_obs, sc, eps=None):
        """hx_obs: [n_obs, B, h, w, C] (or [n_obs, h, w, C] for one sample) encoded observations in
        time order; sc: one Schedule shared by all samples, or a list of B Schedules with the same
        structure (``Schedule.key()``) and per-sample step sizes.
        Returns (selected states [n_T, B, h, w, C], final state [B, h, w, C]); without the B axis
        when hx_obs had none.  With ``self.use_graph`` the whole rollout (every kernel of every
        step and jump) is captured once per (schedule structure, shape) into a hipGraph and
        replayed; step sizes, observations and noise are fed through static device buffers."""
        one = hx_obs.dim() == 4
        if one:
            hx_obs = hx_obs[:, None]
        n_obs, B, h, w, C = hx_obs.shape
        dev = hx_obs.device
        scs = list(sc) if isinstance(sc, (list, tuple)) else [sc]
        s0 = scs[0]
        if len(scs) not in (1, B) or any(x.key() != s0.key() for x in scs):
            raise ValueError("batched rollout needs one schedule, or one per sample with identical structure")
        per_image = len(scs) > 1 and any(x.dts != s0.dts for x in scs)
        if self.feed is not None:
            if eps is not None:
                raise ValueError("rollout_nhwc under a RolloutFeed takes its noise from the feed, not from `eps`")
            need = s0.n_jumps + sched.DRAWS_PER_STEP[self.solver] * s0.n_steps
            out, final = self._run_eager(s0, per_image, hx_obs, *self._fed_operands(self.feed, scs, per_image, need, B, h, w, dev))
            return (out[:, 0], final[0]) if one else (out, final)
        auto_graph = self._auto_graph(s0.key(), B * h * w)
        # draws the kernels will read: one per jump, DRAWS_PER_STEP[solver] per step (a schedule built for another solver
        # would make them read past the end of eps)
        eps, philox = self._rollout_noise(eps, s0.n_jumps + sched.DRAWS_PER_STEP[self.solver] * s0.n_steps, B, h, w, dev)
        coef_np = np.stack([x.coef_array() for x in scs], axis=1) if per_image else s0.coef_array()
        coef = torch.from_numpy(np.ascontiguousarray(coef_np)).to(dev)
        args = (s0, per_image, hx_obs, eps, philox, coef)
        if self.use_graph or auto_graph:
            out, final = self._run_graph(*args)
            if auto_graph:                          # nobody asked for the zero-copy form: hand out fresh tensors
                out, final = out.clone(), final.clone()
        else:
            out, final = self._run_eager(*args)
        out, final = self._flow_checked((out, final), *args)
        return (out[:, 0], final[0]) if one else (out, final)

    def stream(self, delta_t, history=16, **kw):
        """Open a streaming session on this module (streamingflow_amd.stream.StreamSession): the latent state carried across
        ``observe(t, hx)`` calls, ``predict(targets)`` from a fork of it."""
        from ..stream import StreamSession
        return StreamSession(self, delta_t, history=history, **kw)

    def make_schedule(self, times, delta_t, T):
        return sched.build_schedule([float(t) for t in times], [float(t) for t in T], delta_t,
                                    self.use_variable_ode_step, self.solver)

    def forward_nhwc(self, scs, obs_nhwc):
        """obs_nhwc: [n_obs, B, H, W, C] observations in time order; scs: Schedule or list of B
        Schedules.  Returns (final latent state [B, h, w, C], decoded predictions [n_T, B, H', W', C])."""
        n_obs, B, H, W, C = obs_nhwc.shape
        hx = self.srvp_encoder.forward_nhwc(obs_nhwc.reshape(n_obs * B, H, W, C))
        hx = hx.view(n_obs, B, *hx.shape[1:])
        states, final = self.rollout_nhwc(hx, scs)
        n_T = states.shape[0]
        x = self.srvp_decoder.forward_nhwc(states.reshape(n_T * B, *states.shape[2:]))
        return final, x.view(n_T, B, *x.shape[1:])

    def forward(self, times, input, obs, delta_t, T, return_path=True):
        """(:479-627) times: 1-D float64 observation times (sorted), input: (1,1,C,H,W) (only its shape
        matters: the reference's encoding of it is overwritten before use), obs:
        (1,n_obs,C,H,W), T: 1-D float64 target times.  Returns (state, 0, x) as the reference does."""
        runtime.require_cuda(obs)
        if obs.shape[0] != 1:
            raise NotImplementedError("one sample per call (as the reference); FuturePredictionODE batches samples")
        sc = self.make_schedule(times, delta_t, T)
        final, x = self.forward_nhwc(sc, runtime.to_nhwc(obs[0])[:, None])
        return runtime.to_nchw(final), 0, runtime.to_nchw(x[:, 0])[None]
