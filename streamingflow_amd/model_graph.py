"""``ModelGraphSession`` — ``streamingflow.forward`` as one replayable graph.

``session = net.graphed(max_graphs=4)``; ``session(*args)`` takes exactly ``forward``'s arguments and returns ``forward``'s dict, whose
tensors are the session's static outputs: valid until the session's next call.  For the duration of a call the session turns
``static_lidar`` and ``static_camera`` on (``lidar_capacities`` is honoured) and feeds the rollout's host-built operands through a
``RolloutFeed``; afterwards the model is as it was.

A graph is keyed by the shapes and dtypes of every tensor argument, the per-sample schedule structures and their grouping (built on
the host from the CPU timestamp tensors, as ``forward`` builds them), the noise mode and the device.  The first call of a key runs once
eagerly on the static buffers (that run packs weights and sets kernel attributes), records the forward with ``torch.cuda.graph`` on one
side stream — no forks — and replays; later calls copy the inputs into the static buffers, fill the fed ``coef`` and noise record and
replay.  Nothing in a call reads back from the device: ``check()`` is the one synchronising call.
"""
import collections

import torch

from . import packing, runtime, schedule as sched


def _tensors(tree):
    """The tensors of an argument (a tensor, None, or a list / tuple of those), in order."""
    if torch.is_tensor(tree):
        return [tree]
    if isinstance(tree, (list, tuple)):
        return [t for item in tree for t in _tensors(item)]
    if tree is None:
        return []
    raise TypeError("ModelGraphSession: forward's arguments are tensors, None, or lists / tuples of tensors; got %s" % type(tree).__name__)


def _rebuild(tree, it):
    """`tree` with its tensors replaced by the next ones of `it`."""
    if torch.is_tensor(tree):
        return next(it)
    if isinstance(tree, (list, tuple)):
        return type(tree)(_rebuild(item, it) for item in tree)
    return None


def _shape_key(tree):
    if torch.is_tensor(tree):
        return (tuple(tree.shape), str(tree.dtype))
    if isinstance(tree, (list, tuple)):
        return tuple(_shape_key(item) for item in tree)
    return None


class ModelGraphSession:
    # forward's arguments by position; the timestamps stay on the host (the schedules are built from them)
    ARGS = ("image", "intrinsics", "extrinsics", "future_egomotion", "padded_voxel_points", "camera_timestamp", "points", "lidar_timestamp",
            "target_timestamp")
    HOST = (5, 7, 8)

    def __init__(self, net, max_graphs=4):
        if int(max_graphs) < 1:
            raise ValueError("max_graphs must be at least 1")
        self.net, self.max_graphs = net, int(max_graphs)
        self._graphs = collections.OrderedDict()      # key -> entry, least recently used first
        self._weights = None
        self._clouds = 0
        self.captures = 0      # graphs recorded so far (a call that finds its graph cached adds none)

    def __len__(self):
        return len(self._graphs)

    def drop_graphs(self):
        """Destroy every captured graph of this session and release its static buffers."""
        self._graphs.clear()

    # ---- what is decided on the host, before anything is enqueued -------------------------------------------------------------------------
    def _weight_signature(self):
        """Every graph holds raw pointers into packed weights: identity and version of every parameter and buffer, which is what every
        packed copy of the model (PackedModule and the neck's and the trunk's own caches) is stale by, and the packing switches."""
        sig = [packing.math_mode(), packing.winograd(), packing._FLOW[0]]
        for t in self.net.parameters():
            sig.append((t.data_ptr(), t._version))
        for t in self.net.buffers():
            sig.append((t.data_ptr(), t._version))
        return tuple(sig)

    def _rollouts(self, args):
        """The rollouts `forward` will run, as it groups them (FuturePredictionODE.forward): [(schedules of the group's samples)] in call
        order, and their key — per group its members, structure, observation order and whether the step sizes differ per sample."""
        net = self.net
        if net.n_future <= 0:
            return [], ()
        cam_ts, lid_ts, tgt_ts = (args[i] for i in self.HOST)
        need = [("target_timestamp", tgt_ts)] + ([("camera_timestamp", cam_ts)] if net.use_camera else []) + \
               ([("lidar_timestamp", lid_ts)] if net.use_lidar else [])
        for name, t in need:
            if not torch.is_tensor(t):
                raise ValueError("ModelGraphSession: %s must be a CPU tensor [b, n]" % name)
            if t.is_cuda:
                raise ValueError("ModelGraphSession: %s is on %s: the schedules are built on the host, and reading a device tensor back "
                                 "(.tolist()) would synchronise — pass the timestamps as CPU tensors" % (name, t.device))
        fp = net.future_prediction_ode
        b = tgt_ts.shape[0]
        groups, scs, orders = {}, [], []
        for bs in range(b):
            times, order = sched.merge_observations(cam_ts[bs].tolist() if net.use_camera else [], lid_ts[bs].tolist() if net.use_lidar else [])
            scs.append(fp.gru_ode.make_schedule(times, fp.delta_t, tgt_ts[bs].tolist()))
            orders.append(tuple(order))
            groups.setdefault(scs[-1].key(), []).append(bs)
        MAX_GROUP = 64      # as FuturePredictionODE.forward chunks them
        chunks = [m[i:i + MAX_GROUP] for m in groups.values() for i in range(0, len(m), MAX_GROUP)]
        plan = [[scs[i] for i in members] for members in chunks]
        key = tuple((tuple(members), scs[members[0]].key(), tuple(orders[i] for i in members),
                     len(members) > 1 and any(scs[i].dts != scs[members[0]].dts for i in members)) for members in chunks)
        return plan, key

    def _key(self, args, rollout_key):
        net = self.net
        dev_args = [a for i, a in enumerate(args) if i not in self.HOST]
        tensors = _tensors(dev_args)
        if not tensors:
            raise ValueError("ModelGraphSession: no tensor argument")
        for t in tensors:
            if not t.is_cuda:
                raise RuntimeError("streamingflow_amd runs on MI355X only: got a %s tensor (no CPU fallback)" % t.device)
        ode = net.future_prediction_ode.gru_ode if net.n_future > 0 else None
        noise = (ode._feed_mode(), ode.solver, bool(ode.impute)) if ode is not None else None
        caps = tuple(net.lidar_capacities) if net.use_lidar and net.lidar_capacities is not None else None
        return (tuple(_shape_key(a) for a in dev_args), rollout_key, noise, str(tensors[0].device), caps)

    # ---- the call -------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, *args, **kwargs):
        net = self.net
        args = list(args) + [None] * (len(self.ARGS) - len(args))
        if len(args) > len(self.ARGS):
            raise TypeError("ModelGraphSession takes forward's %d arguments" % len(self.ARGS))
        for k, v in kwargs.items():
            if k not in self.ARGS:
                raise TypeError("ModelGraphSession: forward has no argument %r" % k)
            args[self.ARGS.index(k)] = v
        if net.planning_enabled:
            raise NotImplementedError("ModelGraphSession: the planner (PLANNING.ENABLED) is not recorded into the model graph; "
                                      "call forward, or run Planning on the session's outputs")
        if net.training:
            raise RuntimeError("ModelGraphSession is inference-only: call .eval()")
        if packing.flow_active():
            raise NotImplementedError("ModelGraphSession: the persistent flow kernel checks its result on the host; switch it off")
        plan, rollout_key = self._rollouts(args)
        key = self._key(args, rollout_key)
        weights = self._weight_signature()
        if weights != self._weights:      # load_state_dict, .to(), an in-place update: every graph points into stale packs
            self.drop_graphs()
            self._weights = weights
        entry = self._graphs.get(key)
        if entry is None:
            entry = self._capture(key, args, plan)
            # (the first pass packed the weights: same parameters, so the signature stands)
        else:
            self._graphs.move_to_end(key)
            for dst, src in zip(entry["inputs"], _tensors([a for i, a in enumerate(args) if i not in self.HOST])):
                dst.copy_(src)
            ode = net.future_prediction_ode.gru_ode if plan else None
            for slot, scs in zip(entry["feed"].slots, plan):
                ode.fill_feed_slot(slot, scs)
            entry["graph"].replay()
        if net.use_lidar:
            net.lidar_site_counts = entry["site_counts"]
            self._clouds = sum(int(p.shape[0]) for p in args[6])      # forward voxelises B * T clouds
        return dict(entry["out"])

    def _static_args(self, args, inputs):
        it = iter(inputs)
        return [a if i in self.HOST else _rebuild(a, it) for i, a in enumerate(args)]

    def _capture(self, key, args, plan):
        """First call of a key: one eager pass on the static buffers (the real run: it also packs weights, sets kernel attributes, makes
        and fills the feed's slots), the same calls recorded on one side stream, one replay."""
        from .layers.temporal_ode_bayes import RolloutFeed
        net = self.net
        inputs = [t.clone() for t in _tensors([a for i, a in enumerate(args) if i not in self.HOST])]
        static = self._static_args(args, inputs)
        feed = RolloutFeed()
        ode = net.future_prediction_ode.gru_ode if net.n_future > 0 else None
        saved = (getattr(net, "static_lidar", None), net.static_camera, ode.feed if ode is not None else None)
        try:
            if net.use_lidar:
                net.static_lidar = True
            net.static_camera = True
            if ode is not None:
                ode.feed = feed
            feed.begin()
            net.forward(*static)
            if len(feed.slots) != len(plan):
                raise RuntimeError("ModelGraphSession: forward ran %d rollouts where its grouping gives %d" % (len(feed.slots), len(plan)))
            feed.begin()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = net.forward(*static)
            counts = net.lidar_site_counts if net.use_lidar else None
        finally:
            if net.use_lidar:
                net.static_lidar = saved[0]
            net.static_camera = saved[1]
            if ode is not None:
                ode.feed = saved[2]
        entry = {"graph": graph, "inputs": inputs, "feed": feed, "out": out, "site_counts": counts}
        self._graphs[key] = entry
        self.captures += 1
        while len(self._graphs) > self.max_graphs:
            self._graphs.popitem(last=False)
        graph.replay()
        return entry

    def check(self):
        """The one synchronising call: reads the device counters of the last call back and raises where a strided convolution of the
        LiDAR encoder had more output sites than its capacity (SparseEncoder.check_static) or a camera of the rig was singular or
        non-finite (LiftSplat.check_rig)."""
        net = self.net
        torch.cuda.synchronize()
        if net.use_lidar and net.lidar_site_counts is not None:
            backbone, vox = net.encoders["lidar"]["backbone"], net.encoders["lidar"]["voxelize"]
            caps = net.lidar_capacities
            if caps is None:      # what forward_static took: its defaults for the row buffer voxelize_static makes of the clouds
                clouds = self._clouds
                caps = backbone.default_capacities(clouds * int(vox.max_voxels[0] if vox.training else vox.max_voxels[1]), clouds)
            backbone.check_static(net.lidar_site_counts, caps)
        if net.use_camera:
            net.lift.check_rig()
