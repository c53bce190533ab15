"""Device plumbing shared by the modules: current HIP stream handle, a grow-only workspace per
device, NCHW<->NHWC conversion through the library, cached packed weights."""
import collections
import ctypes

import torch

from . import _lib

_WORKSPACES = {}


def stream_ptr(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("streamingflow_amd runs on MI355X only: got a %s tensor (no CPU fallback)" % t.device)


def workspace(nbytes, device):
    """Grow-only fp32 scratch buffer per (device, stream) (pointer is stable while it does not grow)."""
    dev = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)     # one scratch per stream: forwards on different streams may overlap
    cur = _WORKSPACES.get(key)
    need = (int(nbytes) + 3) // 4 + 1024
    if cur is None or cur.numel() < need:
        _WORKSPACES[key] = cur = torch.empty(need, dtype=torch.float32, device=torch.device("cuda", dev))
    return cur


def static_workspace(nbytes, device):      # of a captured graph, which keeps the pointer (`workspace` may move when it grows)
    return torch.empty(int(nbytes) // 4 + 1024, dtype=torch.float32, device=device)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def ptr_at(t, chan_offset=0):
    """Pointer `chan_offset` floats into t: channel `chan_offset` of an NHWC tensor (null for None)."""
    return ctypes.c_void_p(t.data_ptr() + 4 * int(chan_offset)) if t is not None else ctypes.c_void_p(0)


def call(fn, *args, device, scratch=None):
    """The library's calling convention, in its one place: a forward ends in ``(..., stream)``, or in
    ``(..., ws, ws_bytes, stream)`` when it takes scratch.  ``fn``: the short name of ``sf_<fn>_fwd``, or the ctypes function itself
    where the caller picks between variants; ``args``: its arguments up to ``ws``.  ``scratch``: None, or the size query
    ``(name, *dims)`` — ``sf_<name>_ws_bytes(*dims)``, often not the forward's own name — answered from ``workspace``, or a tensor
    to use as it is (a captured graph's ``static_workspace``).  Raises on a non-zero status; returns the scratch tensor."""
    L = _lib.lib()
    if isinstance(fn, str):
        fn = getattr(L, "sf_" + fn + "_fwd")
    if scratch is None:
        status = fn(*args, stream_ptr(device))
    else:
        if isinstance(scratch, tuple):
            scratch = workspace(getattr(L, "sf_" + scratch[0] + "_ws_bytes")(*scratch[1:]), device)
        status = fn(*args, ptr(scratch), scratch.numel() * 4, stream_ptr(device))
    if status != 0:      # (the name is looked up on the failing call only)
        _lib.check(status, fn.__name__)
    return scratch


def conv2d_ex(w, in0, in0_cs, in0_co, n, h, wd, out, out_cs, out_co, in1=None, in1_cs=0, in1_co=0, add=None, add_cs=0,
              act_after_add=False):
    """``sf_conv2d_ex_fwd``: packed conv ``w`` on channels in0_co.. of in0 [P][in0_cs] (beside them in1_co.. of in1 [P][in1_cs]) into channels out_co.. of
    out [P][out_cs], P = n * h * wd input pixels; ``add`` [P'][add_cs] joins after the activation, or before it (act_after_add)."""
    call("conv2d_ex", w, ptr_at(in0, in0_co), in0_cs, ptr_at(in1, in1_co), in1_cs, ptr(add), add_cs, int(act_after_add), ptr(out),
         out_cs, out_co, n, h, wd, 0, device=out.device, scratch=("conv2d_ex",))


def image_frontend_plan(Hs, Ws, Hr, Wr, box, mean, std):
    """``sf_image_frontend_plan``: the host blob (int32 words, include/sfnative.h N9) of the front end that resizes Hs x Ws frames to
    Hr x Wr and crops ``box`` = (l, t, r, b): both axes' resample tables and the normalise table.  Host arithmetic only, no GPU."""
    L = _lib.lib()
    nbytes = L.sf_image_frontend_plan_bytes(Hs, Ws, Hr, Wr, *box)
    blob = torch.zeros(max(nbytes // 4, 1), dtype=torch.int32)
    m, s = ((ctypes.c_float * 3)(*[float(v) for v in t]) for t in (mean, std))
    _lib.check(L.sf_image_frontend_plan(Hs, Ws, Hr, Wr, *box, m, s, ctypes.c_void_p(blob.data_ptr()), nbytes), "sf_image_frontend_plan")
    return blob


def image_frontend(src, plan_host, plan_dev, out, planar=True, out_u8=None):
    """``sf_image_frontend_fwd``: src [n][Hs][Ws][3] uint8 -> out fp32 [n][3][h][w] (planar) or [n][h][w][3], and optionally the resized,
    cropped bytes out_u8 [n][h][w][3]; ``plan_host`` from ``image_frontend_plan``, ``plan_dev`` its copy on src's device."""
    n, Hs, Ws = src.shape[:3]
    h, w = (out.shape[2], out.shape[3]) if planar else (out.shape[1], out.shape[2])
    call("image_frontend", ptr(src), ctypes.c_void_p(plan_host.data_ptr()), ptr(plan_dev), ptr(out), int(bool(planar)), ptr(out_u8), n, Hs, Ws,
         h, w, device=src.device)


def require_no_grad(*tensors):
    """Inference only (the reference evaluates under torch.no_grad(), evaluate.py:117): the HIP path records no autograd
    history, so an input that asks for gradients while grad mode is on would silently get none — refuse it instead.
    Parameters with requires_grad=True are fine: calling a module outside no_grad() works and returns detached tensors
    ("Observable differences")."""
    if torch.is_grad_enabled():
        for t in tensors:
            if t is not None and t.requires_grad:
                raise RuntimeError("streamingflow_amd is inference-only: an input has requires_grad=True under enabled grad mode, "
                                   "but the HIP path records no autograd history (detach the input or use torch.no_grad())")


def f32c(t):
    return t.detach().to(torch.float32).contiguous()


def to_nhwc(x):
    """(n, C, H, W) fp32 cuda -> (n, H, W, C) contiguous (libsfnative transpose kernel)."""
    require_cuda(x)
    require_no_grad(x)      # every module entry point converts its NCHW inputs here
    x = f32c(x)
    n, c, h, w = x.shape
    out = torch.empty((n, h, w, c), dtype=torch.float32, device=x.device)
    if out.numel():
        call(_lib.lib().sf_nchw_to_nhwc, ptr(x), ptr(out), n, c, h * w, device=x.device)
    return out


def to_nchw(x):
    """(n, H, W, C) fp32 cuda -> (n, C, H, W) contiguous."""
    require_cuda(x)
    n, h, w, c = x.shape
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    if out.numel():
        call(_lib.lib().sf_nhwc_to_nchw, ptr(x), ptr(out), n, c, h * w, device=x.device)
    return out


def frames_first(y, b):
    """[b * T, h, w, C] (sample-major) -> [T, b, h, w, C] contiguous."""
    return y.view(b, -1, *y.shape[1:]).permute(1, 0, 2, 3, 4).contiguous()


def frames_last(y):
    """[T, b, h, w, C] -> [b * T, h, w, C] (sample-major)."""
    T, b = y.shape[:2]
    return y.permute(1, 0, 2, 3, 4).reshape(b * T, *y.shape[2:])


def frames_to_nhwc(x):
    """[b, T, C, h, w] -> [T, b, h, w, C] contiguous, the layout of the sequence entry points: one transpose launch, one copy."""
    b, T, c, h, w = x.shape
    return frames_first(to_nhwc(x.reshape(b * T, c, h, w)), b)


def frames_to_nchw(y):
    """[T, b, h, w, C] -> [b, T, C, h, w]: the inverse of ``frames_to_nhwc``."""
    T, b, h, w, C = y.shape
    return to_nchw(frames_last(y)).view(b, T, C, h, w)


def frames_to_nchw_strided(y):
    """[T, b, h, w, C] -> [b, T, C, h, w] written in place: one strided transpose launch per frame, no copy."""
    T, b, h, w, C = y.shape
    res = torch.empty((b, T, C, h, w), dtype=torch.float32, device=y.device)
    fn = _lib.lib().sf_nhwc_to_nchw_strided
    for t in range(T):          # frame (t, b) -> res[b, t]
        call(fn, ptr(y[t]), h * w * C, ptr(res[0, t]), T * C * h * w, b, C, h * w, device=y.device)
    return res


_PACK_GENERATION = [0]      # process-wide, monotonically increasing: never reused (unlike id() of a freed Pack)


def strip_runtime_state(d):
    """A module's ``__dict__`` without what only exists on this process's GPU: packed weight copies (ctypes structs full of device
    pointers), folded packs, captured graphs.  ``copy.deepcopy(model)`` and ``torch.save(model)`` go through ``__getstate__``; the
    copy re-packs (and re-captures) on its first forward."""
    d = dict(d)
    for k in [k for k in d if k.startswith("_sf_")] + ["_folded_tail"]:
        d.pop(k, None)
    return d


class PackedModule(torch.nn.Module):
    """Mixin: lazily packs the module's parameters for the HIP library and re-packs when any
    parameter was replaced, moved or modified in place (load_state_dict, .to(), optimiser).
    ``pack_generation()`` identifies the current packed copy for caches that hold raw pointers into it
    (captured hipGraphs): it changes exactly when ``packed()`` returns a new copy and is never reused."""

    def _param_signature(self):
        from . import packing
        sig = [packing.math_mode(), packing.winograd()]
        for t in list(self.parameters()) + list(self.buffers()):
            sig.append((t.data_ptr(), t._version, t.device))
        return tuple(sig)

    def packed(self):
        sig = self._param_signature()
        cache = self.__dict__.get("_sf_pack")
        if cache is None or cache[0] != sig:
            first = next(self.parameters())
            require_cuda(first)
            with torch.no_grad():
                pk = self._pack()
            _PACK_GENERATION[0] += 1
            self.__dict__["_sf_pack"] = cache = (sig, pk, _PACK_GENERATION[0])
        return cache[1]

    def pack_generation(self):
        self.packed()
        return self.__dict__["_sf_pack"][2]

    def _pack(self):
        raise NotImplementedError

    def __getstate__(self):
        return strip_runtime_state(self.__dict__)


class GraphCache(collections.OrderedDict):
    """Captured hipGraphs of one owner, least recently used first: key -> entry, a dict of the static buffers the graph reads and
    writes plus ``"exec"``, its hipGraphExec handle.  The owner decides the keys, the limit and when the entries are stale.  No
    finalizer: handles are destroyed by eviction and by ``drop()`` only."""

    def capture(self, key, entry, enqueue, device, limit):
        """Run ``enqueue()`` eagerly (the real run; it also sets kernel attributes and packs weights), record the same calls on a
        side stream into a graph, and insert the entry.  Nothing is replayed."""
        L = _lib.lib()
        enqueue()
        torch.cuda.synchronize(device)
        with torch.cuda.stream(torch.cuda.Stream(device=device)):
            sp = stream_ptr(device)
            _lib.check(L.sf_graph_begin(sp), "graph_begin")
            try:
                enqueue()
            finally:
                ex = ctypes.c_void_p()
                _lib.check(L.sf_graph_end(sp, ctypes.byref(ex)), "graph_end")
        entry["exec"] = ex
        self.insert(key, entry, limit)

    def insert(self, key, entry, limit):
        entry["key"] = key
        self[key] = entry
        self.drop(limit)

    def replay(self, entry, device):
        """Launch the entry's graph on the current stream; the entry becomes the most recently used."""
        self.move_to_end(entry["key"])
        _lib.check(_lib.lib().sf_graph_launch(entry["exec"], stream_ptr(device)), "graph_launch")

    def drop(self, keep=0):
        """All entries but the ``keep`` most recently used leave: their graphs are destroyed, their buffers released."""
        while len(self) > keep:
            entry = self.popitem(last=False)[1]
            if entry.get("exec") is not None:
                _lib.lib().sf_graph_destroy(entry["exec"])
