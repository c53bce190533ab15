"""Shared helpers of the single-layer sparse (gather) convolution tests (test_sparse_conv_util.py on the CPU, test_gpu_sparse_conv.py on
the GPU): a float64 reference of one layer of ``sf_sparse_conv_masked_fwd``, its derived forward-error bound, synthetic neighbour
tables with the edges a gather kernel can get wrong, the list of cases, and the launcher that names the kernels a call ran on.

    out[j] = act(scale * sum_t W_t^T . feats[nbr[j, t]] + bias) + add          (after: act(... + add))

Everything here is a pure function of fixed names (workloads.hashfill): the same tables and values on every run and machine.  The
references are cached per case and must not be written to."""
import ctypes
import functools
from collections import namedtuple

import numpy as np
import torch

from util import hashfill

U = 2.0 ** -24            # unit roundoff of fp32
GUARD = 64                # sentinel rows in front of and behind the output
SENTINEL = -7777.0
SLACK = 8                 # poisoned channels behind the c0 real ones of every feature row


# ---- reference and bound ------------------------------------------------------------------------------------------------------------
def _taps(feats, nbr, w):
    """sum_t W_t^T . feats[nbr[:, t]] in float64; feats [n_in, c0], nbr [n_out, ntaps] (-1 = nothing), w [ntaps, c0, cout]"""
    f, w = np.asarray(feats, np.float64), np.asarray(w, np.float64)
    nbr = np.asarray(nbr)
    assert nbr.shape[1] == w.shape[0] and f.shape[1] == w.shape[1]
    out = np.zeros((nbr.shape[0], w.shape[2]), np.float64)
    for t in range(nbr.shape[1]):
        idx = nbr[:, t]
        m = idx >= 0
        if m.any():
            out[m] += f[idx[m]] @ w[t]
    return out


def reference(feats, nbr, w, scale, bias, act, add, after):
    """float64 [n_out, cout]; act is 'relu' or 'none'; add None or [n_out, cout]; after: the residual goes in before the activation"""
    assert act in ("relu", "none")
    f = (lambda v: np.maximum(v, 0.0)) if act == "relu" else (lambda v: v)
    y = _taps(feats, nbr, w) * np.asarray(scale, np.float64) + np.asarray(bias, np.float64)
    if add is None:
        return f(y)
    a = np.asarray(add, np.float64)
    return f(y + a) if after else f(y) + a


def bound(feats, nbr, w, scale, bias, add):
    """Per-element forward-error bound of an fp32 evaluation, float64 [n_out, cout]:
        B[j, o] = |scale_o| * sum_t sum_c |W_t[c, o]| * |feats[nbr[j, t], c]| + |bias_o| + |add[j, o]|
        tol     = (K + 4) * 2^-24 * B,      K = ntaps * c0 products
    the classical bound of a K-term fp32 sum accumulated in ANY order (each partial sum rounds once: K u sum|terms| to first order), plus
    one rounding each for a scale folded into the weights, the scale, the bias and the residual.  ReLU is 1-Lipschitz and keeps it."""
    B = _taps(np.abs(np.asarray(feats, np.float64)), nbr, np.abs(np.asarray(w, np.float64))) * np.abs(np.asarray(scale, np.float64))
    B = B + np.abs(np.asarray(bias, np.float64))
    if add is not None:
        B = B + np.abs(np.asarray(add, np.float64))
    K = np.asarray(nbr).shape[1] * np.asarray(w).shape[1]
    return (K + 4) * U * B


# ---- neighbour tables -----------------------------------------------------------------------------------------------------------------
def special_rows(n_out):
    """(rows whose taps are all -1, rows whose taps all read one input row, rows with entries pinned to input rows 0 and n_in - 1) —
    the last row of the (ragged) last tile is empty, its neighbour is pinned; a one-row table has room for the pins only"""
    if n_out < 8:
        return [], [], [0]
    return [n_out // 2, n_out - 1], [0, n_out - 3], [2, n_out - 2]


def table(name, n_out, n_in, ntaps, empty=0.35, empty_rows=None, same_rows=None, pin_rows=None):
    """int32 [n_out, ntaps] with entries in [-1, n_in): hashed rows, a share `empty` of -1 entries, then the special rows"""
    d_empty, d_same, d_pin = special_rows(n_out)
    empty_rows = d_empty if empty_rows is None else empty_rows
    same_rows = d_same if same_rows is None else same_rows
    pin_rows = d_pin if pin_rows is None else pin_rows
    u = hashfill.uniform01(name + "#row", n_out * ntaps, 5).reshape(n_out, ntaps)
    v = hashfill.uniform01(name + "#live", n_out * ntaps, 6).reshape(n_out, ntaps)
    nbr = np.minimum((u * n_in).astype(np.int64), n_in - 1)
    nbr[v < empty] = -1
    for r in same_rows:
        nbr[r, :] = (r * 7 + 3) % n_in
    for r in pin_rows:
        nbr[r, 0] = 0
        nbr[r, ntaps - 1] = n_in - 1
    for r in empty_rows:
        nbr[r, :] = -1
    assert nbr.min() >= -1 and nbr.max() < n_in
    return nbr.astype(np.int32)


def group_live_sets(kind, n_out, ntaps):
    """per 64-row group the taps its rows may read, bool [groups, ntaps]:
    'rotate'   group g lacks tap (0, 2, 1)[g % 3]                      (3 taps)
    'hashed'   hashed subsets: groups that lack tap 0, tap ntaps - 1, a run of consecutive taps, all taps but one, none, or every tap
    'parity'   even groups keep the even taps, odd groups the odd ones: the two groups of a 128-row tile have disjoint live sets"""
    groups = (n_out + 63) // 64
    live = np.ones((groups, ntaps), bool)
    g = np.arange(groups)
    if kind == "rotate":
        live[g, np.array([0, 2, 1])[g % 3] % ntaps] = False
    elif kind == "parity":
        live[:] = (np.arange(ntaps)[None, :] % 2) == (g[:, None] % 2)
    else:
        assert kind == "hashed"
        u = hashfill.uniform01("sc_groups", groups * 4, ntaps).reshape(groups, 4)
        for i in range(groups):
            k = i % 8 if i < 8 else int(u[i, 0] * 8)      # the first eight groups show every pattern once
            if k == 0:
                live[i, 0] = False
            elif k == 1:
                live[i, ntaps - 1] = False
            elif k == 2:
                a = int(u[i, 1] * ntaps)
                live[i, a:a + 1 + int(u[i, 2] * (ntaps - 1))] = False
                if not live[i].any():
                    live[i, 0] = True
            elif k == 3:                                  # one tap only: the first, the last or a hashed one
                live[i] = False
                live[i, (0, ntaps - 1, int(u[i, 1] * ntaps))[int(u[i, 2] * 3)]] = True
            elif k == 4:
                live[i] = hashfill.uniform01(f"sc_subset_{i}", ntaps, 1) < 0.5
                live[i, int(u[i, 1] * ntaps)] = True
            elif k == 5:
                live[i] = False                           # no site of the group has a neighbour: mask word 0
            elif k == 6:
                live[i, 0] = live[i, ntaps - 1] = False
    return live


def masked_table(name, n_out, n_in, ntaps, kind):
    """a table whose 64-row groups differ in their live taps (group_live_sets); inside the live taps 15 % of the entries are -1"""
    nbr = table(name, n_out, n_in, ntaps, empty=0.15)
    live = group_live_sets(kind, n_out, ntaps)
    nbr[~np.repeat(live, 64, 0)[:n_out]] = -1
    return nbr


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
# add: None, 'pre' (residual before the activation: act(y + add)) or 'post' (act(y) + add); table: 'plain' or a group_live_sets kind
Case = namedtuple("Case", "name ntaps n_out n_in c0 cout act add table")

SPLITK = "conv_igemm<T64x64splitK,affine>"
DMA64 = "conv_glds<64x64,affine>"              # (_lib.KERNEL_NAMES drops the "dma" of the tile configuration's name)
DMA64X128 = "conv_glds<64x128w8,affine>"
DMA128 = "conv_glds<128x128w8,affine>"


def _c(ntaps, n_out, n_in, c0, cout, act, add, table="plain"):
    return Case(f"t{ntaps}_n{n_out}_in{n_in}_c{c0}x{cout}_{act}_{add or 'noadd'}" + ("" if table == "plain" else "_" + table),
                ntaps, n_out, n_in, c0, cout, act, add, table)


# register-staged split-K (fewer than 1300 tiles of 64 rows and 27 >= 8 chunks of K; nsplit = 9 .. 16 at these sizes)
SPLIT_CASES = [
    _c(27, 1, 37, 8, 16, "none", None),
    _c(27, 1, 1, 16, 16, "relu", "post"),
    _c(27, 63, 37, 16, 32, "none", "pre"),
    _c(27, 64, 64, 8, 16, "relu", None),
    _c(27, 65, 1, 48, 64, "none", "post"),
    _c(27, 65, 65, 64, 128, "relu", "pre"),
    _c(27, 200, 37, 16, 16, "none", "post"),
    _c(27, 200, 200, 48, 64, "relu", None),
    _c(27, 200, 200, 16, 32, "none", "pre"),
    _c(27, 1000, 37, 64, 128, "none", "pre"),
    _c(27, 1000, 1000, 16, 32, "relu", "post"),
    _c(27, 1000, 1, 8, 16, "none", None),
    _c(27, 63, 63, 64, 128, "relu", "post"),
]
# 782 tiles: still below the 1300 of the mid-size rule, but the workgroup budget gives every tile one K slice (nsplit == 1)
COLLAPSED_CASES = [_c(27, 50003, 4099, 16, 32, "relu", "pre")]
# unsplit LDS-DMA kernel on 64-row tiles: 3 taps (6 chunks at most: conv_out's shape), or 27 taps from 1300 tiles on (ragged last tile)
DMA64_CASES = [
    _c(3, 1, 1, 32, 16, "none", None),
    _c(3, 65, 37, 32, 16, "relu", "post"),
    _c(3, 200, 200, 32, 16, "none", "pre"),
    _c(3, 1, 37, 64, 64, "relu", "pre"),
    _c(3, 65, 65, 64, 64, "none", None),
    _c(3, 200, 37, 64, 64, "none", "post"),
    _c(27, 83237, 4099, 16, 16, "none", "post"),
    _c(27, 83237, 4099, 16, 64, "relu", "pre"),
]
DMA64X128_CASES = [_c(27, 131109, 4099, 16, 64, "none", "pre")]
DMA128_CASES = [_c(3, 131109, 4099, 32, 128, "relu", "post")]
KERNEL_OF = {c: k for cs, k in ((SPLIT_CASES, SPLITK), (COLLAPSED_CASES, SPLITK), (DMA64_CASES, DMA64), (DMA64X128_CASES, DMA64X128),
                                (DMA128_CASES, DMA128)) for c in cs}
PLAIN_CASES = list(KERNEL_OF)
SMALLEST, LARGEST = SPLIT_CASES[0], DMA64X128_CASES[0]

# tap-mask cases (the walk runs in the unsplit LDS-DMA kernels only)
MASK_CASES = [
    (_c(3, 200, 200, 64, 64, "none", "post", "rotate"), DMA64),
    (_c(27, 83237, 4099, 16, 64, "none", "pre", "hashed"), DMA64),
    (_c(27, 83237, 4099, 64, 64, "relu", None, "hashed"), DMA64),
    (_c(27, 131109, 4099, 16, 64, "relu", "post", "parity"), DMA64X128),
]
MASK_SPLIT_CASE = _c(27, 1000, 200, 16, 32, "none", None, "hashed")


@functools.lru_cache(maxsize=None)
def inputs(case):
    """dict(feats [n_in, c0], nbr [n_out, ntaps], w [ntaps, c0, cout], scale, bias, add or None) of float32 / int32 numpy arrays"""
    c = case
    n = c.name
    w = hashfill.uniform("sc_w_" + n, (c.ntaps, c.c0, c.cout), -1, 1, 3).numpy() * np.float32((3.0 / (c.c0 * c.ntaps)) ** 0.5)
    d = dict(feats=hashfill.normal("sc_x_" + n, (c.n_in, c.c0), 1).numpy(), w=w.astype(np.float32),
             scale=hashfill.uniform("sc_s_" + n, (c.cout,), 0.5, 1.5, 5).numpy(), bias=hashfill.uniform("sc_b_" + n, (c.cout,), -0.5, 0.5, 4).numpy(),
             add=hashfill.normal("sc_a_" + n, (c.n_out, c.cout), 6).numpy() if c.add else None,
             nbr=table("sc_t_" + n, c.n_out, c.n_in, c.ntaps) if c.table == "plain" else masked_table("sc_t_" + n, c.n_out, c.n_in, c.ntaps, c.table))
    for v in d.values():
        if v is not None:
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def expected(case):
    """(reference, tol) of a case, float64, computed once"""
    d = inputs(case)
    ref = reference(d["feats"], d["nbr"], d["w"], d["scale"], d["bias"], case.act, d["add"], case.add == "pre")
    tol = bound(d["feats"], d["nbr"], d["w"], d["scale"], d["bias"], d["add"])
    ref.setflags(write=False)
    tol.setflags(write=False)
    return ref, tol


def empty_row_values(case, rows):
    """what a row without any neighbour must hold, in fp32 arithmetic (one rounding of the residual add): act(bias) + add / act(bias + add)"""
    d = inputs(case)
    f = (lambda v: np.maximum(v, np.float32(0))) if case.act == "relu" else (lambda v: v)
    b = np.broadcast_to(d["bias"], (len(rows), case.cout)).astype(np.float32)
    if d["add"] is None:
        return f(b)
    a = d["add"][rows]
    return f(b + a) if case.add == "pre" else f(b) + a


# ---- the device call --------------------------------------------------------------------------------------------------------------------
def profiled(fn):
    """run fn() under the library profiler: (result, names of the kernels that ran)"""
    from streamingflow_amd import _lib
    L = _lib.lib()
    NK = _lib.SF_PROF_KEYS
    calls, ms = (ctypes.c_int32 * NK)(), (ctypes.c_double * NK)()
    fl, by = (ctypes.c_double * NK)(), (ctypes.c_double * NK)()
    L.sf_prof_enable(1)
    try:
        r = fn()
        torch.cuda.synchronize()
        L.sf_prof_collect(calls, ms, fl, by)
    finally:
        L.sf_prof_enable(0)
    return r, [_lib.KERNEL_NAMES[k] for k in range(NK) if calls[k]]


def pack(w, scale, bias, act):
    """w [ntaps, c0, cout] packed as SparseEncoder._pack packs a layer: [cout, cin, ntaps, 1], fp32 (no bf16x3 copy); (ConvW, its owner)"""
    from streamingflow_amd import packing
    assert packing.math_mode() != "bf16x3"
    pk = packing.Pack({})
    w2 = torch.from_numpy(np.ascontiguousarray(np.transpose(np.asarray(w, np.float32), (2, 1, 0))[..., None])).cuda()
    cw = packing.conv_w(pk, w2, w2.shape[1], 0, _dev(scale), _dev(bias), act, pad=0)
    return cw, pk


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()      # (a copy: the cached inputs are read-only)


def run(case, mask=None, d=None):
    """One sf_sparse_conv_masked_fwd call of a case under the profiler: (out float32 numpy [n_out, cout], kernel names).  The features sit
    in a wider tensor whose slack channels hold finite poison; the output has GUARD sentinel rows on either side, checked here."""
    from streamingflow_amd import _lib, runtime
    d = d or inputs(case)
    c = case
    cw, pk = pack(d["w"], d["scale"], d["bias"], c.act)
    cs = c.c0 + SLACK
    feats = (hashfill.normal("sc_poison_" + c.name, (c.n_in, cs), 9) * 1e3).cuda()
    feats[:, :c.c0] = _dev(d["feats"])
    nbr = _dev(d["nbr"])
    add = _dev(d["add"]) if d["add"] is not None else None
    buf = torch.full((c.n_out + 2 * GUARD, c.cout), SENTINEL, dtype=torch.float32, device="cuda")
    out = buf[GUARD:GUARD + c.n_out]
    L = _lib.lib()
    ws = runtime.workspace(L.sf_conv2d_ex_ws_bytes(), "cuda")

    def call():
        _lib.check(L.sf_sparse_conv_masked_fwd(ctypes.byref(cw), runtime.ptr(feats), cs, c.n_in, runtime.ptr(nbr), runtime.ptr(mask), c.n_out,
                                               runtime.ptr(add), int(c.add == "pre"), runtime.ptr(out), runtime.ptr(ws), ws.numel() * 4,
                                               runtime.stream_ptr()), "sparse_conv")
    _, used = profiled(call)
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + c.n_out:] == SENTINEL).all()), "rows outside the output were written"
    del pk
    return out.cpu().numpy(), used
