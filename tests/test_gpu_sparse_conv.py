"""GPU: one layer of the sparse (gather) convolution, sf_sparse_conv_masked_fwd, against a float64 reference on every kernel form the
dispatch sends a neighbour table to (csrc/dispatch.hip: tiled_plan / tiled_split / tiled_glds) — the register-staged split-K kernel with
several K slices and with one, the LDS-DMA kernel on 64-row tiles (narrow and 64-row weight tiles), on 64 x 128 and on 128 x 128 tiles —,
the tap-mask walk of the unsplit LDS-DMA kernels, the argument checks, sf_sparse_to_dense_fwd, and the failure paths and the 32-bit key
ceiling of the index entry points.  Every value case asserts |got - ref| <= tol elementwise with the DERIVED bound of
sparse_conv_util.bound, prints the largest |got - ref| / tol, and asserts the kernel the library's profiler saw."""
import ctypes

import numpy as np
import pytest
import torch

import sparse_conv_util as SC
from oracle import sparse_encoder_ref as SR
from streamingflow_amd._lib import SF_ERR_INVALID, SF_ERR_WORKSPACE

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the MI355X")]


def _check_values(case, got, what=""):
    ref, tol = SC.expected(case)
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float((err / np.maximum(tol, 1e-300)).max())
    print(f"{case.name}{what}: max |got - ref| / tol = {ratio:.4f}   (max |err| {err.max():.3e}, max |ref| {np.abs(ref).max():.3f})")
    assert np.isfinite(got).all()
    bad = np.argwhere(err > tol)
    assert bad.shape[0] == 0, (case.name, bad.shape[0], bad[:8].tolist(), ratio)
    return ratio


def _differing(a, b):
    """number of elements of two float32 arrays that differ in any bit"""
    return int((a.view(np.int32) != b.view(np.int32)).sum())


def _check_empty_rows(case, got):
    """rows without a neighbour hold act(bias) (+ add) exactly"""
    rows = np.nonzero((SC.inputs(case)["nbr"] < 0).all(1))[0]
    want = SC.empty_row_values(case, rows)
    assert _differing(got[rows], want.astype(np.float32)) == 0, case.name
    return len(rows)


@pytest.mark.parametrize("case", SC.PLAIN_CASES, ids=lambda c: c.name)
def test_one_layer_against_float64(case):
    got, used = SC.run(case)
    print(f"{case.name}: ran on {used}")
    assert used == [SC.KERNEL_OF[case]], (case.name, used)
    _check_values(case, got)
    n_empty = _check_empty_rows(case, got)
    assert n_empty >= 2 or case.n_out < 8


# ---- tap masks ------------------------------------------------------------------------------------------------------------------------
def _tile_mask(case):
    from streamingflow_amd.models.sparse_encoder import SparseEncoder
    m = SparseEncoder._tile_mask(SC._dev(SC.inputs(case)["nbr"]), case.n_out)
    assert m.dtype == torch.int32 and m.numel() == (case.n_out + 63) // 64
    return m


@pytest.mark.parametrize("case,kernel", SC.MASK_CASES, ids=lambda v: v.name if isinstance(v, SC.Case) else None)
def test_tap_mask_walk(case, kernel):
    """The true liveness per 64 rows as the mask: the kernel then walks the live taps of each pixel tile only (nsplit == 1: the unsplit
    LDS-DMA kernels), and the result is the unmasked one bit for bit — a cursor that skipped a live tap, stopped early, or paired a tap's
    pixels with another tap's weights would change it."""
    mask = _tile_mask(case)
    full = (1 << case.ntaps) - 1
    words = mask.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    live = SC.group_live_sets(case.table, case.n_out, case.ntaps)
    assert np.array_equal(words[:-1], (live[:-1] * (1 << np.arange(case.ntaps))).sum(1))      # the groups are what the case describes
    assert len(set(words.tolist())) >= 2 and (words != full).mean() > 0.5
    if case.table == "parity":
        assert not (words[0:-1:2] & words[1::2][: len(words[0:-1:2])]).any()                  # the two halves of a 128-row tile share no tap
    plain, used = SC.run(case)
    assert used == [kernel], used
    masked, used_m = SC.run(case, mask)
    print(f"{case.name}: masked and unmasked ran on {used_m}; {len(set(words.tolist()))} different mask words, "
          f"{int(live.sum())} of {live.size} (group, tap) pairs live")
    assert used_m == [kernel], used_m
    assert _differing(masked, plain) == 0
    _check_values(case, masked, " (masked)")
    _check_empty_rows(case, masked)
    ones, _ = SC.run(case, torch.full_like(mask, full))
    assert _differing(ones, plain) == 0
    high, _ = SC.run(case, mask | torch.tensor(-(1 << 27), dtype=torch.int32, device="cuda"))      # bits 27 .. 31 set
    assert _differing(high, plain) == 0


def test_tap_mask_is_ignored_by_the_split_k_launch():
    case = SC.MASK_SPLIT_CASE
    plain, used = SC.run(case)
    masked, used_m = SC.run(case, _tile_mask(case))
    print(f"{case.name}: ran on {used_m}")
    assert used == [SC.SPLITK] and used_m == [SC.SPLITK]
    assert _differing(masked, plain) == 0
    _check_values(case, masked, " (masked)")


# ---- arguments ------------------------------------------------------------------------------------------------------------------------
def test_sparse_conv_arguments():
    from streamingflow_amd import _lib, runtime
    L = _lib.lib()
    c0, cout, ntaps, n_in, n_out, cs = 16, 16, 27, 5, 9, 24
    case = SC._c(ntaps, n_out, n_in, c0, cout, "none", None)
    d = SC.inputs(case)
    cw, pk = SC.pack(d["w"], d["scale"], d["bias"], "none")
    feats = torch.zeros((n_in, cs), device="cuda")
    nbr = SC._dev(d["nbr"])
    out = torch.full((n_out, cout), SC.SENTINEL, device="cuda")
    ws = runtime.workspace(L.sf_conv2d_ex_ws_bytes(), "cuda")
    P = runtime.ptr

    def call(w=cw, feats=P(feats), cs=cs, n_in=n_in, nbr=P(nbr), n_out=n_out, out=P(out)):
        return L.sf_sparse_conv_masked_fwd(ctypes.byref(w), feats, cs, n_in, nbr, None, n_out, None, 0, out, P(ws), ws.numel() * 4, runtime.stream_ptr())

    def edited(**kw):
        w = _lib.ConvW.from_buffer_copy(cw)
        for k, v in kw.items():
            setattr(w, k, v)
        return w
    null = ctypes.c_void_p(0)
    assert call(w=edited(kw=3)) == SF_ERR_INVALID
    assert call(w=edited(c1=4)) == SF_ERR_INVALID
    assert call(cs=c0 - 4) == SF_ERR_INVALID
    assert call(cs=cs + 2) == SF_ERR_INVALID
    assert call(n_in=0) == SF_ERR_INVALID
    assert call(n_out=-1) == SF_ERR_INVALID
    assert call(feats=null) == SF_ERR_INVALID and call(nbr=null) == SF_ERR_INVALID and call(out=null) == SF_ERR_INVALID
    assert call(n_out=0) == 0
    torch.cuda.synchronize()
    assert bool((out == SC.SENTINEL).all())      # nothing was written by any of them
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out != SC.SENTINEL).all())
    del pk


# ---- sf_sparse_to_dense_fwd -----------------------------------------------------------------------------------------------------------
def _to_dense(feats, coords, n, C, B, X, Y, D, out):
    from streamingflow_amd import _lib, runtime
    P = runtime.ptr
    return _lib.lib().sf_sparse_to_dense_fwd(P(feats), P(coords), n, C, B, X, Y, D, P(out), runtime.stream_ptr())


@pytest.mark.parametrize("D", [1, 4, 41])
@pytest.mark.parametrize("C", [1, 3, 16, 130])
def test_sparse_to_dense(C, D):
    """out[b][x][y][c * D + z] = feats[row][c], zero elsewhere — exact, over poison, for no site, one site, a hashed subset that holds the
    corners of the grid and of the last batch, and every cell occupied (rows in a hashed order)."""
    from util import hashfill
    B, X, Y = 2, 5, 3
    cells = np.array([(b, x, y, z) for b in range(B) for x in range(X) for y in range(Y) for z in range(D)], np.int32)
    corners = [(b, x, y, z) for b in (0, B - 1) for x in (0, X - 1) for y in (0, Y - 1) for z in (0, D - 1)]
    order = np.argsort(hashfill.uniform01(f"sd_order_{C}_{D}", len(cells), 1), kind="stable")
    subset = np.unique(np.array(corners + cells[order[: len(cells) // 3]].tolist(), np.int32), axis=0)
    subset = subset[np.argsort(hashfill.uniform01(f"sd_sub_{C}_{D}", len(subset), 2), kind="stable")]
    for coords in (cells[:0], np.array([[B - 1, X - 1, Y - 1, D - 1]], np.int32), subset, cells[order]):
        n = coords.shape[0]
        feats = hashfill.normal(f"sd_x_{C}_{D}_{n}", (max(n, 1), C), 3).numpy()[:n]
        want = np.zeros((B, X, Y, C, D), np.float32)
        want[coords[:, 0], coords[:, 1], coords[:, 2], :, coords[:, 3]] = feats
        out = torch.full((B, X, Y, C * D), float("nan"), device="cuda")
        fd = torch.from_numpy(np.ascontiguousarray(feats)).cuda() if n else None
        cd = torch.from_numpy(np.ascontiguousarray(coords)).cuda() if n else None
        assert _to_dense(fd, cd, n, C, B, X, Y, D, out) == 0
        assert np.array_equal(out.cpu().numpy().view(np.int32), want.reshape(B, X, Y, C * D).view(np.int32)), (C, D, n)


def test_sparse_to_dense_arguments():
    out = torch.full((2, 5, 3, 8), SC.SENTINEL, device="cuda")
    feats, coords = torch.ones((1, 2), device="cuda"), torch.zeros((1, 4), dtype=torch.int32, device="cuda")
    for bad in (dict(B=0), dict(X=0), dict(Y=0), dict(D=0), dict(C=0), dict(n=-1), dict(out=None), dict(feats=None), dict(coords=None), dict(X=-5)):
        a = dict(feats=feats, coords=coords, n=1, C=2, B=2, X=5, Y=3, D=4, out=out)
        a.update(bad)
        assert _to_dense(**a) == SF_ERR_INVALID, bad
    torch.cuda.synchronize()


# ---- index entry points -----------------------------------------------------------------------------------------------------------------
def _i3(v):
    return (ctypes.c_int32 * 3)(*[int(x) for x in v])


def _sites(n, shape, B, name):
    from util import hashfill
    total = B * shape[0] * shape[1] * shape[2]
    cells = np.argsort(hashfill.uniform01(name, total, 4), kind="stable")[:n]
    z, y, x, b = cells % shape[2], (cells // shape[2]) % shape[1], (cells // (shape[2] * shape[1])) % shape[0], cells // (shape[0] * shape[1] * shape[2])
    return np.stack([b, x, y, z], 1).astype(np.int32)


def _out_sites_raw(coords, B, shape, k, s, p, cap, ws_bytes=None, guard=8):
    """(status, count, rows buffer [cap + guard, 4] pre-filled with -9)"""
    from streamingflow_amd import _lib, runtime
    L = _lib.lib()
    n_in, ntaps = coords.shape[0], k[0] * k[1] * k[2]
    cd = torch.from_numpy(coords).cuda()
    out = torch.full((cap + guard, 4), -9, dtype=torch.int32, device="cuda")
    cnt = torch.full((), -9, dtype=torch.int32, device="cuda")
    need = L.sf_sparse_index_ws_bytes(n_in, ntaps)
    ws = torch.empty(need // 4 + 64, dtype=torch.float32, device="cuda")
    rc = L.sf_sparse_out_sites_fwd(runtime.ptr(cd), n_in, B, _i3(shape), _i3(k), _i3(s), _i3(p), runtime.ptr(out), cap, runtime.ptr(cnt), runtime.ptr(ws),
                                   need if ws_bytes is None else ws_bytes, runtime.stream_ptr())
    torch.cuda.synchronize()
    return rc, int(cnt.item()), out.cpu().numpy()


def _table_raw(coords, out_coords, B, shape, k, s, p, subm, ws_bytes=None):
    from streamingflow_amd import _lib, runtime
    L = _lib.lib()
    n_in, n_out, ntaps = coords.shape[0], out_coords.shape[0], k[0] * k[1] * k[2]
    cd, od = torch.from_numpy(coords).cuda(), torch.from_numpy(out_coords).cuda()
    nbr = torch.full((n_out, ntaps), -9, dtype=torch.int32, device="cuda")
    need = L.sf_sparse_index_ws_bytes(n_in, ntaps)
    ws = torch.empty(need // 4 + 64, dtype=torch.float32, device="cuda")
    rc = L.sf_sparse_table_fwd(runtime.ptr(cd), n_in, runtime.ptr(od), n_out, B, _i3(shape), _i3(k), _i3(s), _i3(p), int(subm), runtime.ptr(nbr),
                               runtime.ptr(ws), need if ws_bytes is None else ws_bytes, runtime.stream_ptr())
    torch.cuda.synchronize()
    return rc, nbr.cpu().numpy()


def test_out_sites_with_a_capacity_below_the_count():
    shape, B, k, s, p = [21, 16, 11], 2, [3, 3, 3], [2, 2, 2], [1, 1, 1]
    coords = _sites(300, shape, B, "si_cap")
    want, _ = SR.down_sites(coords, shape, k, s, p)
    true = want.shape[0]
    assert true > 300
    for cap in (1, true // 2, true - 1, true):
        rc, cnt, rows = _out_sites_raw(coords, B, shape, k, s, p, cap)
        assert rc == 0 and cnt == true, (cap, rc, cnt, true)
        assert np.array_equal(rows[:cap], want[:cap]) and (rows[cap:] == -9).all(), cap


def test_index_workspace_one_byte_short():
    from streamingflow_amd import _lib
    L = _lib.lib()
    assert L.sf_sparse_index_ws_bytes(0, 27) == 0
    shape, B, k, s, p = [21, 16, 11], 1, [3, 3, 3], [2, 2, 2], [1, 1, 1]
    coords = _sites(40, shape, B, "si_ws")
    need = L.sf_sparse_index_ws_bytes(40, 27)
    assert need > 0
    rc, cnt, rows = _out_sites_raw(coords, B, shape, k, s, p, 64, ws_bytes=need - 1)
    assert rc == SF_ERR_WORKSPACE and cnt == -9 and (rows == -9).all()
    rc, nbr = _table_raw(coords, coords, B, shape, k, s, p, True, ws_bytes=need - 1)
    assert rc == SF_ERR_WORKSPACE and (nbr == -9).all()
    rc, nbr = _table_raw(coords, coords, B, shape, k, s, p, True, ws_bytes=need)      # exactly that size is enough
    assert rc == 0 and np.array_equal(nbr, SR.neighbour_table(coords, shape, coords, k, s, p, True).astype(np.int32))
    want, _ = SR.down_sites(coords, shape, k, s, p)
    rc, cnt, rows = _out_sites_raw(coords, B, shape, k, s, p, want.shape[0], ws_bytes=need)
    assert rc == 0 and cnt == want.shape[0] and np.array_equal(rows[:cnt], want)


def test_index_keys_just_under_the_32_bit_ceiling():
    """A grid of 1600 x 1600 x 1677 = 4 293 120 000 cells: the largest keys sit next to the 0xFFFFFFFF sentinel of the candidate sort
    and past 2^31 (a signed key would sort them first).  One more z plane is refused."""
    shape, k3 = [1600, 1600, 1677], [3, 3, 3]
    assert shape[0] * shape[1] * shape[2] == 4293120000 < 0xFFFFFFFF
    coords = np.array([[0, 1599, 1599, 1676], [0, 0, 0, 0], [0, 1599, 1599, 1675], [0, 1598, 1599, 1676], [0, 1599, 1598, 1675], [0, 0, 0, 1], [0, 1, 0, 0],
                       [0, 800, 800, 838], [0, 801, 800, 838], [0, 800, 801, 839], [0, 799, 799, 837], [0, 1599, 0, 1676], [0, 0, 1599, 0]], np.int32)
    rc, tab = _table_raw(coords, coords, 1, shape, k3, [1, 1, 1], [0, 0, 0], True)
    want = SR.neighbour_table(coords, shape, coords, k3, [1, 1, 1], [0, 0, 0], True)
    assert rc == 0 and np.array_equal(tab, want.astype(np.int32))
    assert (want >= 0).sum(1).min() >= 1 and (want >= 0).sum() >= coords.shape[0] + 12      # every site finds itself, neighbours find each other
    s, p = [2, 2, 2], [1, 1, 1]
    wc, wso = SR.down_sites(coords, shape, k3, s, p)
    rc, cnt, rows = _out_sites_raw(coords, 1, shape, k3, s, p, coords.shape[0] * 27)
    assert rc == 0 and cnt == wc.shape[0] and np.array_equal(rows[:cnt], wc) and (rows[cnt:] == -9).all()
    rc, tab2 = _table_raw(coords, wc, 1, shape, k3, s, p, False)
    assert rc == 0 and np.array_equal(tab2, SR.neighbour_table(coords, shape, wc, k3, s, p, False).astype(np.int32))
    # a stride-1 strided conv keeps the output grid as large as the input grid: output keys next to the sentinel too
    wc1, _ = SR.down_sites(coords, shape, k3, [1, 1, 1], p)
    rc, cnt, rows = _out_sites_raw(coords, 1, shape, k3, [1, 1, 1], p, coords.shape[0] * 27)
    assert rc == 0 and cnt == wc1.shape[0] and np.array_equal(rows[:cnt], wc1)
    assert wc1[-1].tolist() == [0, 1599, 1599, 1676]
    big = [1600, 1600, 1678]
    small = coords[:2]
    assert _table_raw(small, small, 1, big, k3, [1, 1, 1], [0, 0, 0], True)[0] == SF_ERR_INVALID
    assert _out_sites_raw(small, 1, big, k3, s, p, 64)[0] == SF_ERR_INVALID
