"""TEST INFRASTRUCTURE of test_gpu_lidar_static.py: row buffers with inactive rows, and the raw calls of the static index entry points
with guard regions.  Nothing here is product code.

holes(n) places n sites in a buffer so that every shape of dead region occurs at once (rows, 64-row tiles):
  rows    0 ..  36   inactive: the first active block starts at row 37, not a multiple of 64
  rows   37 .. 136   sites 0 .. 99; the hole behind them starts at row 137, in the middle of tile 2
  rows  137 .. 511   inactive: tiles 3 .. 7 are dead as a whole, tiles (4, 5) and (6, 7) are aligned 128-row pairs
  rows  512 ..       sites 100 .. n - 1, then 29 inactive rows (30 where that would end the buffer on a tile edge): the last tile is partial
"""
import ctypes

import numpy as np
import torch

INACTIVE = np.array([-1, -1, -1, -1], np.int32)
FILL = -9


def i3(v):
    return (ctypes.c_int32 * 3)(*[int(x) for x in v])


def holes(n):
    """(rows of the buffer, pos [n]: the row of site i)"""
    assert n > 100
    pos = np.concatenate([37 + np.arange(100), 512 + np.arange(n - 100)])
    cap = 512 + (n - 100) + 29
    if cap % 64 == 0:
        cap += 1
    return cap, pos


def dense_rows(n):
    return n, np.arange(n)


def spread(coords, feats, cap, pos, junk=3.5):
    """the row buffer: sites at their rows, inactive rows elsewhere; the feature rows of inactive sites hold `junk` (anything finite)"""
    c = np.tile(INACTIVE, (cap, 1))
    c[pos] = coords
    f = None
    if feats is not None:
        f = np.full((cap, feats.shape[1]), junk, np.float32)
        f[pos] = feats
    return c, f


def compact_table(tab, pos_in):
    """a table over buffer rows -> the same over compact site numbers (-1 stays)"""
    inv = np.full(int(pos_in.max()) + 2, -7, np.int64)
    inv[pos_in] = np.arange(len(pos_in))
    return np.where(tab >= 0, inv[np.maximum(tab, 0)], -1)


def tile_words(tab):
    """numpy restatement of the tile words: OR over the tile's rows of their live taps (dead tiles: 0 here)"""
    n, taps = tab.shape
    live = np.zeros(((n + 63) // 64 * 64, taps), bool)
    live[:n] = tab >= 0
    return (live.reshape(-1, 64, taps).any(1) * (1 << np.arange(taps, dtype=np.int64))).sum(1)


def _ws(n_in, ntaps):
    from streamingflow_amd import _lib
    need = _lib.lib().sf_sparse_index_ws_bytes(n_in, ntaps)
    return torch.empty(need // 4 + 64, dtype=torch.float32, device="cuda"), need


def out_sites_static(rows, B, shape, k, s, p, cap_out, guard=8):
    """-> (status, device count, buffer [cap_out + guard, 4] pre-filled with FILL)"""
    from streamingflow_amd import _lib, runtime
    cd = torch.from_numpy(rows).cuda()
    out = torch.full((cap_out + guard, 4), FILL, dtype=torch.int32, device="cuda")
    cnt = torch.full((), FILL, dtype=torch.int32, device="cuda")
    ws, need = _ws(rows.shape[0], k[0] * k[1] * k[2])
    rc = _lib.lib().sf_sparse_out_sites_static_fwd(runtime.ptr(cd), rows.shape[0], B, i3(shape), i3(k), i3(s), i3(p), runtime.ptr(out), cap_out,
                                                   runtime.ptr(cnt), runtime.ptr(ws), need, runtime.stream_ptr())
    torch.cuda.synchronize()
    return rc, int(cnt.item()), out.cpu().numpy()


def table_static(rows_in, rows_out, B, shape, k, s, p, subm, guard=4):
    """-> (status, table [cap_out, ntaps], words [tiles], the guard rows behind the table, the guard words behind the words)"""
    from streamingflow_amd import _lib, runtime
    cd, od = torch.from_numpy(rows_in).cuda(), torch.from_numpy(rows_out).cuda()
    n_out, ntaps = rows_out.shape[0], k[0] * k[1] * k[2]
    tiles = (n_out + 63) // 64
    nbr = torch.full((n_out + guard, ntaps), FILL, dtype=torch.int32, device="cuda")
    words = torch.full((tiles + guard,), FILL, dtype=torch.int32, device="cuda")
    ws, need = _ws(rows_in.shape[0], ntaps)
    rc = _lib.lib().sf_sparse_table_static_fwd(runtime.ptr(cd), rows_in.shape[0], runtime.ptr(od), n_out, B, i3(shape), i3(k), i3(s), i3(p), int(subm),
                                               runtime.ptr(nbr), runtime.ptr(words), runtime.ptr(ws), need, runtime.stream_ptr())
    torch.cuda.synchronize()
    nbr, words = nbr.cpu().numpy(), words.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    return rc, nbr[:n_out], words[:tiles], nbr[n_out:], words[tiles:]
