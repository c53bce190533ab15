"""CPU: the workspace of the ASPP head with the 1x1 branch inside the projection launch (csrc/api.hip: deeplab_head).

The producer form keeps `cat` at its channel stride of 4 hid (slice 0 unused), so it carves what the two-launch form carves, in the same
order: cat [P][4 hid], y and z [P][hid], the pooling partials [n][64][C], the per-image bias [n][hid], each rounded up to 64 floats.
sf_deeplab_head_ws_bytes must be at least that sum, and a head given less must refuse with SF_ERR_WORKSPACE before anything is launched or
written — in both forms (SF_GLDS bits 4 and 5 are re-read at every head).  The refusal comes before the first launch, so the tensor
pointers are placeholders and no GPU is needed; a call with ENOUGH workspace would launch and is left to the GPU tests."""
import ctypes
import os

import numpy as np
import pytest

SF_ERR_WORKSPACE = -2


def _al(n):
    return (n + 63) // 64 * 64


@pytest.mark.parametrize("glds", ["63", "47", None], ids=["producer_forced", "two_launches_forced", "default"])
@pytest.mark.parametrize("C,hid,n,H,W", [(64, 128, 1, 8, 16), (64, 128, 3, 20, 36), (96, 128, 3, 20, 36), (64, 128, 32, 200, 200)])
def test_workspace_is_enough_and_less_is_refused(C, hid, n, H, W, glds, monkeypatch):
    from streamingflow_amd import _lib
    L = _lib.lib()
    if glds is None:
        monkeypatch.delenv("SF_GLDS", raising=False)
    else:
        monkeypatch.setenv("SF_GLDS", glds)
    P = n * H * W
    takes = 4 * (_al(P * 4 * hid) + 2 * _al(P * hid) + _al(n * 64 * C) + _al(n * hid))
    need = L.sf_deeplab_head_ws_bytes(C, hid, n, H, W)
    assert need >= takes, (need, takes)
    w = _lib.DeepLabW()
    w.C, w.hid = C, hid
    ws = np.full(1024, 7.0, dtype=np.float32)      # what a refused call could reach if it wrote at all
    hole = ctypes.c_void_p(4096)                   # never dereferenced
    for short in (takes - 4, takes // 2, ws.nbytes, 0):
        rc = L.sf_deeplab_head_fwd(ctypes.byref(w), hole, hole, n, H, W, ws.ctypes.data_as(ctypes.c_void_p), short, None)
        assert rc == SF_ERR_WORKSPACE, (short, rc)
        rc = L.sf_deeplab_head_planar_fwd(ctypes.byref(w), hole, hole, n, H, W, 1, 10**9, 10**9, ws.ctypes.data_as(ctypes.c_void_p), short, None)
        assert rc == SF_ERR_WORKSPACE, (short, rc)
    assert float(np.abs(ws - 7.0).max()) == 0.0
    assert "SF_GLDS" not in os.environ or os.environ["SF_GLDS"] == glds
