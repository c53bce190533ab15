"""CPU: one workspace layout per model entry point (csrc/dispatch.h: Arena; csrc/api.hip, csrc/camera_neck.hip).

Every sf_*_ws_bytes is the entry point's own carve run through a measuring arena, so (1) no query returns more than the parent commit's
hand-kept formula did (tests/golden/ws_bytes_parent.json, written by tools/gen_ws_bytes_parent.py against the parent's library) and
the ones that were exact already are unchanged, and (2) a call given less than the query refuses with SF_ERR_WORKSPACE before it
enqueues or writes anything.  The refusal comes before the first launch, so the tensor pointers are placeholders and the whole file
skips where a GPU is present: they must never reach a device.  Every sf_conv_w handed over is a valid descriptor (a refusal that was
missed must end as a failed launch, not as a division by a zero stride)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from streamingflow_amd import _lib
from ws_layout_util import HOLE, NAMES, entry_points, placeholder_weights

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="placeholder tensor pointers: host only")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ws_bytes_parent.json")
# the parent's formula was the carve already: these stay equal, byte for byte
EXACT_BEFORE = {"sf_gru_cell_ws_bytes", "sf_spatial_gru_ws_bytes", "sf_small_decoder_ws_bytes", "sf_deeplab_head_ws_bytes",
                "sf_convnext_block_ws_bytes", "sf_channel_mean_ws_bytes", "sf_bottleneck_ws_bytes", "sf_dist_head_ws_bytes",
                "sf_nnfo_rollout_carry_bytes"}


def test_sizes_do_not_exceed_the_parent():
    L = _lib.lib()
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert len(gold["commit"]) >= 7 and len(gold["records"]) > 100
    was = L.sf_set_flow_mode(0)
    try:
        for r in gold["records"]:
            L.sf_set_flow_mode(r["flow"])
            now = int(getattr(L, r["fn"])(*r["args"]))
            assert 0 < now <= r["bytes"], (r, now)
            if r["fn"] in EXACT_BEFORE:
                assert now == r["bytes"], (r, now)
        # the flow's tables are part of the rollout's layout exactly while the flow mode is on; ode_step never runs a flow
        L.sf_set_flow_mode(0)
        off, step = L.sf_nnfo_rollout_ws_bytes(64, 1, 8, 16), L.sf_ode_step_ws_bytes(64, 1, 8, 16)
        L.sf_set_flow_mode(1)
        assert L.sf_nnfo_rollout_ws_bytes(64, 1, 8, 16) == off + (1 << 20) + 4 * ((1 << 20) + 64)
        assert L.sf_ode_step_ws_bytes(64, 1, 8, 16) == step
    finally:
        L.sf_set_flow_mode(was)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("C,n,H,W", [(64, 1, 8, 16), (64, 3, 20, 36)])
def test_short_workspace_is_refused_and_nothing_is_written(C, n, H, W, name):
    need, call = entry_points(placeholder_weights(C), HOLE, HOLE, n, H, W)[name]
    assert need > 256
    ws = np.full(1024, 7.0, dtype=np.float32)      # what a refused call could reach if it wrote at all
    ptr = ws.ctypes.data_as(ctypes.c_void_p)
    for short in (need - 256, need // 2, 0):
        assert call(ptr, short) == _lib.SF_ERR_WORKSPACE, (name, short)
    assert call(None, need) == _lib.SF_ERR_WORKSPACE, name
    assert float(np.abs(ws - 7.0).max()) == 0.0
