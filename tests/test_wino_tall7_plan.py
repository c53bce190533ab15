"""CPU: the 7x7 + LayerNorm + GELU layer's tap groups in the tall-tile form (conv_wino7t_kernel, conv_wino.hip).  The plan of the launch —
form, segments, block rows, workgroups — does not depend on the arithmetic: SF_WINO_TALL (unset, 1, 0) moves the tall bit of the segment
and nothing else.  The kernel keeps the budget of the kernels it stands beside: two workgroups of 8 waves per CU = 128 registers, no
scratch, no spills of either kind — read from the built code objects."""
import ctypes
import os

import pytest

from test_kernel_resources import READELF, _kernels

EPI_LNG = 2
TALL = "SF_WINO_TALL"


def _plan(value):
    """sf_debug_wino_plan of the rollout's launch (64 + 64 -> 64 channels, 32 latents of 50x50) under SF_WINO_TALL = value (None: unset)"""
    from streamingflow_amd import _lib
    was = os.environ.get(TALL)
    if value is None:
        os.environ.pop(TALL, None)
    else:
        os.environ[TALL] = str(value)
    try:
        w = _lib.ConvW(w=64, cout=64, cout_pad=64, c0=64, c1=64, cin_pad=128, kh=7, kw=7, dil=1, stride=1, pad=3, act=0, w_wino=64, scale=64, bias=64)
        out = (ctypes.c_int32 * _lib.SF_WINO_PLAN_INTS)()
        _lib.check(_lib.lib().sf_debug_wino_plan(ctypes.byref(w), EPI_LNG, 32, 50, 50, 0, 1, 0, out, len(out)), "sf_debug_wino_plan")
        return list(out)
    finally:
        if was is None:
            os.environ.pop(TALL, None)
        else:
            os.environ[TALL] = was


def test_plan_is_the_same_and_only_the_tall_bit_moves():
    unset, on, off = _plan(None), _plan(1), _plan(0)
    assert unset[0] == 1 and unset[2] == 1, unset            # the Winograd kernel takes it, one launch
    assert unset[3] == 4, unset                              # 32-tile blocks
    assert unset[:12] == on[:12] == off[:12], (unset, on, off)
    assert unset[13:] == on[13:] == off[13:], (unset, on, off)
    assert unset[12] == 1 and on[12] == 1 and off[12] == 0, (unset[12], on[12], off[12])


def test_tall_tap_group_kernel_registers_and_scratch():
    from streamingflow_amd import build
    if not os.path.exists(READELF) or not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("ROCm LLVM tools (llvm-readelf / hipcc) are not installed here")
    mine = [k for k in _kernels(build.build()) if "conv_wino7t_kernel" in k.get("name", "")]
    assert len(mine) == 2, [k["name"] for k in mine]         # plain and concatenated images
    for k in mine:
        assert int(k["vgpr_count"]) <= 128 and int(k["private_segment_fixed_size"]) == 0, k
        assert int(k["vgpr_spill_count"]) == 0 and int(k["sgpr_spill_count"]) == 0, k
