"""CPU: the tall-tile Winograd kernel (conv_wino5t_kernel: AFFINE / BLEND x plain / concatenated images) keeps the budget of the F(2x2)
kernel it stands beside — two workgroups of 8 waves per CU = 128 registers, no scratch, no spills — read from the built code objects."""
import os

import pytest

from test_kernel_resources import READELF, _kernels


def test_tall_kernel_registers_and_scratch():
    from streamingflow_amd import build
    if not os.path.exists(READELF) or not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("ROCm LLVM tools (llvm-readelf / hipcc) are not installed here")
    tall = [k for k in _kernels(build.build()) if "conv_wino5t_kernel" in k.get("name", "")]
    assert len(tall) == 4, [k["name"] for k in tall]
    for k in tall:
        assert int(k["vgpr_count"]) <= 128 and int(k["private_segment_fixed_size"]) == 0, k
        assert int(k["vgpr_spill_count"]) == 0 and int(k["sgpr_spill_count"]) == 0, k
        assert int(k["group_segment_fixed_size"]) == 0      # dynamic LDS: 2 x (64 KB exchange + scale / bias / SE-scale rows) per CU
