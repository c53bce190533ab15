"""GPU: the BEVerse ResFuturePrediction family on the device path (sf_conv2d_ex_fwd offset head, sf_flow_warp_fwd with the fused
2-channel 1x1, sf_gru_cell_fwd, sf_spatial_gru_fwd) against fixtures generated from the reference classes
(tests/golden/resfuture.npz, tools/gen_resfuture_golden.py).
  * every variant and shape to 1e-3, the bound of test_beverse.py's test_gpu_matches_reference_fixture and of the north star:
    run on the CPU, the reference's rollouts move by at most 3.7e-5 for a 1e-5 input perturbation, so the device path's
    summation-order differences (1e-6 .. 1e-5 a layer) land well inside it;
  * GRUCell alone to 1e-4, as test_single_branch_cells_gpu;
  * a forward captured with torch.cuda.graph on one stream replays bitwise.
The fixtures stay under 1,000 pixels.  Sizes above them — every kernel family the cells' dispatch reaches, up to the Winograd launches of
the benchmarked 200 x 200 rollout, against a float64 cell on all channels — are in tests/test_gpu_beverse_cells.py."""
import os
import sys

import pytest
import torch

from util import ROOT, gold, maxabs

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_resfuture_golden as GEN  # noqa: E402

pytestmark = pytest.mark.gpu


def _modules():
    from streamingflow_amd.beverse import basic_modules as B, motion_modules as M
    return B, M


@pytest.mark.parametrize("tag,variant", [(t, v) for t in GEN.SHAPES for v in GEN.VARIANTS])
def test_gpu_matches_reference_fixture(tag, variant):
    _, M = _modules()
    g = gold("resfuture.npz")
    net = GEN.build(M, tag, variant).cuda()
    sample, hidden = (t.cuda() for t in GEN.inputs(tag, variant))
    out = net(sample, hidden)
    C, L, h, w, B = GEN.SHAPES[tag]
    assert tuple(out.shape) == (B, GEN.N_FUTURE + (1 if variant.startswith("v1") else 0), C, h, w)
    err = maxabs(out[:, :, GEN.channels(tag)], g[f"{tag}/{variant}/out"])
    print(tag, variant, "max |device - reference|", err)
    assert err <= 1e-3


def test_gru_cell_gpu():
    B, _ = _modules()
    g = gold("resfuture.npz")
    cell = GEN.build_gru_cell(B).cuda()
    x, s = (t.cuda() for t in GEN.gru_cell_inputs())
    err = maxabs(cell(x, s), g["gru_cell/out"])
    print("GRUCell max |device - reference|", err)
    assert err <= 1e-4


def test_graph_capture_replays_bitwise():
    _, M = _modules()
    net = GEN.build(M, "a", "res_flow").cuda()
    sample, hidden = (t.cuda() for t in GEN.inputs("a", "res_flow"))
    eager = net(sample, hidden).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        net(sample, hidden)                                 # this stream's workspace and the packed weights exist before the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = net(sample, hidden)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
