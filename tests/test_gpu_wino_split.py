"""conv_wino5_kernel without workgroups on tiles outside the image.  (1) A layer whose tile rows are not a multiple of four runs as a
main launch on 32-tile blocks and a remainder launch on 16-tile blocks over a window of tile rows (dispatch.hip: wino_plan,
SF_WINO_SPLIT_WGS; 0 keeps the layer whole).  (2) 200x200 layers of 128 or more output channels run on images concatenated along x instead
of 104 tile columns for 100 (wino_plan, SF_WINO_CAT_WIDE; 0 keeps the plain form).  Every real tile is computed by the same arithmetic in both
forms, so the two must agree — and both with the oracle the existing Winograd cases use (test_gpu_conv_random.py: torch's conv2d,
2e-4; the direct form of the same layer, 5e-5)."""
import os

import pytest
import torch

from util import hashfill, maxabs, wino_plan

pytestmark = pytest.mark.gpu

SPLIT, WIDE = "SF_WINO_SPLIT_WGS", "SF_WINO_CAT_WIDE"


class _env:
    """both switches are read at every plan of a launch: set one for the calls inside the block"""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.was = os.environ.get(self.name)
        os.environ[self.name] = str(self.value)

    def __exit__(self, *a):
        if self.was is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.was


# 64 -> 64 and 128 -> 128 layers: 50x50 (25 tile rows: one left over), 100x100 (50: two left over), 200x200 (100: none — the switch must
# change nothing); image counts that keep the layer above the 1 000 workgroups below which it runs whole on 16-tile blocks, and 50x50x32
# with 64 output channels, which does not; one and two sources, residual before / after the activation, channel-sliced tensors
_CASES = [
    dict(c0=128, c1=0, cout=128, n=32, H=50, W=50),
    dict(c0=64, c1=0, cout=64, n=64, H=50, W=50),
    dict(c0=64, c1=0, cout=64, n=32, H=50, W=50),
    dict(c0=64, c1=64, cout=128, n=8, H=100, W=100),
    dict(c0=64, c1=0, cout=64, n=16, H=100, W=100),
    dict(c0=128, c1=0, cout=128, n=4, H=200, W=200),
    dict(c0=64, c1=0, cout=64, n=4, H=200, W=200),
    # odd sizes: 27 tile rows (three left over: two remainder blocks, the last one half outside the image), odd H (half-used last tile)
    dict(c0=32, c1=32, cout=128, n=40, H=53, W=50),
    dict(c0=64, c1=0, cout=64, n=6, H=181, W=187),
]
_SPLITS = [True, True, False, True, True, False, False, True, True]      # which of them the rule splits (checked below)


@pytest.mark.parametrize("i", range(len(_CASES)))
def test_split_layer_equals_the_whole_layer(i):
    from test_gpu_conv_random import _run
    c = dict(k=3, stride=1, dil=1, pad=1, act=["relu", "none", "lrelu", "tanh"][i % 4], add=i % 3 != 1, after=i % 2 == 0, in_slack=8 * (i % 2),
             out_slack=[0, 4, 16][i % 3])
    c.update(_CASES[i])
    layer = {k: c[k] for k in ("c0", "c1", "cout", "n", "H", "W")}
    with _env(SPLIT, 0):
        assert len(wino_plan(**layer)["segs"]) == 1
        whole = _run(c, 700 + i, wino=True)        # (asserts <= 2e-4 against torch)
    with _env(SPLIT, 1):
        # what the library plans (sf_debug_wino_plan): the split case as two launches, the other as one
        assert len(wino_plan(**layer)["segs"]) == (2 if _SPLITS[i] else 1), "the case no longer exercises what it was chosen for"
        split = _run(c, 700 + i, wino=True)
    direct = _run(c, 700 + i, wino=False)
    d = maxabs(split, whole)
    print(f"case {i}: split vs whole {d:.3e}, split vs direct {maxabs(split, direct):.3e}")
    assert maxabs(split, direct) <= 5e-5, maxabs(split, direct)
    assert d <= 5e-5, d


# 200x200 (100 tile columns: 4 % of the plain form's block columns are empty): 128 and 256 output channels take the concatenated form,
# 64 keep the plain one (the switch must change nothing); two images are the smallest launch the form takes; 181x187 has 2 % empty
# columns and stays plain
_WIDE = [
    dict(c0=128, c1=0, cout=128, n=4, H=200, W=200),
    dict(c0=64, c1=64, cout=128, n=2, H=200, W=200),
    dict(c0=32, c1=0, cout=256, n=3, H=200, W=200),
    dict(c0=64, c1=0, cout=64, n=4, H=200, W=200),
    dict(c0=64, c1=0, cout=128, n=5, H=181, W=187),
    dict(c0=64, c1=0, cout=128, n=3, H=198, W=199),
]


@pytest.mark.parametrize("i", range(len(_WIDE)))
def test_concatenated_200x200_layer_equals_the_plain_form(i):
    from test_gpu_conv_random import _run
    c = dict(k=3, stride=1, dil=1, pad=1, act=["lrelu", "relu", "none", "tanh"][i % 4], add=i % 3 != 2, after=i % 2 == 1, in_slack=8 * (i % 2),
             out_slack=[4, 0, 16][i % 3])
    c.update(_WIDE[i])
    with _env(WIDE, 0):
        plain = _run(c, 800 + i, wino=True)        # (asserts <= 2e-4 against torch)
    with _env(WIDE, 1):
        cat = _run(c, 800 + i, wino=True)
    direct = _run(c, 800 + i, wino=False)
    d = maxabs(cat, plain)
    print(f"case {i}: concatenated vs plain {d:.3e}, concatenated vs direct {maxabs(cat, direct):.3e}")
    assert maxabs(cat, direct) <= 5e-5, maxabs(cat, direct)
    assert d <= 5e-5, d


@pytest.mark.parametrize("B,h,w,switch", [(32, 50, 50, SPLIT), (2, 200, 200, WIDE)])
def test_gates_with_second_output_and_blend(B, h, w, switch):
    """The conv-GRU cell: [update ; reset] gates (128 output channels, AFFINE with the reset gate's second output) and the candidate with
    the state blend (BLEND, 64 channels), then infer_state (SE-scaled input, sampling layer).  32 batched 50x50 latents: the gates are
    1 408 workgroups and split, the candidate runs whole on 16-tile blocks, infer_state's SE-scaled and sampling layers have no 16-tile
    form and stay whole.  Two 200x200 frames: the gates take the concatenated form.  Switch on == switch off, and both against the
    direct form at the bound test_winograd_epilogues_of_the_batched_latents_against_the_direct_form holds (2e-5)."""
    from util import build_pair, cases
    from streamingflow_amd import packing
    C = 64
    cts, lts, tts, dt = cases.timeset("shipped")
    assert wino_plan(C, C, 2 * C, B, h, w, flags=4)["wgs32"] >= 1000      # the gates launch, counted on 32-tile blocks

    def build(wino, on):
        was = packing.winograd()
        packing.set_winograd(wino)
        try:
            net, _ = build_pair(C, "euler", True, True, dt)
            gru, ode = net.spatial_grus[0], net.gru_ode
            x = (hashfill.normal("ws_x", (3, B, h, w, C), 11) * 0.5).cuda()
            s0 = (hashfill.normal("ws_s", (B, h, w, C), 12) * 0.5).cuda()
            ode.noise = hashfill.HashedNoise(3)
            with _env(switch, on):
                y = gru.forward_nhwc(x, s0)
                p, q = ode.infer_state(s0.permute(0, 3, 1, 2).contiguous())
                torch.cuda.synchronize()
            return y, p, q
        finally:
            packing.set_winograd(was)
    off, on, direct = build(True, 0), build(True, 1), build(False, 0)
    for a, b, d in zip(on, off, direct):
        print(f"on vs off {maxabs(a, b):.3e}, on vs direct {maxabs(a, d):.3e}")
        assert a.shape == b.shape and maxabs(a, b) <= 2e-5, maxabs(a, b)
        assert maxabs(a, d) <= 2e-5, maxabs(a, d)
