"""CPU: the fixture of the ground-truth label kernels (tests/golden/instance_labels.npz, tools/gen_instance_labels_golden.py):
every scene's three label tensors are there with the shapes of the inputs ``scene(tag)`` rebuilds, and every branch of the
reference function the generator counted is taken by some (frame, id) pair — a fixture that skipped one would let the GPU
test pass without looking at it."""
import os
import sys

import numpy as np

from util import ROOT, gold

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_instance_labels_golden as GEN  # noqa: E402

BRANCHES = ("frames_with_instances", "frames_without_instances", "pairs_present", "pairs_absent", "flow_written", "flow_none_last_frame",
            "flow_none_absent_next", "flow_none_warped_empty", "flow_none_after_gap", "pixels_id_above_k", "pixels_id_negative",
            "half_tie_even_floor", "half_tie_odd_floor", "ids_past_one_chunk")


def test_fixture_keys_shapes_and_dtypes():
    G = gold("instance_labels.npz")
    want = {f"{tag}.{name}" for tag in GEN.SCENES for name in ("centerness", "offset", "flow")} | {f"branch.{b}" for b in BRANCHES}
    assert set(G.files) == want
    for tag, (_, H, W, T, K) in GEN.SCENES.items():
        s = GEN.scene(tag)
        assert tuple(s["instance"].shape) == (T, H, W) and tuple(s["future_egomotion"].shape) == (T, 6) and s["num_instances"] == K
        assert G[f"{tag}.centerness"].shape == (T, 1, H, W)
        for name in ("offset", "flow"):
            assert G[f"{tag}.{name}"].shape == (T, 2, H, W)
        for name in ("centerness", "offset", "flow"):
            assert G[f"{tag}.{name}"].dtype == np.float32
        c = G[f"{tag}.centerness"]
        assert c.min() >= 0.0 and c.max() <= 1.0
    assert {(H, W) for _, H, W, _, _ in GEN.SCENES.values()} == {(48, 40), (96, 80)}
    assert GEN.SCENES["t1"][3] == 1 and GEN.SCENES["k0"][4] == 0 and GEN.SCENES["b96"][4] > 2 * 128


def test_every_branch_is_taken():
    G = gold("instance_labels.npz")
    for b in BRANCHES:
        assert int(G[f"branch.{b}"]) > 0, b


def test_scenes_hold_what_the_fixture_is_for():
    """Straight from the rebuilt inputs: the drop-out, the single-frame instance, the empty frame, the ids past num_instances."""
    a = GEN.scene("a48")["instance"]
    assert [bool((a[t] == 2).any()) for t in range(6)] == [True, True, False, True, True, True]
    assert [bool((a[t] == 3).any()) for t in range(6)] == [False, True, False, False, False, False]
    assert int((a == 6).sum()) == 6 * 6 and int((a == 7).sum()) == 6 * 8 and int(a.max()) == 9 > GEN.SCENES["a48"][4]
    b = GEN.scene("b96")["instance"]
    assert not b[3].any() and sorted(set(b.unique().tolist()) - {0}) == [-4, 7, 130, 131, 257, 300, 301, 1000]
    assert float(GEN.scene("c48")["future_egomotion"][2, 0]) == GEN.BIG_SHIFT
