"""CPU: tests/golden/panoptic_device.npz (tools/gen_panoptic_golden.py) still holds what the device-path tests of PanopticMetric
(tests/test_gpu_panoptic_device.py) lean on, so that a regenerated file cannot go vacuous.  The conditions are read from the
reference's own counters: id switches = thing true positives without tracking minus those with it; unmatched things = the false
negatives / positives without tracking (there every one of them is an unmatched thing); frames without a background true positive =
B * T minus the class-0 true positives."""
import numpy as np

import panoptic_util as PU


def test_scenes_have_the_stated_sizes():
    S = PU.scenes()
    assert sorted(S) == sorted([f"rand{i}" for i in range(6)] + ["k65", "k129", "hand", "two"])
    for tag, sc in S.items():
        for pred, gt in sc.updates:
            assert pred.shape == gt.shape and pred.dtype == gt.dtype and pred.dtype in (np.uint8, np.int16)
            assert pred.min() == 0 and gt.min() == 0 and max(pred.max(), gt.max()) <= sc.M
        for tc in (1, 0):
            assert len(sc.ref[tc]) == len(sc.updates)
            for row in sc.ref[tc]:
                assert all(row[k].shape == (2,) and row[k].dtype == np.float32 for k in PU.COUNTERS)
    for i in range(6):
        assert S[f"rand{i}"].M == 9 and S[f"rand{i}"].updates[0][0].shape == (3, 5, 24, 20)
    for tag, M in (("k65", 64), ("k129", 128)):      # ids up to exactly M in use on both sides
        pred, gt = S[tag].updates[0]
        assert S[tag].M == M and pred.shape == (1, 3, 48, 40) and pred.max() == M and gt.max() == M
    assert S["hand"].updates[0][0].shape == (1, 4, 8, 8) and len(S["two"].updates) == 2


def test_hand_scene_holds_its_cases():
    pred, gt = (a.astype(np.int64) for a in PU.scenes()["hand"].updates[0])
    a, b = gt[0, 0] == 1, pred[0, 0] == 1
    assert a.sum() == 3 and b.sum() == 3 and (a & b).sum() == 2                       # IoU exactly one half
    a, b = gt[0, 0] == 2, pred[0, 0] == 2
    assert 2 * (a & b).sum() > (a | b).sum() and (a & b).sum() / (a | b).sum() < 0.6    # just above
    assert not pred[0, 1].any() and not gt[0, 1].any()                                # background only
    a, b = gt[0, 2] == 0, pred[0, 2] == 0
    assert 2 * (a & b).sum() <= (a | b).sum()                                         # the background is no hit
    assert (gt[0, 0] == 3).any() and not (gt[0, 1:3] == 3).any() and (gt[0, 3] == 3).any()
    assert set(pred[0, 0][gt[0, 0] == 3]) == {3} and set(pred[0, 3][gt[0, 3] == 3]) == {2}


def test_fixture_is_not_vacuous():
    S = PU.scenes()
    final = lambda sc, tc, k: sc.ref[tc][-1][k]
    frames = lambda sc: sum(int(np.prod(gt.shape[:2])) for _, gt in sc.updates)
    thing_tp = sum(float(final(sc, 1, "true_positive")[1]) for sc in S.values())
    switches = sum(float(final(sc, 0, "true_positive")[1] - final(sc, 1, "true_positive")[1]) for sc in S.values())
    unmatched_fn = sum(float(final(sc, 0, "false_negative")[1]) for sc in S.values())
    unmatched_fp = sum(float(final(sc, 0, "false_positive")[1]) for sc in S.values())
    no_background = sum(frames(sc) - float(final(sc, 1, "true_positive")[0]) for sc in S.values())
    assert thing_tp >= 10 and unmatched_fn >= 3 and unmatched_fp >= 3 and switches >= 3 and no_background >= 1
    # a switch costs one true positive and adds one false negative and one false positive, in every scene
    for sc in S.values():
        d = final(sc, 0, "true_positive")[1] - final(sc, 1, "true_positive")[1]
        assert final(sc, 1, "false_negative")[1] - final(sc, 0, "false_negative")[1] == d
        assert final(sc, 1, "false_positive")[1] - final(sc, 0, "false_positive")[1] == d
    # a sample whose ground-truth ids meet other partners than the sample before it (a partner table kept across samples would show)
    pred, gt = (a.astype(np.int64) for a in S["rand0"].updates[0])
    first = lambda b, g: next((int(np.bincount(pred[b, t][gt[b, t] == g]).argmax()) for t in range(5) if (gt[b, t] == g).any()), None)
    assert any(first(0, g) not in (None, 0) and first(1, g) not in (None, 0, first(0, g)) for g in range(1, 6))
    assert len(S["two"].ref[1]) == 2 and (S["two"].ref[1][1]["true_positive"] > S["two"].ref[1][0]["true_positive"]).all()
