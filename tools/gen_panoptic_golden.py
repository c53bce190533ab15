"""TEST INFRASTRUCTURE — tests/golden/panoptic_device.npz: the REFERENCE's own ``PanopticMetric`` (streamingflow/metrics.py:74-261,
imported as it is through oracle.refimport.eval_reference(), CPU) on the instance-id scenes below.  Only data is stored: the id maps
(uint8 / int16) and, per scene, the reference's four counters after each ``update`` with ``temporally_consistent`` True and False.

Usage: python tools/gen_panoptic_golden.py        (where the reference is installed)

Keys.  ``scenes``: the tags.  Per scene <tag>: <tag>.M (the bound on the ids the tests pass as ``max_instances``), <tag>.updates (how
many), <tag>.u<i>.pred / <tag>.u<i>.gt [B, T, H, W], and <tag>.tc<1|0>.u<i>.<counter> [2] float32 = the reference's counter after
update i (tc1: temporally_consistent=True).

Scenes, at the smallest sizes at which the scoring kernel can go wrong:
  rand0 .. rand5  B = 3, T = 5, 24 x 20, M = 9.  Five ground-truth vehicles, 3 x 3 boxes in cells of 6 x 6 that move a pixel every
                  other frame and are absent in some frames.  A prediction is exact (IoU 1), a column wider (0.75), shifted by one pixel
                  (6 / 12: exactly 0.5, NOT a hit) or missing; two vehicles per sample change their predicted id mid-sequence (ids 6, 7);
                  predicted ids 8 and 9 are boxes without ground truth.  The predicted id of ground-truth id g rotates with the sample,
                  so a partner table that is not reset per sample shows.
  k65, k129       ids up to exactly M = 64 / 128 in use on both sides (K = M + 1 is one past a wavefront's 64 lanes), 48 x 40, B = 1,
                  T = 3: 2 x 2 boxes in cells of 3 x 3, predicted id M + 1 - g, some a column wider (4 / 6), some shifted (2 / 6: no hit),
                  some missing, neighbours swapping their predicted ids in the last frame.
  hand            8 x 8, T = 4: areas 3 and 3 with overlap 2 (IoU exactly 0.5: no hit) beside areas 5 and 6 with overlap 4 (4 / 7); an
                  all-background frame; a frame whose background IoU is below 0.5 under a large unmatched prediction; ground-truth id 3
                  that is absent for two frames and comes back under another predicted id (a switch across a gap).
  two             two updates of B = 2, T = 3 scenes of the rand kind: accumulation across updates.

The file is not written unless, over all scenes with tracking on, there are >= 10 thing true positives, >= 3 false negatives and
>= 3 false positives from unmatched things, >= 3 id switches and >= 1 frame without a background true positive
(tests/test_panoptic_fixture.py holds the stored file to the same conditions)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "panoptic_device.npz")
COUNTERS = ("iou", "true_positive", "false_positive", "false_negative")


def rand_update(seed, B=3, T=5, H=24, W=20, n_obj=5):
    """(pred, gt) [B, T, H, W] int64 of the rand kind."""
    rng = np.random.RandomState(seed)
    pred, gt = np.zeros((B, T, H, W), dtype=np.int64), np.zeros((B, T, H, W), dtype=np.int64)
    cells = [(r, c) for r in range(H // 6) for c in range(W // 6)]
    for b in range(B):
        order = rng.permutation(len(cells))
        switchers = rng.choice(n_obj, 2, replace=False)
        switch_at = rng.randint(1, T, size=2)
        down = rng.randint(0, 2, size=n_obj)
        for k in range(n_obj):
            g = k + 1
            r0, c0 = cells[order[k]][0] * 6, cells[order[k]][1] * 6
            for t in range(T):
                if rng.rand() < 0.2:
                    continue                                      # the vehicle is absent in this frame
                r, c = r0 + 1 + (t // 2 if down[k] else 2 - t // 2), c0 + 1
                gt[b, t, r:r + 3, c:c + 3] = g
                p = 1 + (k + b) % n_obj                           # rotates with the sample
                for s, who in enumerate(switchers):
                    if who == k and t >= switch_at[s]:
                        p = 6 + s
                mode = rng.choice(4, p=[0.45, 0.25, 0.15, 0.15])
                if mode == 0:
                    pred[b, t, r:r + 3, c:c + 3] = p
                elif mode == 1:
                    pred[b, t, r:r + 3, c:c + 4] = p              # a column wider: 9 / 12
                elif mode == 2:
                    if rng.rand() < 0.5:
                        pred[b, t, r:r + 3, c + 1:c + 4] = p      # shifted: 6 / 12, exactly one half
                    else:
                        pred[b, t, r - 1:r + 2, c:c + 3] = p
        for s in range(2):                                        # predictions without ground truth
            r0, c0 = cells[order[n_obj + s]][0] * 6, cells[order[n_obj + s]][1] * 6
            for t in range(T):
                if rng.rand() < 0.5:
                    pred[b, t, r0 + 2:r0 + 5, c0 + 1:c0 + 4] = 8 + s
    return pred, gt


def lane_update(M, H=48, W=40, T=3):
    rng = np.random.RandomState(1000 + M)
    pred, gt = np.zeros((1, T, H, W), dtype=np.int64), np.zeros((1, T, H, W), dtype=np.int64)
    per_row = W // 3
    assert (H // 3) * per_row >= M
    for g in range(1, M + 1):
        r, c = ((g - 1) // per_row) * 3, ((g - 1) % per_row) * 3
        for t in range(T):
            p = M + 1 - g
            if t == T - 1 and g % 8 < 2:                          # ids g = 8 n and 8 n + 1 swap their predictions in the last frame
                other = g + 1 if g % 8 == 0 else g - 1
                if 1 <= other <= M:
                    p = M + 1 - other
            gt[0, t, r:r + 2, c:c + 2] = g
            mode = 0 if g in (1, M) else rng.choice(4, p=[0.6, 0.2, 0.1, 0.1])
            if mode == 0:
                pred[0, t, r:r + 2, c:c + 2] = p
            elif mode == 1:
                pred[0, t, r:r + 2, c:c + 3] = p                  # 4 / 6
            elif mode == 2:
                pred[0, t, r:r + 2, c + 1:c + 3] = p              # 2 / 6: no hit
    return pred, gt


def hand_update():
    pred, gt = np.zeros((1, 4, 8, 8), dtype=np.int64), np.zeros((1, 4, 8, 8), dtype=np.int64)
    gt[0, 0, 0, 0:3], pred[0, 0, 0, 1:4] = 1, 1                   # areas 3 and 3, overlap 2: IoU exactly 0.5
    gt[0, 0, 2, 0:5], pred[0, 0, 2, 1:7] = 2, 2                   # areas 5 and 6, overlap 4: 4 / 7
    gt[0, 0, 5:7, 0:3], pred[0, 0, 5:7, 0:3] = 3, 3
    # frame 1: background only
    pred[0, 2, 0:5, :] = 4                                        # 40 of 64 pixels under an unmatched prediction: background IoU 16 / 56
    gt[0, 2, 6:8, 4:8] = 1                                        # ... and an unmatched ground-truth vehicle
    gt[0, 3, 5:7, 0:3], pred[0, 3, 5:7, 0:3] = 3, 2               # id 3 comes back under predicted id 2
    return pred, gt


def scenes():
    """tag -> (M, [(pred, gt), ...] one pair per update)."""
    out = {f"rand{i}": (9, [rand_update(100 + i)]) for i in range(6)}
    out["k65"] = (64, [lane_update(64)])
    out["k129"] = (128, [lane_update(128)])
    out["hand"] = (4, [hand_update()])
    out["two"] = (9, [rand_update(200, B=2, T=3), rand_update(201, B=2, T=3)])
    return out


def conditions(res):
    """The five counts tests/test_panoptic_fixture.py asks of the stored file, from the counters alone."""
    tags = [str(t) for t in res["scenes"]]
    last = {t: int(res[f"{t}.updates"]) - 1 for t in tags}
    final = lambda t, tc, k: res[f"{t}.tc{tc}.u{last[t]}.{k}"]
    thing_tp = sum(float(final(t, 1, "true_positive")[1]) for t in tags)
    switches = sum(float(final(t, 0, "true_positive")[1] - final(t, 1, "true_positive")[1]) for t in tags)
    # without tracking every false negative / false positive is an unmatched thing
    lost = sum(float(final(t, 0, "false_negative")[1]) for t in tags)
    spurious = sum(float(final(t, 0, "false_positive")[1]) for t in tags)
    frames = {t: sum(int(np.prod(res[f"{t}.u{u}.gt"].shape[:2])) for u in range(last[t] + 1)) for t in tags}
    no_bg = sum(frames[t] - float(final(t, 1, "true_positive")[0]) for t in tags)
    return dict(thing_tp=thing_tp, unmatched_fn=lost, unmatched_fp=spurious, switches=switches, frames_without_background_tp=no_bg)


NEEDED = dict(thing_tp=10, unmatched_fn=3, unmatched_fp=3, switches=3, frames_without_background_tp=1)


def main():
    from oracle import refimport
    Ref = refimport.eval_reference().metrics.PanopticMetric
    sc = scenes()
    res = {"scenes": np.array(sorted(sc))}
    for tag, (M, updates) in sorted(sc.items()):
        res[f"{tag}.M"], res[f"{tag}.updates"] = np.int64(M), np.int64(len(updates))
        for u, (pred, gt) in enumerate(updates):
            assert pred.shape == gt.shape and pred.min() == 0 and gt.min() == 0 and max(pred.max(), gt.max()) <= M, tag
            small = np.uint8 if M < 256 else np.int16
            res[f"{tag}.u{u}.pred"], res[f"{tag}.u{u}.gt"] = pred.astype(small), gt.astype(small)
        for tc in (1, 0):
            m = Ref(2, temporally_consistent=bool(tc))
            for u, (pred, gt) in enumerate(updates):
                m.update(torch.from_numpy(pred), torch.from_numpy(gt))
                for k in COUNTERS:
                    res[f"{tag}.tc{tc}.u{u}.{k}"] = getattr(m, k).detach().numpy().astype(np.float32).copy()
            print(tag, "tc", tc, {k: getattr(m, k).tolist() for k in COUNTERS})
    got = conditions(res)
    print(got)
    missed = [k for k, v in NEEDED.items() if got[k] < v]
    if missed:
        sys.exit(f"the scenes miss {missed}: nothing written")
    for tag, (M, _) in sc.items():
        if tag.startswith("k"):
            for side in ("pred", "gt"):
                assert int(res[f"{tag}.u0.{side}"].max()) == M, (tag, side)
    np.savez_compressed(OUT, **res)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
