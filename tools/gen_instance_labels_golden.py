"""TEST INFRASTRUCTURE — tests/golden/instance_labels.npz: the REFERENCE's own convert_instance_mask_to_center_and_offset_label
(streamingflow/utils/instance.py:12-77, imported as is through oracle.refimport.eval_reference(), CPU) on edited
``oracle.cases.eval_scene`` instance maps.  Only results are stored; the tests rebuild the inputs with ``scene(tag)``.

Usage: python tools/gen_instance_labels_golden.py        (where the reference is installed)

Per scene <tag>:  <tag>.centerness [T, 1, H, W], <tag>.offset / <tag>.flow [T, 2, H, W], float32.  branch.<name>: how many
(frame, id) pairs (or frames, or pixels) of all scenes together take each branch of the function; the file is not written when
one of them is zero.  Every scene is also recomputed with its ego-motions scaled by 1 +- 2e-7 and by 1 +- 1e-5: the file is not
written unless the reference's labels stay what they were, so no stored label hangs on a nearest-neighbour rounding boundary and
the tests may demand equality on every pixel.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import cases  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "instance_labels.npz")
EXTENT = (50.0, 50.0)
BIG_SHIFT = 36.0        # metres along x at one step of "c48": 0.72 of the half grid, about 17 rows of 48
# tag -> (seed of eval_scene, H, W, T, num_instances)
SCENES = {
    "a48": (0, 48, 40, 6, 7),       # drop-out, single-frame instance, half-tie blocks, an id above K
    "c48": (2, 48, 40, 6, 7),       # a large ego-motion: warped instances leave the grid; stacks with a48 for the batched call
    "b96": (1, 96, 80, 5, 300),     # sparse ids up to 300 (three table chunks of 128), an empty frame
    "t1": (3, 48, 40, 1, 5),        # a single frame: no warp, no flow
    "k0": (0, 48, 40, 6, 0),        # num_instances = 0 on a48's map: every id is background
}
SPARSE_IDS = (7, 130, 131, 257, 300)
PERTURB = (2e-7, 1e-5)


def _ego(seed, T):
    g = torch.Generator().manual_seed(700 + seed)
    return torch.cat([(torch.rand((T, 3), generator=g) - 0.5) * torch.tensor([6.0, 4.0, 0.0]),
                      (torch.rand((T, 3), generator=g) - 0.5) * torch.tensor([0.0, 0.0, 0.12])], -1)


def _blocks(inst, first_free):
    """A 3x2 and a 2x4 block that move one row per frame (ids first_free, first_free + 1) and a 3x3 block with an id past them.
    The 3x2 block's column mean is 10.5 (even floor), the 2x4 block's 31.5 (odd floor) and its row mean 20.5 + t."""
    for t in range(inst.shape[0]):
        inst[t, 4 + t:7 + t, 10:12] = first_free
        inst[t, 20 + t:22 + t, 30:34] = first_free + 1
        inst[t, 40:43, 5:8] = first_free + 3


def scene(tag):
    """The inputs of a fixture scene (CPU tensors): instance [T, H, W] int64, future_egomotion [T, 6], num_instances and the
    keyword arguments of the call."""
    seed, H, W, T, K = SCENES[tag]
    inst = cases.eval_scene(seed, b=1, s=T, h=H, w=W, n_obj=5)[1]["instance"][0].clone()
    ego = _ego(seed, T)
    if tag in ("a48", "k0", "c48"):
        inst[2][inst[2] == 2] = 0                     # instance 2 misses one middle frame
        for t in range(T):
            if t != 1:
                inst[t][inst[t] == 3] = 0             # instance 3 lives in a single frame
        _blocks(inst, 6)
        if tag == "c48":
            ego[2, 0] = BIG_SHIFT
    elif tag == "b96":
        table = torch.zeros(6, dtype=torch.long)
        table[1:] = torch.tensor(SPARSE_IDS)
        inst = table[inst]
        inst[:, 60:62, 40:43] = 301                   # ids above num_instances
        inst[3] = 0                                   # an empty frame
        inst[1][inst[1] == 130] = 0
        inst[0, 0, 0] = 1000
        inst[4, 95, 79] = -4
    return {"instance": inst.contiguous(), "future_egomotion": ego.contiguous(), "num_instances": K,
            "kwargs": {"ignore_index": 255, "sigma": 3, "spatial_extent": EXTENT}}


def stacked(tags):
    """Scenes of one shape as a batch: (instance [B, T, H, W], future_egomotion [B, T, 6], num_instances, kwargs)."""
    ss = [scene(t) for t in tags]
    assert len({(tuple(s["instance"].shape), s["num_instances"]) for s in ss}) == 1
    return torch.stack([s["instance"] for s in ss]), torch.stack([s["future_egomotion"] for s in ss]), ss[0]["num_instances"], ss[0]["kwargs"]


def _branches(s, warp):
    """How the (frame, id) pairs of a scene spread over the branches of steps 3-5, from the inputs and the reference's warp."""
    inst, ego, K = s["instance"], s["future_egomotion"], s["num_instances"]
    T = inst.shape[0]
    inv = warp["mat2pose_vec"](warp["pose_vec2mat"](ego).inverse())
    warped = {t: warp["warp_features"](inst[t][None, None].float(), inv[t - 1][None], mode="nearest", spatial_extent=EXTENT)[0, 0]
              for t in range(1, T)}
    n = dict.fromkeys(("frames_with_instances", "frames_without_instances", "pairs_present", "pairs_absent", "flow_written",
                       "flow_none_last_frame", "flow_none_absent_next", "flow_none_warped_empty", "flow_none_after_gap",
                       "pixels_id_above_k", "pixels_id_negative", "half_tie_even_floor", "half_tie_odd_floor", "ids_past_one_chunk"), 0)
    rows = torch.arange(inst.shape[1], dtype=torch.float)[:, None].expand(inst.shape[1:])
    cols = torch.arange(inst.shape[2], dtype=torch.float)[None, :].expand(inst.shape[1:])
    n["pixels_id_above_k"] += int((inst > K).sum())
    n["pixels_id_negative"] += int((inst < 0).sum())
    for t in range(T):
        here = [k for k in range(1, K + 1) if bool((inst[t] == k).any())]
        n["frames_with_instances" if here else "frames_without_instances"] += 1
        n["pairs_present"] += len(here)
        n["pairs_absent"] += K - len(here)
        for k in here:
            n["ids_past_one_chunk"] += int(k > 128)
            for grid in (rows, cols):
                m = float(grid[inst[t] == k].mean())
                if m - np.floor(m) == 0.5:
                    n["half_tie_even_floor" if int(np.floor(m)) % 2 == 0 else "half_tie_odd_floor"] += 1
            if t == T - 1:
                n["flow_none_last_frame"] += 1
            elif not bool((inst[t + 1] == k).any()):
                n["flow_none_absent_next"] += 1
            elif not bool((warped[t + 1] == k).any()):
                n["flow_none_warped_empty"] += 1
            else:
                n["flow_written"] += 1
            if t >= 2 and not bool((inst[t - 1] == k).any()) and any(bool((inst[u] == k).any()) for u in range(t - 1)):
                n["flow_none_after_gap"] += 1
    return n


def main():
    from oracle import refimport
    ref = refimport.eval_reference().instance
    from streamingflow.utils import geometry as G
    warp = {"mat2pose_vec": G.mat2pose_vec, "pose_vec2mat": G.pose_vec2mat, "warp_features": G.warp_features}
    fn = ref.convert_instance_mask_to_center_and_offset_label
    res, total = {}, {}
    for tag in SCENES:
        s = scene(tag)
        got = fn(s["instance"], s["future_egomotion"], s["num_instances"], **s["kwargs"])
        for eps in PERTURB:
            for sign in (1.0, -1.0):
                ego = (s["future_egomotion"].double() * (1.0 + sign * eps)).float()
                assert not torch.equal(ego, s["future_egomotion"])
                again = fn(s["instance"], ego, s["num_instances"], **s["kwargs"])
                for name, a, b in zip(("centerness", "offset", "flow"), got, again):
                    if not torch.equal(a, b):
                        sys.exit(f"{tag}: the reference's {name} changes when the ego-motions are scaled by 1 {sign * eps:+g}: "
                                 "a label sits on a rounding boundary, nothing written")
        for name, v in zip(("centerness", "offset", "flow"), got):
            assert v.dtype == torch.float32
            res[f"{tag}.{name}"] = v.numpy()
        br = _branches(s, warp)
        print(tag, tuple(s["instance"].shape), "K", s["num_instances"], br)
        for k, v in br.items():
            total[k] = total.get(k, 0) + v
    print("all scenes", total)
    empty = [k for k, v in total.items() if v == 0]
    if empty:
        sys.exit(f"no (frame, id) pair takes the branches {empty}: nothing written")
    for k, v in total.items():
        res[f"branch.{k}"] = np.int64(v)
    np.savez_compressed(OUT, **res)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
