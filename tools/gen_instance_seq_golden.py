"""TEST INFRASTRUCTURE — tests/golden/instance_short_interval.npz: the REFERENCE's own instance post-processing of the streaming
evaluator (streamingflow/utils/instance.py, imported as is through oracle.refimport.eval_reference(), CPU) on subsampled
``oracle.cases.eval_scene`` sequences.  Only results are stored; the tests regenerate the inputs with ``scene_output``.

Usage: python tools/gen_instance_seq_golden.py        (where the reference is installed)

Per scene <tag>:  <tag>.raw [b, T, H, W] the per-frame maps (get_instance_segmentation_and_centers frame by frame),
<tag>.short / <tag>.regular [b, T, H, W] predict_instance_segmentation_and_trajectories(_short_interval), and for the b = 1
scene <tag>.track_short.<id> / <tag>.track_regular.<id> [n, 2] the matched-centre tracks.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import cases  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "instance_short_interval.npz")
H, W, N_OBJ = 96, 80, 5
# tag -> (seed, k: every k-th frame is kept, b, frames kept, index of a frame whose centre map is zeroed or None)
SCENES = {
    "s0k1": (0, 1, 2, 4, None),      # consecutive frames: both matchers agree
    "s1k4": (1, 4, 2, 4, None),      # the flow no longer reaches the next kept frame: the regular matcher loses instances
    "s3k6": (3, 6, 2, 4, None),      # some instances move more than 10 pixels: the short-interval matcher starts new ids too
    "s2k4e": (2, 4, 1, 5, 2),        # an empty middle frame: the later frames keep their raw ids
}
TRACK_SCENE = "s2k4e"


def scene_output(tag):
    """The decoder-output dict of a scene (CPU tensors)."""
    seed, k, b, kept, empty = SCENES[tag]
    out, _ = cases.eval_scene(seed, b=b, s=(kept - 1) * k + 1, h=H, w=W, n_obj=N_OBJ)
    out = {name: v[:, ::k].contiguous() for name, v in out.items()}
    if empty is not None:
        out["instance_center"][:, empty] = 0
    return out


def main():
    from oracle import refimport
    I = refimport.eval_reference().instance
    res = {}
    for tag, (seed, k, b, kept, empty) in SCENES.items():
        o = scene_output(tag)
        fg = torch.argmax(o["segmentation"], dim=2) == 1
        raw = torch.stack([torch.stack([I.get_instance_segmentation_and_centers(o["instance_center"][bi, t].clone(), o["instance_offset"][bi, t],
                                                                                fg[bi, t])[0][0] for t in range(kept)]) for bi in range(b)])
        res[f"{tag}.raw"] = raw.numpy()
        for name, fn in (("short", I.predict_instance_segmentation_and_trajectories_short_interval),
                         ("regular", I.predict_instance_segmentation_and_trajectories)):
            got = fn({n: v.clone() for n, v in o.items()}, compute_matched_centers=(tag == TRACK_SCENE))
            if tag == TRACK_SCENE:
                got, tracks = got
                for ident, v in tracks.items():
                    res[f"{tag}.track_{name}.{int(ident)}"] = np.ascontiguousarray(v)
            res[f"{tag}.{name}"] = got.numpy()
        print(tag, "frames", tuple(raw.shape), "per-frame max", raw.amax(dim=(2, 3)).tolist(), "short ids", int(res[f"{tag}.short"].max()),
              "regular ids", int(res[f"{tag}.regular"].max()), "equal", bool(np.array_equal(res[f"{tag}.short"], res[f"{tag}.regular"])))
    np.savez_compressed(OUT, **{k: (v.astype(np.int16) if v.dtype == np.int64 else v) for k, v in res.items()})
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
