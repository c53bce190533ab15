"""CPU study behind the bounds of tests/test_gpu_wino_tall7.py: Bottleblock(128 -> 64) — 7x7 + LN + GELU, 1x1 + LN + GELU, 3x3 + LN + GELU, plus
the 1x1 + GELU projection — at the test's data law (input N(0, 1), hashed weights of seed 71), with the 7x7 emulated in fp32 in three
forms: the nine tap groups in F(2x2, 3x3), the nine tap groups in the tall form F(4,3) x F(2,3) (all 24 positions: leaving out the positions
whose weights are zero removes exact zeros from the sums), and the direct form.  Everything behind the 7x7 runs in fp32 too; the reference
is the whole block in fp64.  Writes profiles/winograd42_7x7_accuracy_study.json.

    python tools/winograd42_7x7_study.py
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from workloads import hashfill  # noqa: E402

G4 = [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]]
G2 = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]
B4T = [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]]
B2T = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
A4T = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]
A2T = [[1, 1, 1, 0], [0, 1, -1, -1]]


def groups(x, w, my, mx):
    """the 7x7 / pad-3 convolution of x [n, c, H, W] as nine 3x3 tap groups summed in the transform domain, F(my, 3) along y x F(mx, 3) along x,
    in the dtype of x"""
    dt = x.dtype
    Gy, Gx = torch.tensor(G4 if my == 4 else G2, dtype=dt), torch.tensor(G4 if mx == 4 else G2, dtype=dt)
    By, Bx = torch.tensor(B4T if my == 4 else B2T, dtype=dt), torch.tensor(B4T if mx == 4 else B2T, dtype=dt)
    Ay, Ax = torch.tensor(A4T if my == 4 else A2T, dtype=dt), torch.tensor(A2T if mx == 2 else A4T, dtype=dt)
    n, c, H, W = x.shape
    ty, tx = (H + my - 1) // my, (W + mx - 1) // mx
    xp = F.pad(x, (4, 4 + tx * mx - W, 4, 4 + ty * my - H))
    frame = torch.zeros(w.shape[0], c, 9, 9, dtype=dt)
    frame[:, :, 1:8, 1:8] = w
    M = None
    nz = 0
    for a in range(3):
        for b in range(3):
            g = frame[:, :, 3 * a:3 * a + 3, 3 * b:3 * b + 3]
            U = torch.einsum("ai,ocij,bj->aboc", Gy, g, Gx)
            nz += int((U.abs().amax(dim=(2, 3)) > 0).sum())
            y0, x0 = 4 + 3 * a - 3 - 1, 4 + 3 * b - 3 - 1
            sub = xp[:, :, y0:y0 + ty * my + 2, x0:x0 + tx * mx + 2]
            d = sub.unfold(2, my + 2, my).unfold(3, mx + 2, mx)            # [n, c, ty, tx, my + 2, mx + 2]
            V = torch.einsum("ai,nctsij,bj->abncts", By, d, Bx)
            m = torch.einsum("aboc,abncts->abnots", U, V)
            M = m if M is None else M + m
    Y = torch.einsum("ia,abnots,jb->notisj", Ay, M, Ax).reshape(n, w.shape[0], ty * my, tx * mx)
    return Y[:, :, :H, :W], nz


def ln(x, wt, b):
    u = x.mean(1, keepdim=True)
    s = (x - u).pow(2).mean(1, keepdim=True)
    return wt[None, :, None, None] * ((x - u) / torch.sqrt(s + 1e-6)) + b[None, :, None, None]


def block(sd, x, conv7):
    dt = x.dtype
    p = {k: v.to(dt) for k, v in sd.items()}
    t = F.gelu(ln(conv7(x, p["layers.0.weight"]), p["layers.1.weight"], p["layers.1.bias"]))
    t = F.gelu(ln(F.conv2d(t, p["layers.3.weight"]), p["layers.4.weight"], p["layers.4.bias"]))
    t = F.gelu(ln(F.conv2d(t, p["layers.6.weight"], padding=1), p["layers.7.weight"], p["layers.7.bias"]))
    return t + F.gelu(F.conv2d(x, p["projection.0.weight"]))


def main():
    from streamingflow_amd.layers.convolutions import Bottleblock
    torch.set_num_threads(8)
    m = Bottleblock(128, 64)
    sd = hashfill.fill_state_dict(m.state_dict(), seed=71)
    x = hashfill.normal("t7_study_x", (2, 128, 50, 50), 17)
    want = block(sd, x.double(), lambda v, w: F.conv2d(v, w, padding=3))
    want7 = F.conv2d(x.double(), sd["layers.0.weight"].double(), padding=3)
    res = {"what": "Bottleblock(128 -> 64), input N(0, 1) of 2 x 50x50, hashed weights (seed 71): fp32 emulation against fp64",
           "block_output_abs_max": float(want.abs().max()), "conv7_output_abs_max": float(want7.abs().max()), "forms": {}}
    forms = {"tap_groups_f2x2": lambda v, w: groups(v, w, 2, 2), "tap_groups_tall": lambda v, w: groups(v, w, 4, 2),
             "direct_fp32": lambda v, w: (F.conv2d(v, w, padding=3), None)}
    for name, f in forms.items():
        nzs = []

        def c7(v, w):
            y, nz = f(v, w)
            nzs.append(nz)
            return y
        got = block(sd, x, c7)
        y7, _ = f(x, sd["layers.0.weight"])
        res["forms"][name] = {"block_max_abs_vs_fp64": float((got.double() - want).abs().max()), "conv7_max_abs_vs_fp64": float((y7.double() - want7).abs().max()),
                              "nonzero_positions": nzs[0]}
    tall = res["forms"]["tap_groups_tall"]["block_max_abs_vs_fp64"]
    res["test_bound"] = 5e-5
    res["emulated_tall_below_half_the_bound"] = bool(tall < 2.5e-5)
    out = os.path.join(ROOT, "profiles", "winograd42_7x7_accuracy_study.json")
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
