"""TEST INFRASTRUCTURE — tests/golden/resfuture.npz and resfuture_state_dict_keys.json: the REFERENCE's own
``ResFuturePrediction`` / ``ResFuturePredictionV2`` / ``ResFuturePredictionV1`` / ``GRUCell`` / ``warp_with_flow``
(mmdet3d/models/beverse/models/{motion,basic}_modules.py, imported as they are through oracle.refimport.install(), CPU) on
hashed weights and inputs.  Only results are stored; the tests rebuild weights and inputs with ``build`` / ``inputs``.

Usage: python tools/gen_resfuture_golden.py        (where the reference is installed)

Per shape tag <s> and variant <v>:
  <s>/<v>/out      the module's output (b, T, C, h, w) float32 — in full for the smallest shape, channels ``<s>/channels`` of it
                   for the two larger ones (every frame and pixel, so the image borders the warps sample beyond are all there;
                   every stored channel is a function of every channel of every earlier layer), which keeps the file under 1 MB
  <s>/<v>/flow0    flow-warp variants: the first step's flow (b, 2, h, w), in full
  <s>/<v>/warp0    and warp_with_flow(hidden state, that flow), the same channels as ``out``
  gru_cell/out     GRUCell(48, 32) alone, in full
The file is not written unless every flow-warp case has max |flow| >= 1 px in its first step and, on the two larger shapes,
samples beyond each of the four image edges.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from workloads import hashfill  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "resfuture.npz")
KEYS = os.path.join(ROOT, "tests", "golden", "resfuture_state_dict_keys.json")
N_FUTURE = 3
# tag -> (C, L, h, w, B)
SHAPES = {"a": (32, 16, 13, 21, 2), "b": (64, 32, 24, 20, 2), "s": (16, 8, 9, 7, 1)}
FULL = "s"
# variant -> (class name, constructor keywords)
VARIANTS = {
    "res_flow": ("ResFuturePrediction", {}),
    "res_noflow": ("ResFuturePrediction", {"flow_warp": False}),
    "v2_refine": ("ResFuturePredictionV2", {"with_state_refine": True}),
    "v2_shared": ("ResFuturePredictionV2", {"with_state_refine": False}),
    "v2_noflow": ("ResFuturePredictionV2", {"flow_warp": False}),
    "v1": ("ResFuturePredictionV1", {"n_gru_blocks": 2}),
    "v1_each": ("ResFuturePredictionV1", {"n_gru_blocks": 2, "prob_each_future": True}),
}
GRU_CELL = (48, 32, 11, 9, 2)      # input_size, hidden_size, h, w, b


def has_flow(variant):
    return VARIANTS[variant][1].get("flow_warp", True)


def channels(tag):
    """The output channels a fixture stores: all of them for the smallest shape, four spread over the range otherwise."""
    C = SHAPES[tag][0]
    return list(range(C)) if tag == FULL else list(range(1, C, C // 4))


def build(module, tag, variant):
    """The variant's module from `module` (the reference's motion_modules or this package's), hashed weights loaded, eval mode."""
    C, L = SHAPES[tag][:2]
    name, kw = VARIANTS[variant]
    net = getattr(module, name)(C, L, N_FUTURE, **kw)
    net.load_state_dict(hashfill.fill_state_dict(net.state_dict(), seed=2, gain=1.0))
    return net.eval()


def inputs(tag, variant):
    """(sample (B, L [x n_future], h, w), hidden state (B, C, h, w)), CPU."""
    C, L, h, w, B = SHAPES[tag]
    k = N_FUTURE if VARIANTS[variant][1].get("prob_each_future") else 1
    return hashfill.normal("rf_s", (B, L * k, h, w), 41), hashfill.normal("rf_h", (B, C, h, w), 42)


def flow_head(net, variant):
    """(offset ConvBlock, 2-channel 1x1) of the first step."""
    if variant == "res_flow":
        return net.offset_conv, net.offset_pred
    fp = net.flow_pred if variant.startswith("v1") else net.flow_preds[0]
    return fp[0], fp[1]


def build_gru_cell(module):
    cin, hid = GRU_CELL[:2]
    cell = module.GRUCell(cin, hid)
    cell.load_state_dict(hashfill.fill_state_dict(cell.state_dict(), seed=2, gain=1.0))
    return cell.eval()


def gru_cell_inputs():
    cin, hid, h, w, b = GRU_CELL
    return hashfill.normal("rf_gx", (b, cin, h, w), 43), hashfill.normal("rf_gs", (b, hid, h, w), 44)


def main():
    from oracle import refimport
    refimport.install()
    from mmdet3d.models.beverse.models import basic_modules as RB
    from mmdet3d.models.beverse.models import motion_modules as RM
    res, keys = {}, {}
    with torch.no_grad():
        for tag, (C, L, h, w, B) in SHAPES.items():
            idx = channels(tag)
            res[f"{tag}/channels"] = np.asarray(idx, dtype=np.int64)
            for variant in VARIANTS:
                net = build(RM, tag, variant)
                keys[variant] = list(net.state_dict().keys())
                sample, hidden = inputs(tag, variant)
                out = net(sample.clone(), hidden.clone())
                assert out.dtype == torch.float32 and bool(torch.isfinite(out).all())
                res[f"{tag}/{variant}/out"] = out[:, :, idx].contiguous().numpy()
                line = f"{tag} {variant} out {tuple(out.shape)} max|y| {float(out.abs().max()):.3f}"
                if has_flow(variant):
                    blk, head = flow_head(net, variant)
                    flow = head(blk(torch.cat((sample[:, :L], hidden), dim=1)))
                    warp = RM.warp_with_flow(hidden.clone(), flow.clone())      # the reference overwrites its flow argument
                    mag = float(flow.abs().max())
                    ix = flow[:, 0] + torch.arange(w, dtype=torch.float32).view(1, 1, w)
                    iy = flow[:, 1] + torch.arange(h, dtype=torch.float32).view(1, h, 1)
                    sides = {"left": int((ix < 0).sum()), "right": int((ix > w - 1).sum()), "top": int((iy < 0).sum()),
                             "bottom": int((iy > h - 1).sum())}
                    line += f" max|flow| {mag:.2f} px, samples outside {sides}"
                    if mag < 1.0:
                        sys.exit(f"{tag} {variant}: max |flow| {mag} < 1 px: nothing written")
                    if tag != FULL and not all(sides.values()):
                        sys.exit(f"{tag} {variant}: no sample beyond some image edge {sides}: nothing written")
                    res[f"{tag}/{variant}/flow0"] = flow.contiguous().numpy()
                    res[f"{tag}/{variant}/warp0"] = warp[:, idx].contiguous().numpy()
                print(line)
        x, s = gru_cell_inputs()
        res["gru_cell/out"] = build_gru_cell(RB)(x, s).numpy()
    np.savez_compressed(OUT, **res)
    with open(KEYS, "w") as f:
        json.dump(keys, f, indent=0)
    print(OUT, os.path.getsize(OUT), "bytes;", KEYS, os.path.getsize(KEYS), "bytes")


if __name__ == "__main__":
    main()
