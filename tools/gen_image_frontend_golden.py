"""Writes tests/golden/image_frontend.npz: what the REFERENCE's own functions (streamingflow.utils.geometry.resize_and_crop_image and
update_intrinsics, on PIL images) make of the seeded sources of tests/image_frontend_util.py's CASES, and the ToTensor + Normalize
arithmetic of its data loader (NuscenesData.py:77-79) as torch computes it on the CPU.  Needs the reference tree and PIL; the tests read
the file and need neither.
Per case: "<name>.src" [n][Hs][Ws][3] uint8, "<name>.u8" [n][h][w][3] uint8, "<name>.f32" [n][3][h][w] float32, "<name>.K" and
"<name>.K_out" [3][3] float32.
Usage: python3 tools/gen_image_frontend_golden.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    from PIL import Image
    from oracle import refimport
    import image_frontend_util as U
    refimport.install()
    from streamingflow.utils.geometry import resize_and_crop_image, update_intrinsics
    mean, std = (torch.tensor(v, dtype=torch.float32).view(3, 1, 1) for v in (U.MEAN, U.STD))
    out = {}
    for i, name in enumerate(U.CASES):
        src, dims, box, scale = U.case(name)
        u8 = np.stack([np.asarray(resize_and_crop_image(Image.fromarray(s), resize_dims=dims, crop=box)) for s in src])
        # ToTensor (uint8 HWC -> float CHW / 255) and Normalize ((x - mean) / std), the operations torchvision performs
        f32 = torch.from_numpy(u8).permute(0, 3, 1, 2).float().div(255).sub(mean).div(std)
        K = U.intrinsics(i)
        out[name + ".src"], out[name + ".u8"], out[name + ".f32"] = src, u8, f32.numpy()
        out[name + ".K"] = K.numpy()
        out[name + ".K_out"] = update_intrinsics(K, top_crop=box[1], left_crop=box[0], scale_width=scale, scale_height=scale).numpy()
    path = os.path.join(ROOT, "tests", "golden", "image_frontend.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(U.CASES), "cases")


if __name__ == "__main__":
    main()
