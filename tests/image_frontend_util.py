"""Test-side restatement, in numpy, of what the camera image front end (streamingflow_amd/image_frontend.py -> sf_image_frontend_fwd,
csrc/image_frontend.hip) computes: Pillow's antialiased BILINEAR resize (Resample.c: precompute_coeffs + normalize_coeffs_8bpc, then a
horizontal and a vertical pass in 22-bit fixed point with a uint8 image between them), PIL.Image.crop with its zero padding, and the
ToTensor + Normalize arithmetic of the reference's data loader as torch computes it on the CPU.  The GPU tests compare against this,
because neither the reference tree nor necessarily PIL exists where they run; the CPU tests pin it to a fixture made by the reference."""
import math

import numpy as np
import torch

PRECISION_BITS = 22
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def table(in_size, out_size):
    """(bounds [out_size][2] = (xmin, n), k [out_size][ksize] int32, ksize) of one axis.  All in double, in Pillow's order of operations."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), np.int32)
    k = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            k[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, n)
    return bounds, k, ksize


def _pass(img, bounds, k):
    """One pass along axis 1 of img [rows][in_size][C] uint8 -> [rows][out_size][C] uint8."""
    out = np.zeros((img.shape[0], len(bounds), img.shape[2]), np.uint8)
    src = img.astype(np.int64)
    for xx, (xmin, n) in enumerate(bounds):
        ss = (1 << (PRECISION_BITS - 1)) + (src[:, xmin:xmin + n] * k[xx, :n].astype(np.int64)[None, :, None]).sum(1)
        out[:, xx] = np.clip(ss >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resize(img, size):
    """PIL's img.resize(size = (width, height), BILINEAR) on an [H][W][C] uint8 array: horizontal pass, uint8, vertical pass."""
    Wr, Hr = size
    h = _pass(img, *table(img.shape[1], Wr)[:2])
    return _pass(h.transpose(1, 0, 2), *table(img.shape[0], Hr)[:2]).transpose(1, 0, 2)


def crop(img, box):
    """PIL's img.crop((l, t, r, b)): positions outside the image are 0."""
    l, t, r, b = box
    H, W = img.shape[:2]
    out = np.zeros((b - t, r - l, img.shape[2]), img.dtype)
    y0, y1, x0, x1 = max(t, 0), min(b, H), max(l, 0), min(r, W)
    if y1 > y0 and x1 > x0:
        out[y0 - t:y1 - t, x0 - l:x1 - l] = img[y0:y1, x0:x1]
    return out


def resize_and_crop(img, resize_dims, box):
    return crop(resize(img, resize_dims), box)


def normalise(u8, mean=MEAN, std=STD):
    """[..., h, w, 3] uint8 -> [..., 3, h, w] float32: ToTensor + Normalize as torch computes them on the CPU."""
    t = torch.from_numpy(np.ascontiguousarray(u8)).movedim(-1, -3).float().div(255)
    m, s = (torch.tensor(v, dtype=torch.float32).view(3, 1, 1) for v in (mean, std))
    return t.sub(m).div(s).contiguous()


def geometry(original, resize_scale, top_crop, final_dim):
    """get_resizing_and_cropping_parameters of the reference's data loader: (resize_dims (w, h), crop (l, t, r, b))."""
    (oh, ow), (fh, fw) = original, final_dim
    rw, rh = int(ow * resize_scale), int(oh * resize_scale)
    cw = int(max(0, (rw - fw) / 2))
    return (rw, rh), (cw, top_crop, cw + fw, top_crop + fh)


def update_intrinsics(K, top_crop, left_crop, scale_width, scale_height):
    K = K.clone()
    K[..., 0, 0] *= scale_width
    K[..., 0, 2] *= scale_width
    K[..., 1, 1] *= scale_height
    K[..., 1, 2] *= scale_height
    K[..., 0, 2] -= left_crop
    K[..., 1, 2] -= top_crop
    return K


def source(seed, H, W, kind="random"):
    """Seeded [H][W][3] uint8 test image: random bytes, or a random 0 / 255 pattern (rounding and clipping)."""
    g = np.random.default_rng(seed)
    if kind == "checker":
        return (g.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    return g.integers(0, 256, (H, W, 3)).astype(np.uint8)


# name -> (Hs, Ws, resize_scale, crop box in resized coordinates or None = the whole resized image, kind of source, images)
# The fixture tests/golden/image_frontend.npz (tools/gen_image_frontend_golden.py) holds, per case, what the reference's own functions
# make of source(seed = index of the case, ...): "<name>.u8" and "<name>.f32", and the intrinsics "<name>.K" -> "<name>.K_out".
CASES = {
    "s03_inside": (45, 80, 0.3, (2, 1, 22, 12), "random", 3),          # nine taps, clipped at both borders; three images: the image stride
    "s03_one": (45, 80, 0.3, (2, 1, 22, 12), "random", 1),
    "odd_random": (37, 53, 0.3, None, "random", 1),                   # 159-byte rows: the byte-by-byte form; tap count varies along the axis
    "odd_checker": (37, 53, 0.3, None, "checker", 2),                 # 0 / 255: rounding and clip8
    "half": (64, 96, 0.5, None, "random", 1),                         # five taps
    "identity": (30, 40, 1.0, None, "random", 1),                     # the identity table
    "upscale": (20, 30, 1.7, None, "random", 1),                      # filterscale 1, three taps
    "pad_left_top": (45, 80, 0.3, (-3, -2, 10, 9), "random", 1),      # crop boxes that reach outside the resized image (24 x 13)
    "pad_right_bottom": (45, 80, 0.3, (5, 4, 30, 20), "random", 1),
    "pad_all_sides": (45, 80, 0.3, (-70, -9, 90, 20), "random", 2),   # more than one tile across, whole tiles of padding
    "white": (45, 80, 0.3, None, "white", 1),                         # the coefficient sums are not exactly 2^22
    "black": (45, 80, 0.3, None, "black", 1),
    "fifth": (48, 80, 0.2, None, "random", 2),                        # eleven taps: more than a lane keeps in registers; 240-byte rows
    "fifth_odd": (50, 70, 0.2, (-2, 1, 15, 12), "checker", 1),        # the same with 210-byte rows, a padded crop and 0 / 255 bytes
}


def case(name):
    """(sources [n][Hs][Ws][3] uint8, resize_dims (w, h), crop box, resize_scale) of a case."""
    Hs, Ws, scale, box, kind, n = CASES[name]
    seed = list(CASES).index(name)
    if kind in ("white", "black"):
        src = np.full((n, Hs, Ws, 3), 255 if kind == "white" else 0, np.uint8)
    else:
        src = np.stack([source(100 * seed + i, Hs, Ws, kind) for i in range(n)])
    dims = (int(Ws * scale), int(Hs * scale))
    return src, dims, box or (0, 0, dims[0], dims[1]), scale


def intrinsics(seed):
    g = np.random.default_rng(1000 + seed)
    K = torch.eye(3)
    K[0, 0], K[1, 1] = float(g.uniform(800, 1300)), float(g.uniform(800, 1300))
    K[0, 2], K[1, 2] = float(g.uniform(700, 900)), float(g.uniform(400, 500))
    return K


def expected(name):
    """(u8 [n][h][w][3], f32 [n][3][h][w]) of a case by the restatement."""
    src, dims, box, _ = case(name)
    u8 = np.stack([resize_and_crop(s, dims, box) for s in src])
    return u8, normalise(u8)
