"""``ImageFrontend`` — decoded camera frames (uint8, H x W x 3) to the image tensor the encoder reads, on the device.

What ``NuscenesData.get_input_data`` does between ``Image.open`` and the model (streamingflow/datas/NuscenesData.py:251-269):
``resize_and_crop_image`` (PIL's antialiased BILINEAR resize, then ``crop``; utils/geometry.py:9-13), ``ToTensor``, ``Normalize`` with the
ImageNet statistics (:77-79), and ``update_intrinsics`` (utils/geometry.py:16-37).  The image part is ONE library call
(``sf_image_frontend_fwd``, csrc/image_frontend.hip), bit for bit what PIL and torch compute on the CPU; the intrinsics are a handful of
elementwise torch operations.  The resize dimensions and the crop follow the reference's own rule
(``get_resizing_and_cropping_parameters``, :165-187), its ``int(...)`` truncations included.  Nothing here allocates on the host or
synchronises after the first call on a device, so a forward can be recorded into a graph in front of the encoder.
"""
import torch

from . import runtime

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


class ImageFrontend(torch.nn.Module):
    def __init__(self, original=(900, 1600), resize_scale=0.3, top_crop=46, final_dim=(224, 480), mean=MEAN, std=STD):
        super().__init__()
        self.original, self.final_dim = (int(original[0]), int(original[1])), (int(final_dim[0]), int(final_dim[1]))
        self.resize_scale, self.top_crop = resize_scale, int(top_crop)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        (oh, ow), (fh, fw) = self.original, self.final_dim
        # get_resizing_and_cropping_parameters: (width, height) as PIL takes them, and (left, top, right, bottom)
        self.resize_dims = (int(ow * resize_scale), int(oh * resize_scale))
        crop_w = int(max(0, (self.resize_dims[0] - fw) / 2))
        self.crop = (crop_w, self.top_crop, crop_w + fw, self.top_crop + fh)
        self._plan_host = None
        self._plan_dev = {}      # device -> the plan's copy there, uploaded on first use

    @classmethod
    def from_cfg(cls, cfg, **kw):
        """From ``cfg.IMAGE.{ORIGINAL_HEIGHT, ORIGINAL_WIDTH, RESIZE_SCALE, TOP_CROP, FINAL_DIM}``; a key the configuration does not carry
        takes the reference's default (streamingflow/config.py:65-69)."""
        im = getattr(cfg, "IMAGE", None)
        g = lambda k, d: getattr(im, k, d)
        return cls(original=(g("ORIGINAL_HEIGHT", 900), g("ORIGINAL_WIDTH", 1600)), resize_scale=g("RESIZE_SCALE", 0.3),
                   top_crop=g("TOP_CROP", 46), final_dim=tuple(g("FINAL_DIM", (224, 480))), **kw)

    def plan(self, device):
        """(host blob, its copy on ``device``): built once, uploaded once per device."""
        if self._plan_host is None:
            (oh, ow), (rw, rh) = self.original, self.resize_dims
            self._plan_host = runtime.image_frontend_plan(oh, ow, rh, rw, self.crop, self.mean, self.std)
        device = torch.device(device)
        if device not in self._plan_dev:
            self._plan_dev[device] = self._plan_host.to(device)
        return self._plan_host, self._plan_dev[device]

    def __getstate__(self):      # the device copies stay with this process
        d = dict(self.__dict__)
        d["_plan_dev"] = {}
        return d

    def images(self, raw, planar=True, with_u8=False):
        """raw [..., Hs, Ws, 3] uint8 -> fp32 [..., 3, h, w] (planar) or [..., h, w, 3]; with_u8: also the resized, cropped bytes
        [..., h, w, 3] before the normalisation."""
        runtime.require_cuda(raw)
        if raw.dtype != torch.uint8 or raw.dim() < 3 or raw.shape[-1] != 3 or tuple(raw.shape[-3:-1]) != self.original:
            raise RuntimeError(f"ImageFrontend: expected uint8 frames [..., {self.original[0]}, {self.original[1]}, 3], got {raw.dtype} "
                               f"{tuple(raw.shape)}")
        lead, (h, w) = tuple(raw.shape[:-3]), self.final_dim
        src = raw.contiguous().view(-1, *raw.shape[-3:])
        n = src.shape[0]
        out = torch.empty((n, 3, h, w) if planar else (n, h, w, 3), dtype=torch.float32, device=raw.device)
        u8 = torch.empty((n, h, w, 3), dtype=torch.uint8, device=raw.device) if with_u8 else None
        if n:
            host, dev = self.plan(raw.device)
            runtime.image_frontend(src, host, dev, out, planar, u8)
        out = out.view(*lead, *out.shape[1:])
        return (out, u8.view(*lead, h, w, 3)) if with_u8 else out

    def intrinsics(self, K):
        """``update_intrinsics`` on [..., 3, 3]: the resize scales the focal lengths and the principal point, the crop shifts the latter."""
        K = K.clone()
        K[..., 0, 0] *= self.resize_scale
        K[..., 0, 2] *= self.resize_scale
        K[..., 1, 1] *= self.resize_scale
        K[..., 1, 2] *= self.resize_scale
        K[..., 0, 2] -= self.crop[0]
        K[..., 1, 2] -= self.crop[1]
        return K

    def forward(self, raw, intrinsics=None):
        """(image [..., 3, h, w] fp32, updated intrinsics or None)"""
        return self.images(raw), (self.intrinsics(intrinsics) if intrinsics is not None else None)
