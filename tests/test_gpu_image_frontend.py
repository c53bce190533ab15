"""GPU: the camera image front end (streamingflow_amd/image_frontend.py -> sf_image_frontend_fwd, csrc/image_frontend.hip) against the
numpy restatement of tests/image_frontend_util.py, which tests/test_image_frontend.py pins to the reference's own functions.  Everything
is integer arithmetic and a table lookup, so every comparison is bitwise: the resized and cropped bytes, and the normalised floats in
both output layouts."""
import numpy as np
import pytest
import torch

import image_frontend_util as U

pytestmark = pytest.mark.gpu


def device_run(src, dims, box, planar, mean=U.MEAN, std=U.STD):
    """(out fp32 as [n][3][h][w], out_u8 [n][h][w][3]) of one library call on src [n][Hs][Ws][3] uint8 (numpy)."""
    from streamingflow_amd import runtime
    n, Hs, Ws = src.shape[:3]
    h, w = box[3] - box[1], box[2] - box[0]
    host = runtime.image_frontend_plan(Hs, Ws, dims[1], dims[0], box, mean, std)
    dev, s = host.cuda(), torch.from_numpy(src).cuda()
    out = torch.full((n, 3, h, w) if planar else (n, h, w, 3), float("nan"), device="cuda")
    u8 = torch.full((n, h, w, 3), 77, dtype=torch.uint8, device="cuda")
    runtime.image_frontend(s, host, dev, out, planar, u8)
    torch.cuda.synchronize()
    return (out if planar else out.permute(0, 3, 1, 2)).cpu(), u8.cpu()


@pytest.mark.parametrize("planar", [True, False], ids=["planar", "interleaved"])
@pytest.mark.parametrize("name", list(U.CASES))
def test_cases_bitwise(name, planar):
    src, dims, box, _ = U.case(name)
    want_u8, want = U.expected(name)
    got, got_u8 = device_run(src, dims, box, planar)
    assert np.array_equal(got_u8.numpy(), want_u8)
    assert torch.equal(got, want)
    if name.startswith("pad_"):      # the padded pixels are (0 - mean) / std, and there are some
        outside = torch.ones(want_u8.shape[1:3], dtype=torch.bool)
        outside[max(-box[1], 0):min(dims[1], box[3]) - box[1], max(-box[0], 0):min(dims[0], box[2]) - box[0]] = False
        zero = U.normalise(np.zeros((1, 1, 3), np.uint8))[:, 0, 0]
        assert int(outside.sum()) > 0 and torch.equal(got[0][:, outside], zero[:, None].expand(3, int(outside.sum())))


def test_without_the_byte_output_and_with_other_statistics():
    from streamingflow_amd import runtime
    src, dims, box, _ = U.case("s03_inside")
    mean, std = (0.5, 0.25, 0.125), (0.5, 1.0, 0.3)
    host = runtime.image_frontend_plan(45, 80, dims[1], dims[0], box, mean, std)
    out = torch.empty((3, 3, 11, 20), device="cuda")
    runtime.image_frontend(torch.from_numpy(src).cuda(), host, host.cuda(), out, True, None)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), U.normalise(U.expected("s03_inside")[0], mean, std))


def test_shipped_geometry_one_frame():
    """900 x 1600 -> 480 x 270 -> crop (0, 46, 480, 270): 28 x 8 tiles, the 16-bytes-per-lane staging, the last tile column half empty;
    through the module, which also gives the byte image."""
    from streamingflow_amd import ImageFrontend
    from streamingflow_amd.models.streamingflow import default_cfg
    fe = ImageFrontend.from_cfg(default_cfg())
    src = U.source(2024, 900, 1600)
    want_u8 = U.resize_and_crop(src, fe.resize_dims, fe.crop)[None]
    want = U.normalise(want_u8)
    raw = torch.from_numpy(src).cuda()
    image, u8 = fe.images(raw[None], with_u8=True)
    inter = fe.images(raw[None], planar=False)
    K = U.intrinsics(0).cuda()
    image2, K2 = fe(raw, K)
    torch.cuda.synchronize()
    assert np.array_equal(u8.cpu().numpy(), want_u8)
    assert tuple(image.shape) == (1, 3, 224, 480) and torch.equal(image.cpu(), want)
    assert tuple(inter.shape) == (1, 224, 480, 3) and torch.equal(inter.cpu().permute(0, 3, 1, 2), want)
    assert tuple(image2.shape) == (3, 224, 480) and torch.equal(image2.cpu(), want[0])      # no leading dimension
    assert torch.equal(K2.cpu(), U.update_intrinsics(U.intrinsics(0), 46, 0, 0.3, 0.3))


def test_graph_capture_equals_eager():
    from streamingflow_amd import ImageFrontend
    fe = ImageFrontend(original=(45, 80), resize_scale=0.3, top_crop=1, final_dim=(11, 24))
    a, b = (torch.from_numpy(np.stack([U.source(s + i, 45, 80) for i in range(2)])).cuda() for s in (500, 600))
    eager_a, eager_b = fe.images(a), fe.images(b)      # also uploads the plan, outside the capture
    buf = a.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fe.images(buf)
    buf.copy_(b)
    out.fill_(-7.0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_b) and not torch.equal(eager_a, eager_b)
    assert torch.equal(eager_b.cpu(), U.normalise(np.stack([U.resize_and_crop(s, (24, 13), (0, 1, 24, 12)) for s in b.cpu().numpy()])))


def test_model_takes_raw_frames():
    """Camera-only model with the device encoder: uint8 frames and the cameras' own intrinsics give bitwise the depth prediction that the
    front end's outputs give when passed as float images — the model adds nothing of its own in between."""
    from test_gpu_end_to_end import small_cfg
    from lift_util import rig_cameras
    from streamingflow_amd import ImageFrontend
    from streamingflow_amd.models import streamingflow as SF
    cfg, _ = small_cfg()
    cfg.MODEL.MODALITY.USE_LIDAR = False
    cfg.LIFT.D_BOUND = [2.0, 10.0, 1.0]      # 8 depth bins: the neck takes multiples of 4
    C = 64
    cfg.MODEL.ENCODER.OUT_CHANNELS = cfg.MODEL.TEMPORAL_MODEL.START_OUT_CHANNELS = cfg.MODEL.DISTRIBUTION.LATENT_DIM = C
    cfg.MODEL.SMALL_ENCODER.FILTER_SIZE = C
    cfg.IMAGE.ORIGINAL_HEIGHT, cfg.IMAGE.ORIGINAL_WIDTH, cfg.IMAGE.TOP_CROP = 110, 160, 1      # x 0.3 -> 48 x 33 -> crop (0, 1, 48, 33)
    fe = ImageFrontend.from_cfg(cfg)
    assert fe.resize_dims == (48, 33) and fe.crop == (0, 1, 48, 33)
    torch.manual_seed(7)
    net = SF.streamingflow(cfg, encoder=SF.camera_encoder(cfg, "b0"), frontend=fe).eval().cuda()
    assert net.image_frontend is fe
    b, s, n = 1, 3, 2
    intr, extr, ego = (t.cuda() for t in rig_cameras(s, n, (32, 48), 5))
    raw_K = intr.clone()      # the intrinsics of the 110 x 160 frames whose update gives about the rig's
    raw_K[..., 0, 0] /= 0.3
    raw_K[..., 1, 1] /= 0.3
    raw_K[..., 0, 2] = (intr[..., 0, 2] + fe.crop[0]) / 0.3
    raw_K[..., 1, 2] = (intr[..., 1, 2] + fe.crop[1]) / 0.3
    raw = torch.from_numpy(np.stack([U.source(700 + i, 110, 160) for i in range(b * s * n)])).view(b, s, n, 110, 160, 3).cuda()
    cts = torch.tensor([[-1.0, -0.5, 0.0]], dtype=torch.float64)
    tts = torch.tensor([[0.5, 1.0, 1.5, 2.0]], dtype=torch.float64)
    with torch.no_grad():
        image, K = fe(raw, raw_K)
        assert tuple(image.shape) == (b, s, n, 3, 32, 48) and image.dtype == torch.float32 and tuple(K.shape) == tuple(raw_K.shape)
        want = net(image, K, extr, ego, None, cts, None, None, tts)["depth_prediction"]
        got = net(raw, raw_K, extr, ego, None, cts, None, None, tts)["depth_prediction"]
        torch.cuda.synchronize()
        assert tuple(got.shape) == (b, s, n, 8, 4, 6) and bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
        assert torch.equal(got, want)
        net.image_frontend = None
        with pytest.raises(RuntimeError, match="no image front end"):
            net(raw, raw_K, extr, ego, None, cts, None, None, tts)
