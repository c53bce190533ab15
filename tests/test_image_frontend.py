"""CPU: the camera image front end's host side (streamingflow_amd/image_frontend.py, csrc/image_frontend.hip: sf_resample_table,
sf_image_frontend_plan) and the numpy restatement the GPU tests compare against (tests/image_frontend_util.py):
  * the library's resample tables equal the restatement's, entry for entry, and its normalise table equals torch's CPU arithmetic;
  * the restatement equals the fixture the reference's own functions wrote (tools/gen_image_frontend_golden.py), bitwise, and — where the
    reference tree and PIL are present — the reference function itself at the shipped geometry;
  * ImageFrontend.from_cfg reproduces the reference's resize dimensions and crop; refusals; the model's error for uint8 frames without
    a front end."""
import ctypes

import numpy as np
import pytest
import torch

import image_frontend_util as U
from util import gold, refimport

PAIRS = [(1600, 480), (900, 270), (80, 24), (45, 13), (53, 15), (37, 11), (96, 48), (40, 40), (30, 51)]


def _lib():
    from streamingflow_amd import build, _lib
    build.build()
    return _lib, _lib.lib()


def _table(L, i, o):
    ks = L.sf_resample_ksize(i, o)
    bounds, k = np.full((o, 2), -1, np.int32), np.full((o, ks), -1, np.int32)
    assert L.sf_resample_table(i, o, bounds.ctypes.data, k.ctypes.data) == 0
    return bounds, k, ks


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%dto%d" % p)
def test_host_table_equals_the_restatement(pair):
    _, L = _lib()
    bounds, k, ks = _table(L, *pair)
    rb, rk, rks = U.table(*pair)
    assert ks == rks and np.array_equal(bounds, rb) and np.array_equal(k, rk)
    assert (bounds[:, 1] >= 1).all() and (bounds[:, 0] >= 0).all() and (bounds.sum(1) <= pair[0]).all()
    assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(1)) >= 0).all()      # what the kernel's tile ranges rely on


def test_tap_counts_are_the_derived_ones():
    _, L = _lib()
    assert [L.sf_resample_ksize(i, o) for i, o in [(80, 24), (96, 48), (40, 40), (30, 51), (800, 100)]] == [9, 5, 3, 3, 17]
    assert L.sf_resample_ksize(0, 4) == 0 and L.sf_resample_ksize(4, 0) == 0


def _plan(Hs, Ws, dims, box, mean=U.MEAN, std=U.STD):
    from streamingflow_amd import runtime
    return runtime.image_frontend_plan(Hs, Ws, dims[1], dims[0], box, mean, std)


def test_plan_holds_both_tables_and_torchs_normalise_table():
    _lib()
    blob = _plan(900, 1600, (480, 270), (0, 46, 480, 270)).numpy()
    assert blob[1:11].tolist() == [900, 1600, 270, 480, 0, 46, 480, 224, 9, 9] and blob[19] == len(blob)
    for (i, o), b_off, k_off in (((1600, 480), blob[14], blob[15]), ((900, 270), blob[16], blob[17])):
        rb, rk, ks = U.table(i, o)
        assert np.array_equal(blob[b_off:b_off + 2 * o].reshape(o, 2), rb) and np.array_equal(blob[k_off:k_off + o * ks].reshape(o, ks), rk)
    lut = torch.from_numpy(blob[blob[18]:blob[18] + 768].copy()).view(torch.float32).view(3, 256)
    every_byte = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)      # [h = 256][w = 1][3]
    assert torch.equal(lut, U.normalise(every_byte)[:, :, 0])
    # a workgroup's LDS fits the 64 KB a launch may ask for, at the shipped geometry and at the tap cap
    assert 0 < blob[20] <= 64 * 1024 and blob[21] == 1
    wide = _plan(1600, 1600, (100, 100), (0, 0, 100, 100)).numpy()
    assert wide[9] == wide[10] == 33 and 0 < wide[20] <= 64 * 1024
    assert _plan(37, 53, (15, 11), (0, 0, 15, 11)).numpy()[21] == 0      # 159-byte rows: the byte-by-byte form


@pytest.mark.parametrize("name", list(U.CASES))
def test_restatement_equals_the_reference_fixture(name):
    g = gold("image_frontend.npz")
    src, dims, box, scale = U.case(name)
    assert np.array_equal(src, g[name + ".src"])
    u8, f32 = U.expected(name)
    assert u8.dtype == np.uint8 and np.array_equal(u8, g[name + ".u8"])
    assert torch.equal(f32, torch.from_numpy(g[name + ".f32"]))
    K = U.intrinsics(list(U.CASES).index(name))
    assert torch.equal(K, torch.from_numpy(g[name + ".K"]))
    assert torch.equal(U.update_intrinsics(K, box[1], box[0], scale, scale), torch.from_numpy(g[name + ".K_out"]))


def test_fixture_covers_what_it_is_for():
    g = gold("image_frontend.npz")
    pad = g["pad_all_sides.u8"]
    assert pad.shape == (2, 29, 160, 3) and not pad[:, :9].any() and not pad[:, :, :70].any() and not pad[:, 22:].any() and not pad[:, :, 94:].any()
    assert pad[:, 9:22, 70:94].any()
    zero = U.normalise(np.zeros((1, 1, 3), np.uint8))[:, 0, 0]
    assert torch.equal(torch.from_numpy(g["pad_all_sides.f32"])[0, :, 0, 0], zero)      # padding is (0 - mean) / std
    assert (g["white.u8"] == 255).all() and (g["black.u8"] == 0).all()
    assert set(np.unique(g["odd_checker.src"])) == {0, 255}


def test_restatement_equals_the_reference_function_at_the_shipped_geometry():
    Image = pytest.importorskip("PIL.Image")
    if not refimport.available():
        pytest.skip("reference tree not present")
    refimport.install()
    from streamingflow.utils.geometry import resize_and_crop_image
    src = U.source(2024, 900, 1600)
    dims, box = U.geometry((900, 1600), 0.3, 46, (224, 480))
    want = np.asarray(resize_and_crop_image(Image.fromarray(src), resize_dims=dims, crop=box))
    assert want.shape == (224, 480, 3) and np.array_equal(U.resize_and_crop(src, dims, box), want)


def test_from_cfg_reproduces_the_reference_geometry():
    from streamingflow_amd import ImageFrontend
    from streamingflow_amd.models.streamingflow import default_cfg
    from types import SimpleNamespace as NS
    fe = ImageFrontend.from_cfg(default_cfg())
    assert fe.resize_dims == (480, 270) and fe.crop == (0, 46, 480, 270) and fe.original == (900, 1600) and fe.final_dim == (224, 480)
    assert ImageFrontend.from_cfg(NS(IMAGE=NS(FINAL_DIM=(224, 480)))).crop == (0, 46, 480, 270)      # the reference's defaults for missing keys
    assert (fe.resize_dims, fe.crop) == U.geometry((900, 1600), 0.3, 46, (224, 480))
    # the cases where the reference prints "Zero padding ...": a resized image narrower and shorter than the final one
    pad = ImageFrontend(original=(45, 80), resize_scale=0.3, top_crop=2, final_dim=(16, 32))
    assert pad.resize_dims == (24, 13) and pad.crop == (0, 2, 32, 18) == U.geometry((45, 80), 0.3, 2, (16, 32))[1]
    wide = ImageFrontend(original=(45, 80), resize_scale=0.3, top_crop=0, final_dim=(8, 15))
    assert wide.crop == (4, 0, 19, 8)
    K = U.intrinsics(3).expand(2, 3, 3, 3)
    assert torch.equal(fe.intrinsics(K), U.update_intrinsics(K, 46, 0, 0.3, 0.3)) and torch.equal(K[0, 0], U.intrinsics(3))
    host = fe.plan("cpu")[0]
    assert host is fe.plan("cpu")[0] and host[1:9].tolist() == [900, 1600, 270, 480, 0, 46, 480, 224]


def test_refusals():
    lib, L = _lib()
    INV, UNS = lib.SF_ERR_INVALID, lib.SF_ERR_UNSUPPORTED
    assert lib.SF_IMAGE_FRONTEND_MAX_TAPS == 33
    big = np.zeros(1 << 16, np.int32)
    assert L.sf_resample_table(0, 4, big.ctypes.data, big.ctypes.data) == INV
    assert L.sf_resample_table(8, 4, None, big.ctypes.data) == INV and L.sf_resample_table(8, 4, big.ctypes.data, None) == INV
    assert L.sf_resample_table(1700, 100, big.ctypes.data, big.ctypes.data) == UNS      # 17 x: 35 taps
    assert L.sf_resample_table(1600, 100, big.ctypes.data, big.ctypes.data) == 0        # 16 x: 33 taps
    m = (ctypes.c_float * 3)(*U.MEAN)
    s = (ctypes.c_float * 3)(*U.STD)
    geo = (45, 80, 13, 24, 2, 1, 22, 12)
    need = L.sf_image_frontend_plan_bytes(*geo)
    assert need > 0 and need % 4 == 0
    blob = np.full(need // 4, -1, np.int32)
    plan = lambda g=geo, mean=m, std=s, p=blob.ctypes.data, nb=need: L.sf_image_frontend_plan(*g, mean, std, p, nb)
    assert plan() == 0
    assert plan(mean=None) == plan(std=None) == plan(p=None) == plan(nb=need - 4) == INV
    for bad in [(0, 80, 13, 24, 2, 1, 22, 12), (45, 0, 13, 24, 2, 1, 22, 12), (45, 80, 0, 24, 2, 1, 22, 12), (45, 80, 13, -1, 2, 1, 22, 12),
                (45, 80, 13, 24, 2, 1, 2, 12), (45, 80, 13, 24, 2, 12, 22, 12), (45, 40000, 13, 24, 2, 1, 22, 12)]:
        assert L.sf_image_frontend_plan_bytes(*bad) == 0 and plan(g=bad) == INV, bad
    many = (1700, 80, 100, 24, 0, 0, 24, 100)
    assert L.sf_image_frontend_plan_bytes(*many) == 0 and plan(g=many) == UNS
    assert L.sf_image_frontend_plan_bytes(800, 800, 100, 100, 0, 0, 100, 100) > 0      # 8 x is inside the cap
    # the forward call: every refusal comes before anything is enqueued, so these run without a GPU
    A = 1 << 20      # an aligned placeholder address nobody reads
    fwd = lambda src=A, ph=blob.ctypes.data, pd=A, out=A, n=1, Hs=45, Ws=80, h=11, w=20: \
        L.sf_image_frontend_fwd(src, ph, pd, out, 1, None, n, Hs, Ws, h, w, None)
    assert fwd(src=None) == fwd(ph=None) == fwd(pd=None) == fwd(out=None) == INV
    assert fwd(n=0) == fwd(Hs=0) == fwd(Ws=0) == fwd(h=0) == fwd(w=0) == INV
    assert fwd(Hs=46) == fwd(Ws=96) == fwd(h=12) == fwd(w=21) == INV      # not the plan's sizes
    assert fwd(src=A + 8) == fwd(pd=A + 4) == INV                          # 240-byte rows are staged 16 bytes per lane: src must be aligned
    assert fwd(ph=np.zeros(64, np.int32).ctypes.data) == INV              # not a plan


def test_uint8_frames_without_a_front_end_raise():
    from streamingflow_amd.models.streamingflow import default_cfg, streamingflow
    cfg = default_cfg()
    cfg.MODEL.MODALITY.USE_LIDAR = False
    cfg.LIFT.X_BOUND, cfg.LIFT.Y_BOUND = [-4.0, 4.0, 0.5], [-4.0, 4.0, 0.5]
    cfg.IMAGE.FINAL_DIM = (32, 48)
    net = streamingflow(cfg)
    assert net.image_frontend is None
    fe = object()
    assert streamingflow(cfg, frontend=fe).image_frontend is fe
    raw = torch.zeros((1, 3, 2, 110, 160, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no image front end"):
        net(raw, torch.eye(3).expand(1, 3, 2, 3, 3), torch.eye(4).expand(1, 3, 2, 4, 4), torch.zeros(1, 3, 6))
