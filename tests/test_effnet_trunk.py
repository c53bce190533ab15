"""CPU: the EfficientNet trunk's structure (streamingflow_amd/models/efficientnet.py) against the architecture restated in
tests/effnet_util.py, its state_dict keys, its workspace layout (sf_effnet_trunk_ws_bytes / sf_mbconv_ws_bytes, csrc/effnet.hip) and
the two descriptions of the endpoint walk.  Nothing here launches a kernel."""
import ctypes

import numpy as np
import pytest
import torch

import effnet_util as U
import encoder_neck_util as NU
from streamingflow_amd import _lib
from streamingflow_amd.models import efficientnet as E
from streamingflow_amd.models.encoder import BREAK_INDEX, REDUCTION_CHANNEL, EfficientNetEndpoints

VERSIONS = ("b0", "b4", "b7")


def _tlbr(pad):      # F.pad order (left, right, top, bottom) -> the module's (top, left, bottom, right)
    l, r, t, b = pad
    return (t, l, b, r)


@pytest.mark.parametrize("downsample", [8, 16])
@pytest.mark.parametrize("version", VERSIONS)
def test_structure(version, downsample):
    t = E.EfficientNetTrunk(version, downsample)
    want = U.blocks_of(version, downsample)
    assert len(t._blocks) == len(want) == {8: BREAK_INDEX[version] + 1, 16: {"b0": 16, "b4": 32, "b7": 55}[version]}[downsample]
    assert [(a.k, a.stride, a.cin, a.cout, a.expand, a.cse) for a in t.blocks_args] == want
    assert [a.skip for a in t.blocks_args] == [s == 1 and ci == co for _, s, ci, co, _, _ in want]
    assert t.c_stem == U.filters(32, U.VERSIONS[version][0])
    # the break index is the last block of stage 5: the next block of the full version opens stage 6 with stride 2
    full = U.blocks_of(version, 16)
    outs5 = U.filters(112, U.VERSIONS[version][0])
    assert full[BREAK_INDEX[version]][3] == outs5 and full[BREAK_INDEX[version] + 1][1:3] == (2, outs5)
    # endpoint channels on the shipped image size
    _, hi, lo = t.plan(224, 480)
    k = t.index
    assert (hi[0], lo[0]) == (REDUCTION_CHANNEL[version][k + 1], REDUCTION_CHANNEL[version][k])
    assert hi[1:] == (224 // (2 * downsample), 480 // (2 * downsample)) and lo[1:] == (224 // downsample, 480 // downsample)
    # the four pads of every layer: static from the nominal size, dynamic from the input
    ref = U.RefTrunk({}, version, downsample)
    assert t.pads() == t.pads(37, 51) == [_tlbr(p) for p in ref.static_pads]
    dyn = E.EfficientNetTrunk(version, downsample, image_size=None)
    for H, W in ((37, 51), (224, 480)):
        h, w, want_pads = H, W, []
        for kk, stride in [(3, 2)] + [(b[0], b[1]) for b in want]:
            pad, (h, w) = U.pad4(h, w, kk, stride)
            want_pads.append(_tlbr(pad))
        assert dyn.pads(H, W) == want_pads
    assert dyn.pads(37, 51) != t.pads()


def test_b4_numbers_of_the_architecture():
    t = E.EfficientNetTrunk("b4")
    assert t.c_stem == 48 and t.image_size == (380, 380)
    stage_out = []
    for a in t.blocks_args:
        if not stage_out or stage_out[-1] != a.cout:
            stage_out.append(a.cout)
    assert stage_out == [24, 32, 56, 112, 160]
    pads = t.pads()
    assert pads[0] == (0, 0, 1, 1)                                    # stem at 380: (0, 1) on both axes
    first = {a.cout: i for i, a in reversed(list(enumerate(t.blocks_args)))}
    assert pads[1 + first[32]] == (0, 0, 1, 1)                        # stride-2 3x3 at 190
    assert pads[1 + first[56]] == (2, 2, 2, 2)                        # stride-2 5x5 at 95
    assert pads[1 + first[112]] == (0, 0, 1, 1)                       # stride-2 3x3 at 48
    assert pads[1 + first[160]] == (2, 2, 2, 2)                       # stride-1 5x5 at 24
    assert [a.cse for a in t.blocks_args[:4]] == [12, 6, 6, 8]     # a quarter of the block's INPUT filters: 48, 24, 24, 32
    assert E.EfficientNetTrunk("b0").image_size == (224, 224) and E.EfficientNetTrunk("b7").image_size == (600, 600)
    with pytest.raises(NotImplementedError):
        E.EfficientNetTrunk("b3")


@pytest.mark.parametrize("downsample", [8, 16])
@pytest.mark.parametrize("version", VERSIONS)
def test_state_dict_keys(version, downsample):
    t = E.EfficientNetTrunk(version, downsample)
    sd = t.state_dict()
    assert list(sd) == U.expected_keys(version, downsample)
    assert not any(k.startswith(("_conv_head", "_bn1", "_fc")) for k in sd)
    assert not any(k.startswith("_blocks.%d." % len(t._blocks)) for k in sd)
    for i, (k, stride, cin, co, e, se) in enumerate(U.blocks_of(version, downsample)):
        p = "_blocks.%d." % i
        cexp = cin * e
        assert tuple(sd[p + "_depthwise_conv.weight"].shape) == (cexp, 1, k, k)
        assert tuple(sd[p + "_se_reduce.weight"].shape) == (se, cexp, 1, 1) and tuple(sd[p + "_se_expand.bias"].shape) == (cexp,)
        assert tuple(sd[p + "_project_conv.weight"].shape) == (co, cexp, 1, 1)
        assert (p + "_expand_conv.weight" in sd) == (e != 1)
    assert all(m.eps == 1e-3 for m in t.modules() if isinstance(m, torch.nn.BatchNorm2d))
    biased = {n for n, m in t.named_modules() if isinstance(m, torch.nn.Conv2d) and m.bias is not None}
    assert biased == {"_blocks.%d.%s" % (i, s) for i in range(len(t._blocks)) for s in ("_se_reduce", "_se_expand")}


def test_checkpoint_slice_loads_strict_through_the_encoder():
    trunk = E.EfficientNetTrunk("b4")
    enc = NU.build("b4", 48, backbone=trunk)      # hashed neck, the trunk as constructed
    keys = list(enc.state_dict())
    assert sorted(k[len("backbone."):] for k in keys if k.startswith("backbone.")) == sorted(U.expected_keys("b4", 8))
    sd = {k: v.clone() for k, v in enc.state_dict().items()}
    sd.update(U.state("b4"))
    enc.load_state_dict(sd, strict=True)
    got = enc.state_dict()
    assert all(torch.equal(got[k], sd[k]) for k in keys)
    assert torch.equal(trunk._blocks[21]._bn2.running_var, U.state("b4")["backbone._blocks.21._bn2.running_var"])
    for extra in ("backbone._conv_head.weight", "backbone._blocks.22._bn2.weight"):
        with pytest.raises(RuntimeError):
            enc.load_state_dict(dict(sd, **{extra: torch.zeros(1)}), strict=True)


def test_inference_only_and_no_cpu_fallback():
    t = E.EfficientNetTrunk("b0")
    with pytest.raises(RuntimeError, match="inference-only"):
        t.train()._pack(t.pads())
    with pytest.raises(RuntimeError, match="MI355X"):
        t.eval()(torch.zeros(1, 3, 32, 32))
    with pytest.raises(RuntimeError):
        t._blocks[0](torch.zeros(1, 32, 8, 8))


def test_wiring_helper_supplies_the_missing_keys():
    from streamingflow_amd.models import streamingflow as SF
    cfg = SF.default_cfg()
    assert not hasattr(cfg.MODEL.ENCODER, "NAME") and not hasattr(cfg.MODEL.ENCODER, "USE_DEPTH_DISTRIBUTION")
    enc = SF.camera_encoder(cfg)
    assert isinstance(enc.backbone, E.EfficientNetTrunk) and enc.backbone.version == "b4" and enc.backbone.downsample == 8
    assert (enc.D, enc.C, enc.c_hi, enc.c_lo) == (48, 64, 160, 56)
    assert not hasattr(cfg.MODEL.ENCODER, "NAME")      # the caller's configuration is not written to
    b0 = SF.camera_encoder(cfg, "b0", image_size=None)
    assert b0.backbone.version == "b0" and b0.backbone.image_size is None and b0.c_hi == 112


@pytest.mark.parametrize("version,shape,size", [("b4", (2, 3, 32, 48), "nominal"), ("b0", (1, 3, 32, 32), "nominal"), ("b4", (1, 3, 37, 51), None)])
def test_the_two_descriptions_of_the_walk_agree(version, shape, size):
    """The restatement walked by its own endpoint rule returns the tensors ``EfficientNetEndpoints`` (the reference's walk, with the
    drop-connect bookkeeping) selects on it."""
    ref = U.RefTrunk(U.trunk_state(version), version, 8, size, torch.float32)
    x = U.images("walk", shape)
    hi, lo = ref.walk(x)
    with torch.no_grad():
        hi2, lo2 = EfficientNetEndpoints(ref, version, 8)(x)
    assert torch.equal(hi, hi2) and torch.equal(lo, lo2)
    t = E.EfficientNetTrunk(version, 8, image_size=E.NOMINAL if size == "nominal" else size)
    _, s_hi, s_lo = t.plan(*shape[2:])
    assert tuple(hi.shape[1:]) == s_hi and tuple(lo.shape[1:]) == s_lo


# ---- workspace layout: the pattern of tests/test_workspace_layout.py -------------------------------------------------------------------
def _query(version, downsample, n, H, W, size=E.NOMINAL):
    t = E.EfficientNetTrunk(version, downsample, image_size=size)
    w, keep = U.placeholder_trunk(version, downsample, t.pads(H, W))
    return _lib.lib().sf_effnet_trunk_ws_bytes(ctypes.byref(w), n, H, W), w, keep


def test_workspace_query_is_monotone_and_is_the_layout():
    base, w, keep = _query("b4", 8, 2, 64, 96)
    assert base > 0
    for n, H, W in ((3, 64, 96), (2, 72, 96), (2, 64, 104), (18, 224, 480)):
        assert _query("b4", 8, n, H, W)[0] > base, (n, H, W)
    # what the layout holds, from the issue's description: two activation buffers of the largest block output (or the stem's), the
    # largest expanded tensor, the largest depthwise output, sums (8 bytes) and gate (4 bytes) per image and expanded channel; every
    # buffer rounded up to 64 floats
    al = lambda floats: (floats + 63) // 64 * 64 * 4
    t = E.EfficientNetTrunk("b4")
    n, H, W = 2, 64, 96
    shapes, _ = E.walk_shapes(t.blocks_args, t.c_stem, t.pads(), H, W)
    x_max = max(n * c * h * ww for c, h, ww in shapes)
    e_max = max(n * a.cin * a.expand * s[1] * s[2] for a, s in zip(t.blocks_args, shapes) if a.expand != 1)
    d_max = max(n * a.cin * a.expand * s[1] * s[2] for a, s in zip(t.blocks_args, shapes[1:]))
    nc = max(n * a.cin * a.expand for a in t.blocks_args)
    assert base == 2 * al(x_max) + al(e_max) + al(d_max) + al(2 * nc) + al(nc)
    # nothing of it depends on pointers
    w.stem_w = 0
    assert _lib.lib().sf_effnet_trunk_ws_bytes(ctypes.byref(w), 2, 64, 96) == base
    # sizes that cannot be walked give 0
    assert _lib.lib().sf_effnet_trunk_ws_bytes(ctypes.byref(w), 0, 64, 96) == 0
    assert _lib.lib().sf_effnet_trunk_ws_bytes(ctypes.byref(w), 2, 8, 8) == 0      # too small to reach reduction_4
    assert _lib.lib().sf_effnet_trunk_ws_bytes(None, 2, 64, 96) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="placeholder tensor pointers: host only")
@pytest.mark.parametrize("version,n,H,W", [("b4", 1, 32, 48), ("b0", 3, 64, 64)])
def test_short_workspace_and_unsupported_blocks_are_refused_before_anything_runs(version, n, H, W):
    from ws_layout_util import HOLE
    L = _lib.lib()
    need, w, keep = _query(version, 8, n, H, W)
    ws = np.full(1024, 7.0, dtype=np.float32)
    ptr = ws.ctypes.data_as(ctypes.c_void_p)
    call = lambda p, b: L.sf_effnet_trunk_fwd(ctypes.byref(w), HOLE, 1, HOLE, HOLE, n, H, W, p, b, None)
    for short in (need - 256, need // 2, 0):
        assert call(ptr, short) == _lib.SF_ERR_WORKSPACE, short
    assert call(None, need) == _lib.SF_ERR_WORKSPACE
    blk = keep[1]
    bneed = L.sf_mbconv_ws_bytes(ctypes.byref(blk), n, H // 2, W // 2)
    assert bneed > 256
    for short in (bneed - 256, 0):
        assert L.sf_mbconv_fwd(ctypes.byref(blk), HOLE, HOLE, n, H // 2, W // 2, ptr, short, None) == _lib.SF_ERR_WORKSPACE
    for field, bad in (("k", 7), ("k", 4), ("stride", 3), ("cexp", blk.cexp + 4), ("cout", blk.cout + 4)):
        good = getattr(blk, field)
        setattr(blk, field, bad)
        assert call(ptr, need) == _lib.SF_ERR_UNSUPPORTED, (field, bad)
        assert L.sf_mbconv_fwd(ctypes.byref(blk), HOLE, HOLE, n, H // 2, W // 2, ptr, bneed, None) == _lib.SF_ERR_UNSUPPORTED
        setattr(blk, field, good)
    assert float(np.abs(ws - 7.0).max()) == 0.0
