"""GPU: the rig's affines on the device (sf_rig_affines_fwd, csrc/rig_affines.hip; LiftSplat.rig_affines_device / device_affines /
check_rig) against the float64 oracle of tests/rig_util.py, with bad cameras, inside the lift against the oracle chain of
tests/test_gpu_lift.py, and — what DESIGN.md §6b N2 records as impossible with torch.inverse — the lift recorded into a graph from RAW
intrinsics and replayed on another rig."""
import ctypes

import numpy as np
import pytest
import torch

import rig_util as RU
from util import cases, maxabs
from oracle import lift_splat as LS

pytestmark = pytest.mark.gpu
TOL = 1e-5      # tests/test_gpu_lift.py: the fused path against the oracle


def _cuda(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _module(bounds=((-6.0, 6.0, 0.5), (-6.0, 6.0, 0.5), (-10.0, 10.0, 20.0)), discount=0.5, **kw):
    from streamingflow_amd.models.lift_splat import LiftSplat
    kw = {"d_bound": (2.0, 8.0, 1.0), "final_dim": (32, 48), "encoder_downsample": 8, **kw}
    return LiftSplat(bounds[0], bounds[1], bounds[2], discount=discount, **kw).cuda()


@pytest.mark.parametrize("shape", RU.SHAPES)
def test_kernel_against_the_float64_oracle(shape):
    """|dev - ref32| <= 2^-23 |ref32| + 1e-9 max|row| (rig_util.bound: derived, not measured)."""
    m = _module()
    K, E, ego = RU.general_rig(*shape, seed=11 + sum(shape))
    ref32, tol = RU.bound(RU.affines64(K, E, ego))
    Kd, Ed, egod = _cuda(K, E, ego)
    dev = m.rig_affines_device(Kd, Ed, egod)
    torch_path = m.rig_affines(Kd, Ed, egod)
    assert dev.dtype == torch.float32 and tuple(dev.shape) == shape + (12,)
    got = dev.cpu().numpy()
    err = np.abs(got.astype(np.float64) - ref32.astype(np.float64))
    print(shape, "elements", got.size, "differing from the fp32 oracle", int((got != ref32).sum()), "from rig_affines on the device",
          int((dev != torch_path).sum()), "worst error / bound", float((err / tol).max()))
    assert np.isfinite(got).all() and (err <= tol).all()
    m.check_rig()      # no flag


def test_bad_cameras_come_out_nan_and_set_the_flag():
    m = _module()
    (K, E, ego), (Kb, _, _), bad = RU.bad_rig()
    sound = m.rig_affines_device(*_cuda(K, E, ego)).view(6, 12)
    m.check_rig()
    got = m.rig_affines_device(*_cuda(Kb, E, ego)).view(6, 12)
    keep = [i for i in range(6) if i not in bad]
    assert bool(torch.isnan(got[list(bad)]).all())
    assert torch.equal(got[keep], sound[keep]) and bool(torch.isfinite(sound).all())
    with pytest.raises(ValueError, match="singular"):
        m.check_rig()
    m.check_rig()      # cleared by the raise
    # a non-finite extrinsic or ego-motion value does the same for the cameras that read it: camera (0, 1, 2) its own extrinsics,
    # frame 0's cameras pose 0 (frame 1, the last, meets no pose)
    Eb, egob = E.copy(), ego.copy()
    Eb[0, 1, 2, 1, 3] = np.nan
    egob[0, 0, 4] = np.inf
    got = m.rig_affines_device(*_cuda(K, Eb, egob)).view(6, 12)
    assert bool(torch.isnan(got[[0, 1, 2, 5]]).all()) and torch.equal(got[[3, 4]], sound[[3, 4]])
    with pytest.raises(ValueError):
        m.check_rig()
    m.check_rig()


def _lift_inputs(C=8, seed=3):
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn((1, 2, 3, C, 4, 6), generator=g)
    depth = torch.randn((1, 2, 3, 6, 4, 6), generator=g) * 2
    return feat, depth


def test_lift_with_bad_cameras_equals_the_sound_rig_with_their_rays_zeroed():
    """A NaN affine sends every point of the camera to the sentinel cell; zero rays on a sound rig add +0.0 to the cells they reach,
    which changes no sum: the two BEVs are bitwise equal."""
    m = _module()
    (K, E, ego), (Kb, _, _), bad = RU.bad_rig()
    feat, depth = _lift_inputs()
    zeroed = feat.clone().view(6, -1)
    zeroed[list(bad)] = 0.0
    zeroed = zeroed.view_as(feat)
    full = m.lift_splat(feat.cuda(), depth.cuda(), *_cuda(K, E, ego), device_affines=True)
    want = m.lift_splat(zeroed.cuda(), depth.cuda(), *_cuda(K, E, ego), device_affines=True)
    m.check_rig()
    got = m.lift_splat(feat.cuda(), depth.cuda(), *_cuda(Kb, E, ego), device_affines=True)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    assert float(want.abs().max()) > 0 and not torch.equal(full, want)      # the sound cameras feed cells, and so would the two bad ones
    with pytest.raises(ValueError):
        m.check_rig()


@pytest.mark.parametrize("tag", list(cases.LIFT_RIG_CASES))
def test_lift_with_device_affines_against_the_oracle(tag):
    feat, depth, intr, extr, ego, fr, (start, res, dim), discount = cases.lift_rig_inputs(tag)
    b, s, n, C, final_dim, down, d_bound, xb, yb, zb, _ = cases.LIFT_RIG_CASES[tag]
    fH, fW = feat.shape[-2:]
    m = _module((xb, yb, zb), discount, d_bound=d_bound, final_dim=final_dim, encoder_downsample=down)
    args = (feat.cuda(), depth.cuda(), intr.cuda(), extr.cuda(), ego.cuda())
    m.device_affines = True
    out = m.lift_splat(*args)
    m.device_affines = False
    g = LS.get_geometry(fr, intr.view(b * s, n, 3, 3), extr.view(b * s, n, 4, 4)).view(b, s, n, *fr.shape)
    x = LS.depth_outer(feat.reshape(b * s * n, C, fH, fW), depth.reshape(b * s * n, -1, fH, fW)).reshape(b, s, n, -1, fH, fW, C)
    want = LS.projection_to_birds_eye_view(x, g, ego, start, res, dim, discount, stable=True)
    assert maxabs(out, want) <= TOL
    same = torch.equal(m.rig_affines_device(*args[2:]), m.rig_affines(*args[2:]))
    print(tag, "affines bitwise equal to the torch path:", same)
    if same:
        assert torch.equal(out, m.lift_splat(*args))
    m.check_rig()


def test_lift_is_captured_from_raw_intrinsics_and_replayed_on_a_second_rig():
    tag = "rig_small"
    feat, depth, intr, extr, ego, fr, _, discount = cases.lift_rig_inputs(tag)
    b, s, n, C, final_dim, down, d_bound, xb, yb, zb, _ = cases.LIFT_RIG_CASES[tag]
    m = _module((xb, yb, zb), discount, d_bound=d_bound, final_dim=final_dim, encoder_downsample=down)
    m.device_affines = True
    intr2 = intr * 1.03      # K[2][2] = 1.03 too: a general K
    intr2[..., 0, 1] = 0.7
    ego2 = ego.flip(1) * 0.5
    rigs = {"one": (intr.cuda(), extr.cuda(), ego.cuda()), "two": (intr2.cuda(), extr.flip(2).contiguous().cuda(), ego2.cuda())}
    fd, dd = feat.cuda(), depth.cuda()
    eager = {k: m.lift_splat(fd, dd, *rig).clone() for k, rig in rigs.items()}
    assert not torch.equal(eager["one"], eager["two"])
    static = [t.clone() for t in rigs["one"]]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m.lift_splat(fd, dd, *static)
    for k in ("one", "two", "one"):
        for dst, src in zip(static, rigs[k]):
            dst.copy_(src)
        out.fill_(-7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[k]), k
    m.check_rig()


def test_c_abi_refusals_write_nothing():
    from streamingflow_amd import _lib, runtime
    K, E, ego = _cuda(*RU.general_rig(1, 2, 3, seed=9))
    out = torch.full((6, 12), 7.0, device="cuda")
    flags = torch.zeros((1,), dtype=torch.int32, device="cuda")
    fn = _lib.lib().sf_rig_affines_fwd
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    good = [p(K), p(E), p(ego), 1, 2, 3, p(out), p(flags)]
    for pos, bad in [(0, None), (1, None), (2, None), (6, None), (7, None), (3, 0), (4, 0), (5, 0), (3, -1), (4, -1), (5, -1)]:
        args = list(good)
        args[pos] = bad
        assert fn(*args, runtime.stream_ptr("cuda")) == _lib.SF_ERR_INVALID, (pos, bad)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and int(flags) == 0
    assert fn(*good, runtime.stream_ptr("cuda")) == _lib.SF_OK
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == 7.0).any()) and int(flags) == 0
