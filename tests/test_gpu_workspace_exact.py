"""GPU: the workspace a size query returns is exactly enough, and less is refused before anything is enqueued (csrc/dispatch.h: Arena).

Exact size: every module's forward runs through the package twice, once on the package's grow-only workspace (1024 floats of slack
behind the queried bytes) and once with runtime.workspace / static_workspace handing out exactly the queried bytes as a 256-byte-aligned
view inside a canary-filled tensor.  The guards on both sides stay untouched and every output is bitwise the first run's.  Shapes
(C = 64): one latent on the small-P kernel, several images (slab sums), one image above LARGE_P (two-level SE sums), and a batch above
SF_WINO_MIN_P; the decoder (output 16 x the input) at the first two.

Short workspace: the same entry points through the C ABI on the packed weights of those modules, every tensor and the workspace
allocated at full size but `query - 256` passed as ws_bytes: SF_ERR_WORKSPACE, and after a synchronise the canary-filled workspace
and outputs are unchanged.  A defined return path: nothing here is meant to fault."""
import functools
import types

import pytest
import torch

from util import build_pair
from ws_layout_util import NAMES, entry_points
from streamingflow_amd import _lib, packing, runtime, schedule as S
from streamingflow_amd.runtime import ptr

pytestmark = pytest.mark.gpu
C = 64
SHAPES = [(1, 8, 16), (3, 20, 36), (1, 96, 96), (4, 60, 60)]
CANARY = -7.5
GUARD = 4096      # floats on either side of a handed-out workspace
DT = 0.05


def rnd(*shape, seed=0):
    g = torch.Generator(device="cuda").manual_seed(1000 + seed)
    return torch.randn(shape, device="cuda", generator=g) * 0.5


@functools.lru_cache(maxsize=None)
def modules():
    from streamingflow_amd.layers import convolutions as cv, temporal, temporal_ode_bayes as tob
    from streamingflow_amd.models.distributions import DistributionModule
    from streamingflow_amd.beverse import motion_modules as mm
    import encoder_neck_util
    torch.manual_seed(0)
    M = types.SimpleNamespace()
    M.ode = build_pair(C, "rk4", True, True, DT)[0].gru_ode      # every solver-stage buffer in use
    M.ode.use_graph = False
    M.bottleneck, M.bottleneck_down = cv.Bottleneck(C, 2 * C), cv.Bottleneck(C, 2 * C, downsample=True)
    M.block, M.bottle, M.bottle_proj, M.deeplab = cv.Block(C), cv.Bottleblock(C), cv.Bottleblock(2 * C, C), cv.DeepLabHead(C, 8, 128)
    M.gru_cell, M.gru_ode_cell, M.spatial_gru = tob.SpatialGRUCell(C, C), tob.SpatialGRUODECell(C, C), temporal.SpatialGRU(C, C)
    M.dist, M.dist_bev, M.dist_spatial = DistributionModule(C, 32), mm.DistributionModule(C, 32, -5.0, 5.0), mm.SpatialDistributionModule(C, 32, -5.0, 5.0)
    for m in vars(M).values():
        m.cuda().eval()
    M.neck = encoder_neck_util.build(encoder_neck_util.CASES[0]).cuda()
    return M


def schedule(solver):
    return S.build_schedule([0.0, 2 * DT], [3 * DT, 4 * DT], DT, True, solver)


def rollout(M, n, H, W):
    sc = schedule(M.ode.solver)
    return M.ode.rollout_nhwc(rnd(2, n, H, W, C), sc, rnd(sc.n_draws, n, H, W, C, seed=1))


def rollout_flow(M, n, H, W):
    packing.set_persistent_flow(True)      # checked: a wait that timed out on a busy device re-runs the rollout launch per layer, bitwise the same
    try:
        return rollout(M, n, H, W)
    finally:
        packing.set_persistent_flow(None)


def resumed(M, n, H, W):
    M.ode.seed_noise(11)
    sess = M.ode.stream(DT, use_graph=False)
    sess.observe(0.0, rnd(H, W, C))
    sess.observe(2 * DT, rnd(H, W, C, seed=1))
    return sess.predict([3 * DT, 4 * DT]), sess.state


def seeded(fn):
    def run(*a):
        torch.manual_seed(5)      # the draws of infer_state / ode_step
        return fn(*a)
    return run


def planar(M, n, H, W):
    out = torch.zeros((n, 8, H, W), device="cuda")
    return M.deeplab.forward_nhwc_into_planar(rnd(n, H, W, C), out, 1, 8 * H * W, 8 * H * W)


def neck(M, n, H, W):
    return M.neck.neck_nhwc(rnd(n, M.neck.c_hi, H, W), rnd(n, M.neck.c_lo, 2 * H, 2 * W, seed=1))


# name -> (forward(M, n, H, W) -> tensor(s), the shapes it runs at)
ALL, ONE, SMALL = SHAPES, [s for s in SHAPES if s[0] == 1], SHAPES[:2]
FORWARDS = {
    "bottleneck": (lambda M, n, H, W: M.bottleneck(rnd(n, C, H, W)), ALL),
    "bottleneck_down": (lambda M, n, H, W: M.bottleneck_down(rnd(n, C, H, W)), ALL),
    "block": (lambda M, n, H, W: M.block(rnd(n, C, H, W)), ALL),
    "bottleblock": (lambda M, n, H, W: M.bottle(rnd(n, C, H, W)), ALL),
    "bottleblock_proj": (lambda M, n, H, W: M.bottle_proj.forward_nhwc(rnd(n, H, W, C), rnd(n, H, W, C, seed=1)), ALL),
    "deeplab_head": (lambda M, n, H, W: M.deeplab(rnd(n, C, H, W)), ALL),
    "deeplab_head_planar": (planar, ALL),
    "gru_cell": (lambda M, n, H, W: M.gru_cell(rnd(n, C, H, W), rnd(n, C, H, W, seed=1)), ALL),
    "gru_ode_cell": (lambda M, n, H, W: M.gru_ode_cell(rnd(n, C, H, W), rnd(n, C, H, W, seed=1)), ALL),
    "spatial_gru": (lambda M, n, H, W: M.spatial_gru(rnd(n, 2, C, H, W)), ALL),
    "dual_cell": (lambda M, n, H, W: M.ode.gru_c(rnd(n, C, H, W), rnd(n, C, H, W, seed=1)), ALL),
    "dual_cell_obs": (lambda M, n, H, W: M.ode.gru_obs.gru_d(rnd(n, C, H, W), rnd(n, C, H, W, seed=1)), ALL),
    "infer_state": (seeded(lambda M, n, H, W: M.ode.infer_state(rnd(n, C, H, W))), ALL),
    "ode_step": (seeded(lambda M, n, H, W: M.ode.ode_step(rnd(n, C, H, W), rnd(n, C, H, W, seed=1), DT, 0.0)[:2]), ALL),
    "rollout": (rollout, ALL),
    "rollout_flow": (rollout_flow, SHAPES[:1]),
    "rollout_resumed": (resumed, ONE),
    "small_encoder": (lambda M, n, H, W: M.ode.srvp_encoder.forward_nhwc(rnd(n, H, W, M.ode.srvp_encoder.nc)), ALL),
    "small_decoder": (lambda M, n, H, W: M.ode.srvp_decoder.forward_nhwc(rnd(n, H, W, M.ode.srvp_decoder.nc)), SMALL),
    "dist_head": (lambda M, n, H, W: M.dist(rnd(n, 1, C, H, W)), ALL),
    "dist_head_beverse": (lambda M, n, H, W: M.dist_bev(rnd(n, 1, C, H, W)), ALL),
    "dist_head_spatial": (lambda M, n, H, W: M.dist_spatial(rnd(n, 1, C, H, W)), ALL),
    "camera_neck": (neck, ALL),
}


class ExactWorkspaces:
    """runtime.workspace / static_workspace that hand out exactly the requested bytes, 256-byte aligned, between two guards."""

    def __init__(self):
        self.handed = []

    def __call__(self, nbytes, device):
        n = (int(nbytes) + 3) // 4
        buf = torch.full((n + 2 * GUARD + 64,), CANARY, dtype=torch.float32, device="cuda")
        lo = GUARD + (-(buf.data_ptr() // 4 + GUARD)) % 64
        view = buf[lo:lo + n]
        assert view.data_ptr() % 256 == 0 and view.numel() * 4 == int(nbytes)
        self.handed.append((buf, lo, n))
        return view

    def guards_untouched(self):
        assert self.handed
        return all(bool((buf[:lo] == CANARY).all()) and bool((buf[lo + n:] == CANARY).all()) for buf, lo, n in self.handed)


def flat(out):
    return [out] if torch.is_tensor(out) else [t for o in out for t in flat(o)]


@pytest.mark.parametrize("name,n,H,W", [(k, *s) for k, (_, shapes) in FORWARDS.items() for s in shapes],
                         ids=lambda v: v if isinstance(v, str) else str(v))
def test_exactly_the_queried_size_is_enough(name, n, H, W, monkeypatch):
    M, fwd = modules(), FORWARDS[name][0]
    with torch.no_grad():
        want = [t.clone() for t in flat(fwd(M, n, H, W))]
        exact = ExactWorkspaces()
        monkeypatch.setattr(runtime, "workspace", exact)
        monkeypatch.setattr(runtime, "static_workspace", exact)
        got = flat(fwd(M, n, H, W))
    torch.cuda.synchronize()
    assert exact.guards_untouched()
    assert len(got) == len(want) > 0
    for g, w in zip(got, want):
        assert bool(torch.isfinite(w).all()) and torch.equal(g, w)


def packed_weights(M, H, W):
    """The packed structs of the modules above (tests/ws_layout_util.py: entry_points)."""
    Wt = types.SimpleNamespace()
    Wt.gru, Wt.dual, Wt.pm = M.gru_cell.packed().struct, M.ode.gru_c.packed().struct, M.ode.p_model.packed().struct
    Wt.bottle = M.bottle.packed().struct
    Wt.bottle_proj = _lib.BottleW.from_buffer_copy(M.bottle_proj.packed().struct)      # the channel split of a two-tensor call
    Wt.bottle_proj.c7.c0 = Wt.bottle_proj.c7.c1 = Wt.bottle_proj.proj.c0 = Wt.bottle_proj.proj.c1 = C
    Wt.enc, Wt.dec = M.ode.srvp_encoder.packed().struct, M.ode.srvp_decoder.packed().struct
    Wt.bottlenecks = [M.bottleneck.packed().struct, M.bottleneck_down.packed().struct]
    Wt.dist, Wt.convnext, Wt.deeplab = M.dist_bev.packed().struct, M.block.packed().struct, M.deeplab.packed().struct
    pk = M.neck.packed(H, W)
    Wt.twin, Wt.neck_convs = pk.struct, pk.convs
    return Wt


@pytest.mark.parametrize("n,H,W", SHAPES[:2])
def test_short_workspace_is_refused_and_nothing_is_written(n, H, W):
    M = modules()
    # every tensor at full size, so that even a call that went ahead would stay inside its allocations: the largest input or output of
    # any entry point here is below 2048 floats a pixel (the decoder's [n][4H][4W][C] output: 1024)
    x = torch.zeros(2048 * n * H * W, device="cuda")
    y = torch.full((2048 * n * H * W,), CANARY, device="cuda")
    E = entry_points(packed_weights(M, H, W), ptr(x), ptr(y), n, H, W)
    ws = torch.full((max(need for need, _ in E.values()) // 4 + 64,), CANARY, device="cuda")
    for name in NAMES:
        need, call = E[name]
        assert need % 256 == 0 and need > 256
        rc = call(ptr(ws), need - 256)
        assert rc == _lib.SF_ERR_WORKSPACE, (name, rc)
    torch.cuda.synchronize()
    assert bool((ws == CANARY).all()) and bool((y == CANARY).all())
