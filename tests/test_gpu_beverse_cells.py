"""GPU: the BEVerse conv-GRU cells (``GRUCell`` -> sf_gru_cell_fwd, ``SpatialGRU`` without decoder -> sf_spatial_gru_fwd) against a float64
reference of the same cell at every kernel family their dispatch reaches (tests/beverse_cell_util.py: CASES, FAMILIES) — the sizes above
the fixtures of test_gpu_resfuture.py, up to the Winograd launches the benchmarked 200 x 200 rollout runs on, and the only callers with
x and state of different widths.
  * every channel and pixel within the measured tolerance of beverse_cell_util (8 x the float32 reference's own error; + 2e-5 on the
    Winograd forms), and the profiler must name the kernels the case was chosen for (tests/test_beverse_cell_plan.py holds the same on
    the host, with the sensitivity of every case to a wrong cell);
  * a cell writing into a slice of a larger buffer touches nothing outside it and computes what it computes into its own tensor;
  * Winograd and direct forms of the same cell agree to 2e-5, the bar of test_gates_with_second_output_and_blend;
  * whole rollouts at the kernel families of the benchmarked size against the module's own plain-torch wiring, all channels."""
import ctypes

import pytest
import torch

import beverse_cell_util as U
from util import maxabs

pytestmark = pytest.mark.gpu

_CELLS = [c for c in U.CASES if c["kind"] == "cell"]
_GRUS = [c for c in U.CASES if c["kind"] == "spatial_gru"]
_WINO = [c for c in U.CASES if U.FAMILIES[c["family"]][2]]
_name = lambda c: c["name"]


def _profiled(fn):
    """run fn() under the library profiler: (result, names of the conv kernels that ran)"""
    from streamingflow_amd import _lib
    L = _lib.lib()
    NK = _lib.SF_PROF_KEYS
    calls, ms = (ctypes.c_int32 * NK)(), (ctypes.c_double * NK)()
    fl, by = (ctypes.c_double * NK)(), (ctypes.c_double * NK)()
    L.sf_prof_enable(1)
    try:
        r = fn()
        torch.cuda.synchronize()
        L.sf_prof_collect(calls, ms, fl, by)
    finally:
        L.sf_prof_enable(0)
    return r, {_lib.KERNEL_NAMES[k] for k in range(NK) if calls[k]}


def _device_forward(case):
    net = U.build(case).cuda()
    x, s = U.inputs(case)
    return _profiled(lambda: net(x.cuda(), s.cuda() if s is not None else None))


def _check(case):
    got, used = _device_forward(case)
    ref = U.reference(case)
    assert tuple(got.shape) == tuple(ref.shape)
    err, tol = maxabs(got, ref), U.tolerance(case)
    print(case["name"], case["family"], "max |device - float64| %.3e bound %.3e kernels %s" % (err, tol, sorted(used)))
    want = U.planned(case)["names"]
    if want is None:      # the batched Winograd kernel: the gates launch (AFFINE, second output), then the candidate (BLEND)
        assert used and all(k.startswith("conv_wino<") for k in used), used
        assert any(k.endswith(",affine>") for k in used) and any(k.endswith(",blend>") for k in used), used
    else:
        assert used == want and all(k.startswith(U.kernel_prefix(case)) for k in used), (used, want)
    assert err <= tol, (case["name"], err, tol)


@pytest.mark.parametrize("case", _CELLS, ids=_name)
def test_cell_vs_fp64(case):
    _check(case)


@pytest.mark.parametrize("case", _GRUS, ids=_name)
def test_spatial_gru_vs_fp64(case):
    """all T states: each is written straight into out[t] and read back from there as the next step's state"""
    _check(case)


@pytest.mark.parametrize("case", [U.BY_NAME["sp_3img"], U.BY_NAME["wino_rows_over_4"]], ids=_name)
def test_cell_into_given_out_and_slack(case):
    from streamingflow_amd import runtime
    net = U.build(case).cuda()
    x, s = (runtime.to_nhwc(t.cuda()) for t in U.inputs(case))
    own = net.forward_nhwc(x, s)
    n, h, w, C = own.shape
    lead, trail, fill = 64, 192, -777.25
    buf = torch.full((lead + own.numel() + trail,), fill, dtype=torch.float32, device="cuda")
    out = buf[lead:lead + own.numel()].view(n, h, w, C)
    res = net.forward_nhwc(x, s, out=out)
    torch.cuda.synchronize()
    assert res.data_ptr() == out.data_ptr()
    assert bool((buf[:lead] == fill).all()) and bool((buf[lead + own.numel():] == fill).all())
    assert torch.equal(out, own)
    assert maxabs(runtime.to_nchw(own), U.reference(case)) <= U.tolerance(case)


def test_one_step_is_bitwise_the_same_through_every_module_that_shares_the_cell():
    """``GRUCell.forward_nhwc``, ``SpatialGRU.forward_nhwc`` over T = 1 and ``SpatialGRUCell.forward`` (NCHW in and out) pack the same
    parameters with one routine (layers/temporal.py: pack_gru_block) and run them through one wrapper each of sf_gru_cell_fwd and
    sf_spatial_gru_fwd: the same weights and inputs give the same bits, at the smallest shape of this file (1 x 9 x 7), gate bias 0.3."""
    from streamingflow_amd import runtime
    from streamingflow_amd.beverse import basic_modules as B
    from streamingflow_amd.layers.temporal_ode_bayes import SpatialGRUCell
    case = U.BY_NAME["direct_24_16"]
    cell = U.build(case).cuda()
    gru = B.SpatialGRU(case["Cx"], case["C"], gru_bias_init=case["gru_bias_init"])
    single = SpatialGRUCell(case["Cx"], case["C"], gru_bias_init=case["gru_bias_init"])
    for m in (gru, single):
        m.load_state_dict(cell.state_dict())
        m.cuda().eval()
    x, s = (t.cuda() for t in U.inputs(case))
    xn, sn = runtime.to_nhwc(x), runtime.to_nhwc(s)
    a = cell.forward_nhwc(xn, sn)
    b = gru.forward_nhwc(xn[None], sn)
    c = single(x, s)
    torch.cuda.synchronize()
    assert tuple(b.shape) == (1,) + tuple(a.shape) and tuple(c.shape) == tuple(s.shape)
    print("max |GRUCell - SpatialGRU| %.3e, max |GRUCell - SpatialGRUCell| %.3e" % (maxabs(a, b[0]), maxabs(runtime.to_nchw(a), c)))
    assert maxabs(c, U.reference(case)) <= U.tolerance(case)
    assert torch.equal(a, b[0])
    assert torch.equal(runtime.to_nchw(a), c)


@pytest.mark.parametrize("case", _WINO, ids=_name)
def test_winograd_and_direct_forms_agree(case):
    from streamingflow_amd import packing
    was = packing.winograd()
    try:
        packing.set_winograd(True)
        a, used_a = _device_forward(case)
        packing.set_winograd(False)
        b, used_b = _device_forward(case)
    finally:
        packing.set_winograd(was)
    diff = maxabs(a, b)
    print(case["name"], "max |Winograd - direct| %.3e" % diff, sorted(used_a), sorted(used_b))
    if case["family"] == "wino":
        assert all(k.startswith("conv_wino<") for k in used_a) and not any(k.startswith("conv_wino<") for k in used_b), (used_a, used_b)
    else:      # the small-P kernel reports one name for both of its forms: the arithmetic must have changed
        assert used_a == used_b and all(k.startswith("conv_sp<") for k in used_a), (used_a, used_b)
    assert not torch.equal(a, b)
    assert diff <= 2e-5, diff
    assert maxabs(b, U.reference(case)) <= U.TOL_DIRECT


@pytest.mark.parametrize("r", U.ROLLOUTS, ids=_name)
def test_rollouts_at_the_benchmarked_kernel_families(r):
    """ResFuturePredictionV2(64, 32) at 1 x 100 x 142 (the batched Winograd launches the 200 x 200 benchmark runs on),
    ResFuturePrediction(32, 16) at 1 x 70 x 66 (direct-fragment kernel at mid P, reset gate while staging) and
    ResFuturePredictionV1(64, 32, n_gru_blocks=2, prob_each_future=True) at 1 x 30 x 34 (small-P kernel, its Winograd form), n_future = 2,
    against the module's own _forward_torch on the CPU in float32, all channels, to 1e-3 as test_gpu_resfuture.py.

    Measured on the CPU path (beverse_cell_util.perturbation_movement: both inputs moved by hashed U(-1e-5, 1e-5)), the rollouts move by
    2.0e-5 (v2_wino), 1.9e-5 (res_direct_mid) and 4.4e-6 (v1_each_sp) — as the 3.7e-5 of the fixture shapes, far inside the bar; the
    first step's flow reaches 3.18 / 3.21 / 2.46 px and samples beyond all four image edges (test_beverse_cell_plan.py asserts both)."""
    mag, sides = U.first_flow(r)
    assert mag >= 1.0 and all(sides.values()), (mag, sides)
    net = U.build_rollout(r).cuda()
    sample, hidden = (t.cuda() for t in U.rollout_inputs(r))
    got, used = _profiled(lambda: net(sample, hidden))
    ref = U.rollout_reference(r)
    assert tuple(got.shape) == tuple(ref.shape)
    err = maxabs(got, ref)
    print(r["name"], "max |device - plain torch| %.3e, first flow %.2f px %s, kernels %s" % (err, mag, sides, sorted(used)))
    assert any(k.startswith(r["prefix"]) for k in used), (r["prefix"], used)
    assert err <= 1e-3
