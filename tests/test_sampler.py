"""CPU: the trajectory sampler's plain-torch path (streamingflow_amd.sampler) against the REFERENCE's rows
(tests/golden/sampler.npz, tools/gen_sampler_golden.py).  The comparison rule and its tolerances: sampler_util.py."""
import numpy as np
import pytest
import torch

import sampler_util as SU


@pytest.fixture(autouse=True)
def _torch_path(monkeypatch):
    monkeypatch.setenv("SF_PLAN_TORCH", "1")        # the same code whether or not the machine has a device


@pytest.mark.parametrize("tag", SU.TAGS)
def test_torch_path_matches_the_reference(tag):
    out, order = SU.run_scene(tag, "cpu")
    assert out.dtype == torch.float64 and order.dtype == torch.int32
    SU.check_rows(tag, out, order)


@pytest.mark.parametrize("tag", SU.TAGS)
def test_sample_draws_and_returns_what_the_reference_does(tag):
    """``sample`` after ``np.random.seed``: its rows are the reference's sorted result, compared through the order the same draws give
    (rule (a) - (d)), and ``np.random`` is left where the reference leaves it (the state after the replayed draws, which the fixture
    generator holds equal to the reference's)."""
    from streamingflow_amd import sampler as S
    sc, G = SU.GEN.scene(tag), SU.golden()
    seed = int(G[f"{tag}.seed"])
    ns, nl, nr = S.counts(sc["M"], sc["possibility"])
    np.random.seed(seed)
    u = SU.GEN.replay_draws(sc["M"], nl + nr)
    want_state = np.random.get_state()
    assert np.array_equal(u, G[f"{tag}.uniforms"])
    np.random.seed(seed)
    got = S.sample(sc["v0"], sc["kappa"], sc["T0"], sc["N0"], sc["tt"], sc["M"], *(() if sc["possibility"] is None else (sc["possibility"],)))
    assert SU.GEN._same_state(np.random.get_state(), want_state)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (sc["M"], len(sc["tt"]), 3)
    full, order = SU.run_scene(tag, "cpu", full_grid=True)
    assert np.array_equal(got, full.numpy())
    SU.check_rows(tag, torch.from_numpy(got[:, ::sc["fine"]].copy()), order, " (sample)")
    # outside runs of near-equal keys the rows sit where the reference's own argsort put them
    keys, ref_order = G[f"{tag}.keys"], G[f"{tag}.order_ref"]
    k = np.sort(keys)
    apart = np.ones(len(k), dtype=bool)
    apart[1:] &= np.diff(k) > SU.KEY_TOL
    apart[:-1] &= np.diff(k) > SU.KEY_TOL
    assert np.array_equal(order.numpy()[apart], ref_order[apart])


def test_fresnel_matches_scipy():
    from streamingflow_amd.sampler import fresnel
    G = SU.golden()
    S, C = fresnel(torch.from_numpy(G["fresnel.z"]))
    err = max(float(np.abs(S.numpy() - G["fresnel.S"]).max()), float(np.abs(C.numpy() - G["fresnel.C"]).max()))
    print(f"torch Fresnel: largest |error| against scipy over {len(G['fresnel.z'])} points {err:.3e}")
    assert err <= SU.FRESNEL_TOL
    z = torch.tensor([float("inf"), -float("inf"), float("nan"), 1e200])
    S, C = fresnel(z)
    assert S.tolist()[:2] == C.tolist()[:2] == [0.5, -0.5] and bool(torch.isnan(S[2])) and bool(torch.isnan(C[2])) and float(S[3]) == float(C[3]) == 0.5


def test_counts_follow_the_reference():
    from streamingflow_amd.sampler import TrajectorySampler, counts
    for M in (66, 64, 128):
        with pytest.raises(ValueError):
            counts(M)
        with pytest.raises(ValueError):
            TrajectorySampler(6, n_samples=M)
    assert counts(5) == (1, 2, 2) and counts(1800) == (360, 720, 720) and counts(50, [0.2, 0.6, 0.2]) == (30, 10, 10)
    assert TrajectorySampler(6).n_samples == 1800


def test_stamps_are_the_references():
    from streamingflow_amd.sampler import TrajectorySampler
    for n_future in (1, 4, 6, 7):
        s = TrajectorySampler(n_future, n_samples=5)
        tt = np.arange(0, n_future * 0.5 + 0.05, 0.05)          # NuscenesData.py:545-548 at SAMPLE_INTERVAL = 0.5
        assert np.array_equal(s.tt_kept.numpy(), tt[::10]) and s.t_key == tt[-1] and s.n_t == n_future + 1


def test_kappa_from_steering():
    from streamingflow_amd.sampler import kappa_from_steering
    assert kappa_from_steering(0.1) == 2 * 0.1 / 2.588 and kappa_from_steering(0.1, left_hand_traffic=True) == 2 * -0.1 / 2.588
    t = torch.tensor([0.2, -0.3], dtype=torch.float64)
    assert torch.equal(kappa_from_steering(t), 2 * t / 2.588)


def test_sampler_object_equals_the_core_and_batches_are_independent():
    from streamingflow_amd.sampler import TrajectorySampler
    sc, G = SU.GEN.scene("m600"), SU.golden()
    smp = TrajectorySampler(sc["n_future"], n_samples=sc["M"])
    u = torch.from_numpy(G["m600.uniforms"])
    out, order = smp(torch.tensor([sc["v0"]]), torch.tensor([sc["kappa"]]), uniforms=u[None], return_order=True)
    assert out.dtype == torch.float32 and tuple(out.shape) == (1, 600, 7, 3)
    core, core_order = SU.run_scene("m600", "cpu")
    assert torch.equal(out[0], core.float()) and torch.equal(order[0], core_order)
    # B = 3 with mixed signs of kappa equals three B = 1 calls
    v0 = torch.tensor([0.0, 4.0, 20.0])
    kappa = torch.tensor([0.3, 0.0, -0.5])
    us = torch.stack([u, u.flip(-1), (u * 0.5)])
    both = smp(v0, kappa, uniforms=us, return_order=True)
    for b in range(3):
        one = smp(v0[b:b + 1], kappa[b:b + 1], uniforms=us[b:b + 1], return_order=True)
        assert torch.equal(both[0][b], one[0][0]) and torch.equal(both[1][b], one[1][0]), b
    # drawn uniforms: reproducible from a generator, rows finite and in ascending x at the key stamp
    g = torch.Generator().manual_seed(3)
    a = smp(v0, kappa, generator=g)
    b = smp(v0, kappa, generator=torch.Generator().manual_seed(3))
    assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and tuple(a.shape) == (3, 600, 7, 3)
    if smp.t_key == float(smp.tt_kept[-1]):                          # the key stamp is the last kept one
        assert bool((a[:, 1:, -1, 0] >= a[:, :-1, -1, 0]).all())
