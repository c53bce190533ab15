"""TEST INFRASTRUCTURE — tests/golden/sampler.npz: the REFERENCE's own trajectory sampler (streamingflow/utils/sampler.py ``sample``,
loaded by file path as it is, numpy + scipy in float64 on the CPU) on the scenes below, and scipy's Fresnel integrals at the test
points.  Only inputs and results are stored.

Usage: python tools/gen_sampler_golden.py        (where the reference and scipy are installed)

Per scene <tag>:
  <tag>.uniforms [5, M] float64   the reference's five draws after ``np.random.seed(seed)``, replayed (rand(M) three times,
                                  rand(left + right), random_sample(left + right); rows 3 and 4 zero-padded to M).  The generator asserts
                                  that the replay leaves ``np.random`` in the state the reference's call leaves it in;
  <tag>.unsorted [M, n_t, 3] fp32 the reference's rows with ``np.argsort`` replaced by the identity for the duration of the call, at
                                  the kept stamps ``[:, ::fine]``, cast as the reference's caller casts them;
  <tag>.keys [M] float64          x at the last stamp of the fine grid of those rows: the reference's sort key;
  <tag>.order_ref [M] int32       the reference's own ``argsort``: its sorted result is ``unsorted[order_ref]`` (asserted here bit for bit
                                  against its unpatched call, so the sorted rows are not stored twice);
  <tag>.seed                      the seed that was used.
The scene's other inputs (v0, Kappa, T0, N0, tt, fine, M, possibility) are rebuilt by ``scene(tag)``; float64 is kept only for the
uniforms and the keys.  ``fresnel.z / .S / .C``: 4096 hashed points on [-4, 24], 0, +-1e-300, +-1e-8, +-40, +-4e4 and k / 8 for
k <= 192, with scipy.special.fresnel's values.

A scene's seed is moved on (seed += 1) until
  * no heading before the wrap lies within 1e-6 rad of an odd multiple of pi at a kept stamp (the wrap cannot flip under rounding);
  * with M >= 15, circles and clothoids, both speed choices, a negative longitudinal distance and a mirrored curve all occur;
and the file is not written unless circles occur with both signs of the clamped curvature over the scenes.
"""
import contextlib
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from workloads import hashfill  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sampler.npz")
WRAP_MARGIN = 1e-6
_A = 0.3        # the rotated frame's angle
# tag -> M, Kappa, v0, time grid (n_future, interval: the caller's arange; or an explicit tt), fine, possibility, frame, first seed
SCENES = {
    "m5":     dict(M=5, kappa=0.0, v0=4.0, n_future=1, seed=1),
    "m15":    dict(M=15, kappa=0.004, v0=0.0, n_future=6, seed=2),
    "m50":    dict(M=50, kappa=-0.001, v0=20.0, n_future=1, seed=3),
    "m600":   dict(M=600, kappa=-0.5, v0=0.0, n_future=6, seed=4),
    "m1030":  dict(M=1030, kappa=0.0, v0=4.0, n_future=1, seed=5),
    "m1800":  dict(M=1800, kappa=0.3, v0=20.0, n_future=6, seed=6),
    "tt64":   dict(M=50, kappa=-0.001, v0=4.0, tt=np.arange(64) * 0.05, seed=7),            # the key stamp tt[63] is not a kept one
    "main":   dict(M=50, kappa=0.0, v0=4.0, tt=np.arange(0.0, 3.01, 0.01), fine=100, seed=8),   # the reference's own __main__
    "poss":   dict(M=50, kappa=0.3, v0=4.0, n_future=6, possibility=[0.2, 0.6, 0.2], seed=9),
    "frame":  dict(M=50, kappa=0.004, v0=20.0, n_future=6, T0=[np.sin(_A), np.cos(_A)], N0=[-np.cos(_A), np.sin(_A)], seed=10),
}
TAGS = tuple(SCENES)
INTERVAL = 0.5


def scene(tag):
    """The inputs of a scene: M, Kappa, v0, T0, N0 (float64 arrays), tt (the fine grid), fine, possibility (or None), first seed."""
    s = dict(SCENES[tag])
    s.setdefault("fine", 10)
    s.setdefault("possibility", None)
    if "tt" not in s:
        t_interval = INTERVAL / s["fine"]
        s["tt"] = np.arange(0, s["n_future"] * INTERVAL + t_interval, t_interval)       # NuscenesData.py:545-548
    s["T0"] = np.asarray(s.get("T0", [0.0, 1.0]), dtype=np.float64)
    s["N0"] = np.asarray(s.get("N0", [1.0, 0.0] if s["kappa"] <= 0 else [-1.0, 0.0]), dtype=np.float64)
    return s


def fresnel_points():
    z = -4.0 + 28.0 * hashfill.uniform01("sampler.fresnel", 4096, seed=17)
    special = [0.0, 1e-300, -1e-300, 1e-8, -1e-8, 40.0, -40.0, 4e4, -4e4]
    return np.concatenate([z, special, np.arange(193) / 8.0])


def _counts(M, possibility):
    p = [0.4, 0.2, 0.4] if possibility is None else possibility
    return int(M * p[1]), int(M * p[0]), int(M * p[2])


def replay_draws(M, n_curves):
    """The five draws of the reference's ``sample`` from the current state of ``np.random``, as [5, M]."""
    u = np.zeros((5, M))
    u[0], u[1], u[2] = np.random.rand(M), np.random.rand(M), np.random.rand(M)
    u[3, :n_curves] = np.random.rand(n_curves)
    u[4, :n_curves] = np.random.random_sample(n_curves)
    return u


@contextlib.contextmanager
def identity_argsort():
    real = np.argsort
    np.argsort = lambda a, *args, **kw: np.arange(len(a))
    try:
        yield
    finally:
        np.argsort = real


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def facts(s, u):
    """What the draws of a scene exercise, from the draws alone: (smallest distance of a heading before the wrap from an odd multiple of
    pi over the kept stamps, has circle, has clothoid, has v0 speed, has random speed, has negative distance, has mirrored curve)."""
    M, kappa = s["M"], s["kappa"]
    ns, nl, nr = _counts(M, s["possibility"])
    tt = s["tt"][::s["fine"]]
    acc = 10 * (u[0] - 0.5) + 2
    own = u[2] < 0.2
    vel = np.where(own, s["v0"], 15 * u[1])
    L = vel[:, None] * tt[None, :] + acc[:, None] * (tt[None, :] ** 2) / 2
    Lc = L[ns:]
    alpha = 74 * u[3, :nl + nr] + 6
    circle = u[4, :nl + nr] < 0.2
    krappa = min(-0.01, kappa) if kappa <= 0 else max(0.01, kappa)
    th_circle = Lc * abs(krappa)
    z = (abs(kappa) / np.pi + Lc) / alpha[:, None]
    th_cloth = (0.5 * np.pi * z ** 2 - 0.5 * np.pi * (kappa / np.pi / alpha[:, None]) ** 2) * np.sign(kappa)
    th = np.where(circle[:, None], th_circle, th_cloth)
    margin = float(np.abs(np.mod(th, 2 * np.pi) - np.pi).min())
    # the mirrored block is the second one (n_right curves), whichever side of the lines it ends up on
    return margin, bool(circle.any()), bool((~circle).any()), bool(own.any()), bool((~own).any()), bool((L < 0).any()), nr > 0


def reference_sample():
    from oracle import refimport
    path = os.path.join(refimport.REF_ROOT, "streamingflow", "utils", "sampler.py")
    spec = importlib.util.spec_from_file_location("_reference_sampler", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.sample


def generate():
    from scipy.special import fresnel
    ref = reference_sample()
    out, krappa_signs, margins = {}, set(), {}
    for tag in TAGS:
        s = scene(tag)
        M = s["M"]
        ns, nl, nr = _counts(M, s["possibility"])
        assert M - ns == nl + nr, tag
        seed = s["seed"]
        while True:
            np.random.seed(seed)
            u = replay_draws(M, nl + nr)
            state = np.random.get_state()
            f = facts(s, u)
            if f[0] >= WRAP_MARGIN and (M < 15 or all(f[1:])):
                break
            seed += 1
        args = (s["v0"], s["kappa"], s["T0"], s["N0"], s["tt"], M) + (() if s["possibility"] is None else (s["possibility"],))
        np.random.seed(seed)
        ordered = ref(*args)
        assert _same_state(np.random.get_state(), state), tag       # the replay draws what the reference draws
        np.random.seed(seed)
        with identity_argsort():
            unsorted = ref(*args)
        keys = unsorted[:, -1, 0].copy()
        order_ref = np.argsort(keys)
        assert np.array_equal(unsorted[order_ref], ordered), tag      # the reference's result is its unsorted rows under its own argsort
        assert ordered.shape == (M, len(s["tt"]), 3) and ordered.dtype == np.float64
        if f[1]:
            krappa_signs.add(s["kappa"] > 0)
        margins[tag] = f[0]
        out[f"{tag}.uniforms"] = u
        out[f"{tag}.unsorted"] = unsorted[:, ::s["fine"]].astype(np.float32)
        out[f"{tag}.keys"] = keys
        out[f"{tag}.order_ref"] = order_ref.astype(np.int32)
        out[f"{tag}.seed"] = np.int64(seed)
        gaps = np.diff(np.sort(keys))
        print(f"{tag}: seed {seed}, wrap margin {f[0]:.2e}, smallest gap between distinct keys {gaps[gaps > 0].min():.2e}")
    assert krappa_signs == {True, False}, krappa_signs
    z = fresnel_points()
    S, C = fresnel(z)
    out["fresnel.z"], out["fresnel.S"], out["fresnel.C"] = z, S, C
    return out


if __name__ == "__main__":
    res = generate()
    np.savez_compressed(OUT, **res)
    print(OUT, os.path.getsize(OUT), "bytes")
