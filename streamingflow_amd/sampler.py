"""The planner's trajectory sampler on the MI355X: ``streamingflow/utils/sampler.py::sample`` as
``NuscenesData.get_trajectory_sampling`` calls it, for a batch of (speed, curvature) pairs, without a host round trip.

``TrajectorySampler(n_future)(v0, kappa)`` returns ``[B, M, n_future + 1, 3]`` fp32 rows ``(x, y, heading)`` on the inputs' device, in
the planner's row order (ascending x at the last stamp of the fine time grid); ``Planning.forward`` takes ``[:, :, 1:]``.  On the
device it is ``sf_plan_sample_fwd`` (csrc/plan_sampler.hip): enqueue only, capturable.  For CPU tensors or ``SF_PLAN_TORCH=1`` the
plain-torch fp64 functions below state the same semantics.

What the reference does and this keeps: the counts ``int(M p)`` (and its failure when they do not add up: ``ValueError`` here); the
five uniform draws and what each decides; lines ``L T0``; circles of the curvature clamped away from 0 to +-0.01, which ignore
``T0`` / ``N0``; clothoids of the unclamped curvature with the Fresnel argument ``(|kappa| / pi + L) / alpha``, shifted by their point
at the first stamp and rotated by ``sign(kappa) theta0``; Python's ``%`` in the heading wrap; the mirrored block and its place before
or after the lines by the sign of ``kappa``; the sort key taken on the fine grid's last stamp, in fp64, before decimation.
What differs: the sort is stable (rows with equal keys — all lines have the key +-0 — keep their order before the sort; numpy's
default ``argsort`` leaves that order to chance), and only the kept stamps and the key stamp are evaluated.
"""
import math
import os

import numpy as np
import torch

from . import _fresnel_tables as FT
from . import runtime
from .runtime import ptr

WHEELBASE = 2.588            # NuscenesData.py:539
DEFAULT_POSSIBILITY = (0.4, 0.2, 0.4)
MAX_SAMPLES = 4096           # csrc/plan_sampler.hip: the keys of one sample are sorted in LDS


def counts(M, possibility=None):
    """(straight, left, right) as the reference forms them; ``ValueError`` where its broadcast would fail."""
    p = DEFAULT_POSSIBILITY if possibility is None else possibility
    straight, left, right = int(M * p[1]), int(M * p[0]), int(M * p[2])
    if M < 1 or min(straight, left, right) < 0 or M - straight != left + right:
        raise ValueError(f"n_samples = {M} with possibility {[float(v) for v in p]}: {straight} lines + {left} + {right} curves do not add up "
                         "to it (the reference fails to broadcast there)")
    return straight, left, right


def kappa_from_steering(steering, left_hand_traffic=False):
    """Curvature from the steering-angle feedback: 2 phi / wheelbase; the sign flips in left-hand traffic (NuscenesData.py:534-539)."""
    return 2 * (-steering if left_hand_traffic else steering) / WHEELBASE


def use_torch_path(*tensors):
    return os.environ.get("SF_PLAN_TORCH") == "1" or not all(t.is_cuda for t in tensors)


def _clenshaw(table, piece, x):
    c = torch.tensor(table, dtype=torch.float64, device=x.device)[piece]        # [..., n]
    x2 = 2.0 * x
    b1 = torch.zeros_like(x)
    b2 = torch.zeros_like(x)
    for k in range(c.shape[-1] - 1, 0, -1):
        b1, b2 = c[..., k] + x2 * b1 - b2, b1
    return c[..., 0] + x * b1 - b2


def fresnel(z):
    """(S, C) of an fp64 tensor, scipy.special.fresnel's convention; the algorithm of csrc/plan_sampler.hip (tables:
    tools/gen_fresnel_tables.py), within 1e-12 of scipy."""
    z = z.to(torch.float64)
    az = z.abs()
    small = az <= FT.Z0
    zs = torch.where(small, az, torch.zeros_like(az))
    x = (zs * zs) ** 2
    hs = torch.full_like(x, FT.S[-1])
    hc = torch.full_like(x, FT.C[-1])
    for n in range(len(FT.S) - 2, -1, -1):
        hs = hs * x + FT.S[n]
        hc = hc * x + FT.C[n]
    s_small, c_small = zs * zs * zs * hs, zs * hc
    zl = torch.where(small | ~(az < 1e100), torch.full_like(az, 2.0), az)
    z2 = zl * zl
    t = 1.0 / z2
    piece = (t > FT.EDGES[1]).long() + (t > FT.EDGES[2]).long()
    edges = torch.tensor(FT.EDGES, dtype=torch.float64, device=z.device)
    lo, hi = edges[piece], edges[piece + 1]
    xc = (2.0 * t - lo - hi) / (hi - lo)
    f = _clenshaw(FT.F, piece, xc) / (math.pi * zl)
    g = _clenshaw(FT.G, piece, xc) / (math.pi * math.pi * zl * z2)
    ph = (0.5 * math.pi) * torch.fmod(z2, 4.0)
    sn, cs = torch.sin(ph), torch.cos(ph)
    c_large = 0.5 + f * sn - g * cs
    s_large = 0.5 - f * cs - g * sn
    far = torch.where(az != az, az, torch.full_like(az, 0.5))
    s = torch.where(small, s_small, torch.where(az < 1e100, s_large, far))
    c = torch.where(small, c_small, torch.where(az < 1e100, c_large, far))
    neg = z < 0
    return torch.where(neg, -s, s), torch.where(neg, -c, c)


def _wrap(a):
    return torch.remainder(a + math.pi, 2 * math.pi) - math.pi       # Python's %: the divisor's sign


def rows_torch(v0, kappa, t0, n0, stamps, uniforms, n_straight, n_left, n_right):
    """The unsorted rows at ``stamps`` [n] in fp64: [B, M, n, 3], in the order before the sort ([first block, lines, mirrored block]
    for kappa > 0, [mirrored block, lines, first block] otherwise).  v0, kappa [B]; t0, n0 [B, 2]; uniforms [B, 5, M]."""
    B, _, M = uniforms.shape
    dev = uniforms.device
    p = torch.arange(M, device=dev)[None, :]
    pos = (kappa > 0)[:, None]
    first = torch.where(pos, n_left, n_right)
    line = (p >= first) & (p < first + n_straight)
    j = torch.where(pos, torch.where(p < first, p, p - n_straight), torch.where(p < first, n_left + p, p - first - n_straight))
    mirror = torch.where(pos, p >= first, p < first) & ~line
    j = torch.where(line, torch.zeros_like(j), j)
    g = torch.where(line, p - first, n_straight + j)
    u = uniforms
    acc = 10 * (u[:, 0].gather(1, g) - 0.5) + 2
    vel = torch.where(u[:, 2].gather(1, g) >= 0.2, 15 * u[:, 1].gather(1, g), v0[:, None].expand(B, M))
    alpha = ((80 - 6) * u[:, 3].gather(1, j) + 6)[:, :, None]
    circle = (u[:, 4].gather(1, j) < 0.2)[:, :, None]
    tt = stamps[None, None, :]
    L = vel[:, :, None] * tt + acc[:, :, None] * (tt ** 2) / 2
    k = kappa[:, None, None]
    t0x, t0y, n0x, n0y = t0[:, 0, None, None], t0[:, 1, None, None], n0[:, 0, None, None], n0[:, 1, None, None]
    # circles
    krappa = torch.where(k <= 0, torch.clamp(k, max=-0.01), torch.clamp(k, min=0.01))
    radius = torch.abs(1 / krappa)
    kp = krappa >= 0
    phi = torch.where(kp, L / radius, math.pi - L / radius)
    cx = -1 / krappa + radius * torch.cos(phi)
    cy = 0.0 + radius * torch.sin(phi)
    cth = _wrap(torch.where(kp, L / radius, -L / radius))
    # clothoids
    sgn = torch.sign(k)
    z = (torch.abs(k) / math.pi + L) / alpha
    S, C = fresnel(z)
    px = alpha * (C * t0x + S * n0x)
    py = alpha * (C * t0y + S * n0y)
    X, Y = px - px[:, :, :1], py - py[:, :, :1]
    theta0 = 0.5 * math.pi * ((k / math.pi / alpha) ** 2)
    rc, rs = torch.cos(theta0 * sgn), torch.sin(theta0 * sgn)
    qx = rc * X + rs * Y
    qy = -rs * X + rc * Y
    qth = _wrap((0.5 * math.pi * (z ** 2) - theta0) * sgn)
    x = torch.where(circle, cx, qx)
    y = torch.where(circle, cy, qy)
    th = torch.where(circle, cth, qth)
    m = mirror[:, :, None]
    x, th = torch.where(m, -x, x), torch.where(m, -th, th)
    ln = line[:, :, None]
    x = torch.where(ln, L * t0x, x)
    y = torch.where(ln, L * t0y, y)
    th = torch.where(ln, torch.zeros_like(th), th)
    return torch.stack([x, y, th], dim=-1)


def sample_torch(v0, kappa, t0, n0, tt_kept, t_key, uniforms, n_straight, n_left, n_right):
    """Plain-torch fp64 statement of sf_plan_sample_fwd: (rows [B, M, n_t, 3] fp64 sorted, order [B, M] int32)."""
    stamps = torch.cat([tt_kept, torch.as_tensor([t_key], dtype=torch.float64, device=tt_kept.device)])
    rows = rows_torch(v0, kappa, t0, n0, stamps, uniforms, n_straight, n_left, n_right)
    order = torch.sort(rows[:, :, -1, 0], dim=1, stable=True)[1]
    kept = rows[:, :, :-1]
    out = kept.gather(1, order[:, :, None, None].expand(-1, -1, kept.shape[2], 3))
    return out, order.to(torch.int32)


def sample_device(v0, kappa, t0, n0, tt_kept, t_key, uniforms, n_straight, n_left, n_right, want_order=True):
    """sf_plan_sample_fwd on device tensors (fp64, contiguous): (rows [B, M, n_t, 3] fp32, order [B, M] int32 or None)."""
    B, _, M = uniforms.shape
    n_t = tt_kept.numel()
    dev = uniforms.device
    out = torch.empty((B, M, n_t, 3), dtype=torch.float32, device=dev)
    order = torch.empty((B, M), dtype=torch.int32, device=dev) if want_order else None
    runtime.call("plan_sample", ptr(v0), ptr(kappa), ptr(t0), ptr(n0), ptr(tt_kept), float(t_key), ptr(uniforms), n_straight, n_left, n_right,
                 B, M, n_t, ptr(out), ptr(order), device=dev, scratch=("plan_sample", B, M, n_t))
    return out, order


def _f64(t, device=None):
    return torch.as_tensor(t, device=device).detach().to(torch.float64).contiguous()


def _run(v0, kappa, t0, n0, tt_kept, t_key, uniforms, cnt, want_order):
    B, five, M = uniforms.shape
    if five != 5 or tuple(v0.shape) != (B,) or tuple(kappa.shape) != (B,) or tuple(t0.shape) != (B, 2) or tuple(n0.shape) != (B, 2):
        raise ValueError("sampler: v0, kappa [B]; T0, N0 [B, 2]; uniforms [B, 5, M]")
    if use_torch_path(v0, kappa, t0, n0, tt_kept, uniforms):
        out, order = sample_torch(v0, kappa, t0, n0, tt_kept, t_key, uniforms, *cnt)
        return out, order
    if M > MAX_SAMPLES:
        raise NotImplementedError(f"sampler: n_samples = {M} > {MAX_SAMPLES} on the device")
    return sample_device(v0, kappa, t0, n0, tt_kept, t_key, uniforms, *cnt, want_order=want_order)


class TrajectorySampler:
    """``get_trajectory_sampling`` for a batch: ``n_samples`` candidate trajectories per (speed, curvature) at the ``n_future + 1``
    stamps ``0, sample_interval, ...`` the reference keeps of its ``fine`` times finer grid."""

    def __init__(self, n_future, sample_interval=0.5, n_samples=1800, possibility=None, fine=10):
        self.n_samples = int(n_samples)
        self.counts = counts(self.n_samples, possibility)
        t_end = n_future * sample_interval                          # NuscenesData.py:545-548, the reference's own expressions
        t_interval = sample_interval / fine
        tt = np.arange(0, t_end + t_interval, t_interval)
        self.tt = tt
        self.tt_kept = torch.from_numpy(np.ascontiguousarray(tt[::fine]))
        self.t_key = float(tt[-1])
        self.n_t = int(self.tt_kept.numel())
        self._stamps = {}

    def _kept_on(self, device):
        key = str(device)
        if key not in self._stamps:
            self._stamps[key] = self.tt_kept.to(device)
        return self._stamps[key]

    def __call__(self, v0, kappa, uniforms=None, generator=None, return_order=False):
        """v0, kappa [B] -> [B, n_samples, n_future + 1, 3] fp32 (and order [B, n_samples] int32: the row's position before the sort).
        uniforms [B, 5, n_samples] in [0, 1): acceleration, random speed, speed choice, alpha, curve choice (the last two use the first
        left + right entries); drawn with ``torch.rand`` on the inputs' device when None."""
        v0, kappa = _f64(v0), _f64(kappa, v0.device if isinstance(v0, torch.Tensor) else None)
        dev, B = v0.device, v0.shape[0]
        if uniforms is None:
            uniforms = torch.rand(B, 5, self.n_samples, dtype=torch.float64, device=dev, generator=generator)
        uniforms = _f64(uniforms, dev)
        if uniforms.shape[-1] != self.n_samples:
            raise ValueError(f"uniforms [B, 5, {self.n_samples}] expected, got {tuple(uniforms.shape)}")
        one, zero = torch.ones_like(kappa), torch.zeros_like(kappa)
        t0 = torch.stack([zero, one], dim=1)
        n0 = torch.stack([torch.where(kappa <= 0, one, -one), zero], dim=1)
        out, order = _run(v0, kappa, t0, n0, self._kept_on(dev), self.t_key, uniforms, self.counts, return_order)
        out = out.to(torch.float32)
        return (out, order) if return_order else out


def sample(v0, Kappa, T0, N0, tt, M, possibility=None):
    """The reference's ``sample``: numpy in, [M, len(tt), 3] float64 out, every stamp of ``tt`` evaluated, the key at ``tt[-1]``.  It
    draws from ``np.random`` as the reference does (after ``np.random.seed(s)`` the rows are the reference's, up to the order inside a
    run of equal keys, and the generator is left where the reference leaves it).  On a machine with a device the rows are computed
    there and are fp32 values; otherwise they come from the torch path in full fp64."""
    n_straight, n_left, n_right = cnt = counts(M, possibility)
    u = np.zeros((1, 5, M))
    u[0, 0], u[0, 1], u[0, 2] = np.random.rand(M), np.random.rand(M), np.random.rand(M)
    u[0, 3, :n_left + n_right] = np.random.rand(n_left + n_right)
    u[0, 4, :n_left + n_right] = np.random.random_sample(n_left + n_right)       # np.random.choice draws one of these per entry
    tt = np.ascontiguousarray(tt, dtype=np.float64)
    dev = "cuda" if torch.cuda.is_available() and os.environ.get("SF_PLAN_TORCH") != "1" else "cpu"
    as_t = lambda a, shape: torch.from_numpy(np.asarray(a, dtype=np.float64).reshape(shape).copy()).to(dev)
    out, _ = _run(as_t(v0, (1,)), as_t(Kappa, (1,)), as_t(T0, (1, 2)), as_t(N0, (1, 2)), as_t(tt, (-1,)), float(tt[-1]), as_t(u, u.shape), cnt, False)
    return out[0].double().cpu().numpy()
