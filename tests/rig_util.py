"""TEST INFRASTRUCTURE — a numpy float64 statement of the camera rig's affines (LiftSplat.rig_affines, sf_rig_affines_fwd), the rigs the
kernel tests run, the derived bound, and the timestamp sets of the model-graph tests.

affine[b, s, n] = the 3x4 taking (u*d, v*d, d, 1) to the final ego frame: R_cam K^-1 | t_cam (get_geometry), then
ego[t] = pose_vec2mat(future_egomotion[b, t]) applied on the left for t = own frame .. s-2, in that order
(projection_to_birds_eye_view).  Written with its own inverse (numpy's LU, where the kernel divides cofactors by the determinant) and
its own loops, so it shares no code with either implementation it judges."""
import numpy as np


def euler2mat64(angle):
    """utils/geometry.py:124-155 for one (rx, ry, rz): xmat @ ymat @ zmat, float64."""
    x, y, z = (float(v) for v in angle)
    cx, sx, cy, sy, cz, sz = np.cos(x), np.sin(x), np.cos(y), np.sin(y), np.cos(z), np.sin(z)
    xmat = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    ymat = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    zmat = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    return xmat @ ymat @ zmat


def pose64(vec):
    """utils/geometry.py:158-172: (tx, ty, tz, rx, ry, rz) -> 4x4, float64."""
    m = np.eye(4)
    m[:3, :3] = euler2mat64(vec[3:])
    m[:3, 3] = np.asarray(vec[:3], np.float64)
    return m


def affines64(intrinsics, extrinsics, future_egomotion):
    """intrinsics [b,s,n,3,3], extrinsics [b,s,n,4,4], future_egomotion [b,s,6] (any float dtype; promoted to float64 first, as both
    implementations promote their fp32 inputs) -> [b, s, n, 12] float64, not yet rounded to fp32."""
    K = np.asarray(intrinsics, np.float64)
    E = np.asarray(extrinsics, np.float64)
    ego = np.asarray(future_egomotion, np.float64)
    b, s, n = K.shape[:3]
    out = np.zeros((b, s, n, 12))
    for bi in range(b):
        poses = [pose64(ego[bi, t]) for t in range(s)]
        for t0 in range(s):
            for c in range(n):
                A = np.eye(4)
                A[:3, :3] = E[bi, t0, c, :3, :3] @ np.linalg.inv(K[bi, t0, c])
                A[:3, 3] = E[bi, t0, c, :3, 3]
                for t in range(t0, s - 1):
                    A = poses[t] @ A
                out[bi, t0, c] = A[:3].reshape(12)
    return out


def bound(ref64):
    """(ref32, tol) of the issue's derived bound |dev - ref32| <= 2^-23 |ref32| + 1e-9 max|row|: ref32 is the fp32 rounding of the
    float64 oracle; the first term is one fp32 rounding flip (two fp64 evaluations that differ by ~1e-13 relative can fall on either side
    of a rounding boundary), the second the fp64 work's own error at these condition numbers with four decades to spare, relative to
    the largest element of the camera's twelve."""
    ref32 = ref64.astype(np.float32)
    row = np.abs(ref32.astype(np.float64)).max(-1, keepdims=True)
    return ref32, 2.0 ** -23 * np.abs(ref32.astype(np.float64)) + 1e-9 * row


# the shapes the kernel test runs: no chain; a chain of one; a chain of two over several samples (a wrong multiplication order or a
# wrong sample's ego row shows); 65 cameras, one past a 64-thread block
SHAPES = [(1, 1, 1), (1, 2, 1), (2, 3, 6), (5, 1, 13)]


def general_rig(b, s, n, seed):
    """fp32 (intrinsics, extrinsics, future_egomotion) with general invertible K — skew, K[2][2] != 1, small entries below the
    diagonal, focal lengths 10^2 .. 10^3, and camera 0 of the LAST frame with its rows rotated (a permuted dominant diagonal) —
    rotations about all three axes (they do not commute) and non-zero translations in both the extrinsics and the ego-motion."""
    r = np.random.RandomState(seed)
    K = np.zeros((b, s, n, 3, 3))
    K[..., 0, 0] = 10.0 ** r.uniform(2.0, 3.0, (b, s, n))
    K[..., 1, 1] = 10.0 ** r.uniform(2.0, 3.0, (b, s, n))
    K[..., 2, 2] = r.uniform(0.8, 1.25, (b, s, n))
    K[..., 0, 1] = r.uniform(-5.0, 5.0, (b, s, n))                     # skew
    K[..., 0, 2] = r.uniform(100.0, 500.0, (b, s, n))
    K[..., 1, 2] = r.uniform(100.0, 500.0, (b, s, n))
    K[..., 1, 0] = r.uniform(-0.5, 0.5, (b, s, n))
    K[..., 2, 0] = r.uniform(-1e-4, 1e-4, (b, s, n))
    K[..., 2, 1] = r.uniform(-1e-4, 1e-4, (b, s, n))
    K[-1, -1, 0] = K[-1, -1, 0][[1, 2, 0]]                              # rows (1, 2, 0): the large entries leave the diagonal
    E = np.zeros((b, s, n, 4, 4))
    for idx in np.ndindex(b, s, n):
        E[idx][:3, :3] = euler2mat64(r.uniform(-3.0, 3.0, 3))
        E[idx][:3, 3] = r.uniform(-2.0, 2.0, 3)
        E[idx][3, 3] = 1.0
    ego = np.concatenate([r.uniform(-1.5, 1.5, (b, s, 3)), r.uniform(-0.6, 0.6, (b, s, 3))], -1)
    return K.astype(np.float32), E.astype(np.float32), ego.astype(np.float32)


def bad_rig(seed=7):
    """(sound rig, bad rig, the bad cameras' flat indices) of (b, s, n) = (1, 2, 3): six cameras; in the bad rig camera 1 has a
    singular K (rows 0 and 1 equal: the cofactor sum cancels to rounding noise, not to an exact zero) and camera 3 a K holding inf."""
    K, E, ego = general_rig(1, 2, 3, seed)
    Kb = K.copy().reshape(6, 3, 3)
    Kb[1, 1] = Kb[1, 0]
    Kb[3, 0, 2] = np.inf
    return (K, E, ego), (Kb.reshape(K.shape), E, ego), (1, 3)


# ---- timestamp sets of tests/test_gpu_model_graph.py: (camera, lidar, target) ------------------------------------------------------------
# A and B: the same sequence of jumps and steps and the same target selection (one Schedule.key()), different step sizes.
# C: another structure (the first LiDAR frame comes less than delta_t after the first camera frame: no step between their jumps)
TS_A = ([[-1.0, -0.5, 0.0]], [[-0.3, 0.0]], [[0.0, 0.5, 1.0]])
TS_B = ([[-1.0, -0.5, 0.0]], [[-0.28, 0.0]], [[0.0, 0.45, 1.0]])
TS_C = ([[-1.0, -0.5, 0.0]], [[-0.98, 0.0]], [[0.0, 0.5, 1.0]])
DELTA_T = 0.05      # default_cfg: MODEL.FUTURE_PRED.DELTA_T


def schedule_of(ts, delta_t=DELTA_T, variable=True, solver="euler"):
    """The Schedule FuturePredictionODE.forward builds for sample 0 of a timestamp set (camera and LiDAR both on)."""
    from streamingflow_amd import schedule as sched
    cam, lid, tgt = ts
    times, _ = sched.merge_observations(list(cam[0]), list(lid[0]))
    return sched.build_schedule([float(t) for t in times], [float(t) for t in tgt[0]], delta_t, variable, solver)
