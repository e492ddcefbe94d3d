"""Seeded cases of the scan registration (lidar_rt_amd/registration.py), shared by tests/test_registration.py and tests/test_registration_gpu.py.

The scene is analytic, so no tracer is needed: a sensor stands inside a room of eight planes n . x = d --

    a skewed box  x = 9, x = -6, y = 7, y = -11, floor z = -1.8, ceiling z = 6,
    two slanted walls  (0.8, 0.6, 0) . x = 8.0  and  (0.6, -0.7, 0.39) . x = 7.5

-- so that all six degrees of freedom are constrained.  The range of a pixel is the nearest positive ray-plane intersection along the local
direction of the ray grid.  The target sensor stands at ``base`` (the identity unless a case says otherwise), the source at ``base Exp(xi)`` with a
seeded ``xi``: the truth of the pair is ``X = Exp(xi)`` and a registration that starts at the identity starts ``xi`` away from it.

The shapes are the smallest at which the kernels can still go wrong: 16 x 128 (8 workgroups per pair: the order of the partial rows matters),
5 x 37 (a multiple of nothing, one partly filled workgroup), 8 x 40 with a Waymo per-beam table and a sensor2ego yaw, a motion that is mostly
yaw (partner windows cross the column seam), the largest window (rh = 4, rw = 16), three pairs of which one has an empty source mask and one a
zero normal image, and a target with two pixels that carry the same point (the tie rule).

RECORDED holds, per case, what the committed twin (``align_reference``) gives: its translation and rotation error against the truth and the
condition number of its last hessian.  tests/test_registration.py asserts twice the recorded errors and nothing looser (and, for the room cases,
less than 1 % of the initial offset); tests/test_registration_gpu.py uses the condition number in the bound of ``align`` against the twin.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from lidar_rt_amd import registration as rg, sweep as sw

PLANES = np.array([[1.0, 0.0, 0.0, 9.0], [-1.0, 0.0, 0.0, 6.0], [0.0, 1.0, 0.0, 7.0], [0.0, -1.0, 0.0, 11.0], [0.0, 0.0, -1.0, 1.8], [0.0, 0.0, 1.0, 6.0],
                   [0.8, 0.6, 0.0, 8.0], [0.6, -0.7, 0.39, 7.5]])
BOUNDS = [-0.43, 0.12]
ROOM_SCHEDULE = [tuple(r) for r in rg.DEFAULT_SCHEDULE]
WIDE_SCHEDULE = [(4, 16, 3.0)] * 3 + [(2, 8, 1.0)] * 3 + [(1, 2, 0.5)] * 4
SMALL_SCHEDULE = [(1, 2, 2.0)] * 3 + [(1, 1, 1.0)] * 5
WAYMO_S2E = np.array([[math.cos(0.4), -math.sin(0.4), 0.0, 1.2], [math.sin(0.4), math.cos(0.4), 0.0, 0.0], [0.0, 0.0, 1.0, 2.0], [0.0, 0.0, 0.0, 1.0]])


def waymo_table(H):
    return np.sort(np.random.default_rng(H).uniform(-0.40, 0.10, size=H)).astype(np.float32).astype(np.float64).tolist()


def twist(seed, trans, rot_deg, yaw_only=False):
    """A seeded xi = (rho, phi) with |rho| = trans [m] and |phi| = rot_deg [degrees]."""
    rng = np.random.default_rng(seed)
    rho, phi = rng.normal(size=3), rng.normal(size=3)
    if yaw_only:
        phi = np.array([0.02 * phi[0], 0.02 * phi[1], 1.0])
    rho[2] *= 0.3                                                            # a vehicle moves in its plane, mostly
    return np.concatenate([rho / np.linalg.norm(rho) * trans, phi / np.linalg.norm(phi) * math.radians(rot_deg)])


def exp4(xi):
    Re, te = rg.exp_reference(xi)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Re, te
    return T


# key: (H, W, inclination, data_type, sensor2ego, [xi per pair], schedule, min_pairs)
_SPECS = {
    "room_a": (16, 128, BOUNDS, "KITTI", None, [twist(1, 0.3, 2.0)], ROOM_SCHEDULE, 50),
    "room_b": (16, 128, BOUNDS, "KITTI", None, [twist(2, 0.8, 4.0)], ROOM_SCHEDULE, 50),
    "room_c": (16, 128, BOUNDS, "KITTI", None, [twist(3, 1.2, 3.0)], ROOM_SCHEDULE, 50),
    "odd": (5, 37, BOUNDS, "KITTI", None, [twist(4, 0.10, 1.0)], SMALL_SCHEDULE, 20),
    "waymo": (8, 40, "table", "Waymo", WAYMO_S2E, [twist(5, 0.15, 1.5)], SMALL_SCHEDULE, 20),
    "yaw": (16, 128, BOUNDS, "KITTI", None, [twist(6, 0.05, 8.0, yaw_only=True)], ROOM_SCHEDULE, 50),
    "wide": (16, 128, BOUNDS, "KITTI", None, [twist(7, 1.0, 5.0)], WIDE_SCHEDULE, 50),
    "batch3": (16, 128, BOUNDS, "KITTI", None, [twist(8, 0.3, 2.0), twist(9, 0.3, 2.0), twist(10, 0.4, 1.0)], ROOM_SCHEDULE, 50),
    "tie": (5, 37, BOUNDS, "KITTI", None, [twist(11, 0.05, 0.5)], SMALL_SCHEDULE, 20),
}
KEYS = tuple(_SPECS)
ROOM_KEYS = ("room_a", "room_b", "room_c")
ROOM_OFFSETS = {"room_a": (0.3, 2.0), "room_b": (0.8, 4.0), "room_c": (1.2, 3.0)}

# what align_reference gives on the case (pair 0): |t - t_true| [m], the rotation angle between R and R_true [rad], cond(hessian)
RECORDED = {
    "room_a": (1.886e-03, 8.322e-04, 2.635e+01),
    "room_b": (1.927e-03, 3.421e-04, 2.949e+01),
    "room_c": (9.621e-04, 7.532e-04, 3.340e+01),
    "odd": (1.795e-02, 3.139e-03, 2.779e+01),
    "waymo": (1.986e-02, 4.490e-03, 5.232e+01),
    "yaw": (4.334e-03, 5.669e-04, 3.054e+01),
    "wide": (3.167e-03, 7.849e-04, 3.165e+01),
    "batch3": (3.117e-03, 2.401e-04, 2.517e+01),
    "tie": (1.337e-02, 3.497e-03, 2.723e+01),
}
# the twin's odometry over odometry_frames(3): the error of the second and of the third pose (two compositions)
RECORDED_ODOMETRY = {12: (3.493e-03, 5.483e-04), 14: (5.533e-03, 1.015e-03)}


def local_directions(H, W, inclination, data_type, sensor2ego):
    """(H, W, 3) float32: the ray grid's directions in the sensor frame (what frame_geometry multiplies the ranges with)."""
    P = torch.eye(4, dtype=torch.float32)[:3].contiguous()
    _, d = sw.sweep_rays(P, None, H, W, inclination, data_type, sensor2ego)
    return d


def room_depth(d_local, pose):
    """(H, W) float32 ranges of a sensor at `pose` (4, 4) in the room: the nearest positive intersection of every ray with the eight planes."""
    d = d_local.numpy().astype(np.float64) @ pose[:3, :3].T
    o = pose[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (PLANES[:, 3] - PLANES[:, :3] @ o)[None, None, :] / (d @ PLANES[:, :3].T)
    t = np.where(t > 0.0, t, np.inf).min(-1)
    return torch.from_numpy(t.astype(np.float32))


def geometry(H, W, inclination, data_type, sensor2ego, pose):
    d_local = local_directions(H, W, inclination, data_type, sensor2ego)
    depth = room_depth(d_local, pose)
    mask = torch.isfinite(depth) & (depth > 0)
    depth = torch.where(mask, depth, torch.zeros_like(depth))
    return rg.frame_geometry(depth, mask, inclination, H, W, data_type, sensor2ego)


@functools.lru_cache(maxsize=None)
def case(key):
    """src, tgt: batched geometries (F, H, W, .) on the CPU; X_true (F, 3, 4) float64; kw: the sensor model; schedule, min_pairs."""
    H, W, inc, data_type, s2e, xis, schedule, min_pairs = _SPECS[key]
    inc = waymo_table(H) if inc == "table" else list(inc)
    base = exp4(np.array([0.5, -0.3, 0.1, 0.0, 0.0, 0.2])) if key == "wide" else np.eye(4)
    tgt = geometry(H, W, inc, data_type, s2e, base)
    srcs, truth = [], []
    for xi in xis:
        X = exp4(xi)
        srcs.append(geometry(H, W, inc, data_type, s2e, base @ X))
        truth.append(X[:3])
    sp, sn, sm = (torch.stack([s[k] for s in srcs]) for k in range(3))
    F = len(xis)
    tp, tn, tm = (tgt[k][None].expand(F, *tgt[k].shape).clone() for k in range(3))
    if key == "batch3":
        sm[1] = False                                                        # pair 1: no source pixel, status 1
        tn[2] = 0.0                                                          # pair 2: no usable normal, status 1 as well (no partner)
    if key == "tie":
        tp[0, 2, 11] = tp[0, 2, 10]                                          # two neighbouring target pixels carry the same point
        tn[0, 2, 11] = tn[0, 2, 10]
        tm[0, 2, 10] = tm[0, 2, 11] = True
    return SimpleNamespace(key=key, F=F, H=H, W=W, src=(sp, sn, sm), tgt=(tp, tn, tm), X_true=torch.from_numpy(np.stack(truth)), xi=np.stack(xis),
                           kw=dict(inclination=inc, data_type=data_type, sensor2ego=s2e), schedule=schedule, min_pairs=min_pairs,
                           n_valid=[int(sm[f].sum()) for f in range(F)])


def to_device(c, dev):
    mv = lambda g: tuple(t.to(dev) for t in g)
    return mv(c.src), mv(c.tgt)


def pose_error(X, X_true):
    """(|t - t_true|, the angle of R_true^T R) of two (3, 4) float64 poses."""
    X, T = np.asarray(X, np.float64), np.asarray(X_true, np.float64)
    R = T[:, :3].T @ X[:, :3]
    w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return float(np.linalg.norm(X[:, 3] - T[:, 3])), float(math.atan2(np.linalg.norm(w), 0.5 * (np.trace(R) - 1.0)))


@functools.lru_cache(maxsize=None)
def reference(key):
    """align_reference on the case from the identity, computed once and shared."""
    c = case(key)
    return rg.align_reference(c.src, c.tgt, None, c.schedule, min_pairs=c.min_pairs, **c.kw)


def linearize_points(c):
    """The X at which linearize is compared: the identity (the start) and the truth (the end) of every pair."""
    eye = torch.eye(4, dtype=torch.float64)[:3].expand(c.F, 3, 4).contiguous()
    return [("start", eye), ("truth", c.X_true.clone())]


def odometry_frames(n=3):
    """n frames of the 16 x 128 room along a seeded trajectory: ({id: geometry}, {id: (4, 4) true pose}, the sensor model)."""
    H, W, inc = 16, 128, list(BOUNDS)
    poses, T = {}, np.eye(4)
    for k in range(n):
        poses[10 + 2 * k] = T.copy()
        T = T @ exp4(twist(20, 0.35, 1.5) * (1.0 + 0.1 * k))                # a nearly constant velocity
    frames = {i: geometry(H, W, inc, "KITTI", None, P) for i, P in poses.items()}
    return frames, poses, dict(inclination=inc, data_type="KITTI", sensor2ego=None)
