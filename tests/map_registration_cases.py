"""Seeded cases of the scan-to-map registration (lidar_rt_amd/map_registration.py), shared by tests/test_map_registration.py and
tests/test_map_registration_gpu.py.  The scenes are those of tests/registration_cases.py (the analytic room, ``geometry``) and
tests/mesh_cases.py (the room grids fused by ``integrate_reference``, ``sdf_grid``), both imported.

* ``room1`` / ``room3``: the 17 x 19 x 23 room grid (voxel 0.9 m, trunc 2.7 m) fused from one and from three frames, at 5 x 37 (one partly
  filled workgroup), 9 x 61 (three workgroups, the last partly filled) and 16 x 128, in the KITTI-bounds and the Waymo-table convention.  The
  source is a scan of the room from ``P_0 Exp(xi)`` -- ``P_0`` the first fused frame's pose, ``xi`` seeded, 0.25 m and 1.5 degrees -- started at
  ``P_0``.
* ``batch3``: F = 3 on the room3 grid at 16 x 128: frame 1 has an empty mask, frame 2 lies wholly outside the grid (100 m away).
* ``sphere``: ``mesh_cases.sdf_grid("sphere")``, scanned from inside; the analytic gradient is the unit normal.
* ``thin2`` / ``thin1``: a sampled plane with a z axis of 2 voxels, and of 1 voxel (no domain: status FEW, X unchanged bit for bit).
* ``holes``: the sampled plane with unobserved voxels and an all-ones block; random points, a tenth of them outside the domain.
* ``last_centre``: points exactly on the last voxel centre of one, two and three axes: cell n - 2, fraction 1.  Its margin is 0 by construction
  (the point IS the boundary); the transform is the identity, so q is exact and the decision cannot differ.

A case is kept only if the twin's margin is at least ``mesh_cases.MARGIN`` (tests/test_map_registration.py checks; ``last_centre`` excepted).

RECORDED holds, per aligned case, what the committed twin gives for frame 0: the condition number of its last hessian (the bound of ``align_to_grid``
against the twin uses it), and its translation and rotation error against the truth.  RECORDED_SPHERE is the twin's largest |n - n_true| on the
sphere.  RECORDED_TRACKING are the last frame's errors of the 12-frame trajectory: map tracking (t [m], r [rad]) and the odometry chain (t, r).
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from lidar_rt_amd import map_registration as mr, mesh, registration as rg
from tests import mesh_cases as mcs
from tests import registration_cases as rc

MARGIN = mcs.MARGIN
SIZES = ((5, 37), (9, 61), (16, 128))
CONVENTIONS = mcs.CONVENTIONS
ROOM_DIMS = (17, 19, 23)
ROOM_KEYS = tuple(f"room{F}_{H}x{W}_{conv}" for F in (1, 3) for H, W in SIZES for conv in CONVENTIONS)
ALIGN_KEYS = ROOM_KEYS + ("batch3", "thin1")
LINEARIZE_KEYS = ROOM_KEYS + ("batch3", "sphere", "thin2", "thin1", "holes", "last_centre")
ITERS = 8
HUBER = 0.1

# cond(hessian), |t - t_true| [m], rotation error [rad] of align_to_grid_reference on frame 0 of the case
RECORDED = {
    "room1_5x37_kitti_bounds": (5.373e+02, 1.923e-01, 5.331e-02),
    "room1_5x37_waymo_table": (9.687e+02, 2.760e-01, 1.921e-02),
    "room1_9x61_kitti_bounds": (4.160e+02, 1.379e-01, 2.791e-02),
    "room1_9x61_waymo_table": (4.739e+02, 1.333e-01, 1.982e-02),
    "room1_16x128_kitti_bounds": (4.654e+02, 6.416e-02, 1.113e-02),
    "room1_16x128_waymo_table": (3.664e+02, 2.448e-02, 1.350e-02),
    "room3_5x37_kitti_bounds": (2.352e+02, 4.119e-02, 8.272e-03),
    "room3_5x37_waymo_table": (5.292e+02, 6.908e-02, 9.651e-03),
    "room3_9x61_kitti_bounds": (2.807e+02, 6.284e-02, 6.236e-03),
    "room3_9x61_waymo_table": (1.870e+02, 3.844e-02, 2.124e-02),
    "room3_16x128_kitti_bounds": (4.236e+02, 3.235e-02, 1.966e-03),
    "room3_16x128_waymo_table": (3.082e+02, 1.736e-02, 7.678e-03),
    "batch3": (4.236e+02, 3.235e-02, 1.966e-03),
}
# these grids have voxels of 0.9 m, made to be small, not accurate: the errors above are large and say so.  The start is 0.25 m and 26 mrad off.
RECORDED_SPHERE = 1.275e-01                                                  # the bound of sphere_normals() is 0.978: h / rho is a third here
RECORDED_TRACKING = (7.040e-03, 4.750e-04, 2.909e-02, 4.618e-03)            # 32 x 256, voxel 0.2 m, trunc 0.8 m, 12 frames


def plane_grid(dims, voxel=0.3, trunc=0.9):
    """A sampled tilted plane (0.36, 0.48, 0.8) . x = d through the middle of the grid, weight 1 everywhere."""
    g = mesh.TsdfGrid((0.0, 0.0, 0.0), voxel, dims, trunc, intensity=False)
    c = [mesh.centres(voxel, n).astype(np.float64) for n in dims]
    x, y, z = np.meshgrid(*c, indexing="ij")
    nrm = np.array([0.36, 0.48, 0.8])
    mid = np.array([d * voxel / 2 for d in dims])
    f = nrm[0] * x + nrm[1] * y + nrm[2] * z - float(nrm @ mid) + 0.0137
    g.tsdf[:] = torch.from_numpy(np.clip(f / trunc, -1, 1).astype(np.float32))
    g.weight[:] = 1
    return g


def random_points(seed, dims, voxel, H, W, outside=0.1):
    """(points (1, H, W, 3) float32, mask (1, H, W)): uniform in the box of the voxel centres, a share `outside` up to one voxel beyond it."""
    rng = np.random.default_rng(seed)
    lo, hi = 0.5 * voxel, (np.array(dims) - 0.5) * voxel
    p = rng.uniform(lo, np.maximum(hi, lo + 1e-3), (H * W, 3))
    out = rng.uniform(size=H * W) < outside
    p[out] += rng.choice([-1.0, 1.0], (int(out.sum()), 3)) * rng.uniform(0.0, voxel, (int(out.sum()), 3)) + rng.choice([0.0, 1.0], (int(out.sum()), 3)) * (hi - lo)
    m = rng.uniform(size=H * W) > 0.05
    return torch.from_numpy(p.astype(np.float32).reshape(1, H, W, 3)), torch.from_numpy(m.reshape(1, H, W))


def _eye(F):
    return torch.eye(4, dtype=torch.float64)[:3].expand(F, 3, 4).contiguous()


def _case(key, grid, src, X_start, X_true=None, min_pairs=10):
    F, H, W = (int(x) for x in src[0].shape[:3])
    return SimpleNamespace(key=key, grid=grid, src=src, F=F, H=H, W=W, X_start=X_start, X_true=X_true, min_pairs=min_pairs, iters=ITERS, huber=HUBER,
                           n_valid=[int(src[1][f].sum()) for f in range(F)])


def _room(F, H, W, conv, n_src=1):
    grid, margin = mcs.room_reference(ROOM_DIMS, F, H, W, conv, False)
    assert margin >= MARGIN
    fr = mcs.room_frames(F, H, W, conv)
    kw = mcs.convention(conv, H)
    P0 = fr["sensor2world"][0]
    pts, msk, truth = [], [], []
    for k in range(n_src):
        T = P0 @ rc.exp4(rc.twist(60 + k, 0.25, 1.5))
        g = rc.geometry(H, W, kw["inclination"], kw["data_type"], kw["sensor2ego"], T)
        pts.append(g[0]); msk.append(g[2]); truth.append(mr.grid_pose(grid, T)[:3])
    start = torch.from_numpy(np.stack([mr.grid_pose(grid, P0)[:3]] * n_src))
    return grid, (torch.stack(pts), torch.stack(msk)), start, torch.from_numpy(np.stack(truth))


@functools.lru_cache(maxsize=None)
def case(key):
    """grid: a CPU TsdfGrid; src: (points (F, H, W, 3), mask (F, H, W)); X_start, X_true (F, 3, 4) float64 in the grid frame (X_true may be None)."""
    if key.startswith("room"):
        F, size, conv = key[4:].split("_", 2)
        H, W = (int(x) for x in size.split("x"))
        return _case(key, *_room(int(F), H, W, conv))
    if key == "batch3":
        grid, (p, m), start, truth = _room(3, 16, 128, "kitti_bounds", 3)
        m = m.clone()
        m[1] = False                                                         # frame 1: no source pixel, status 1
        start, truth = start.clone(), truth.clone()
        start[2, :, 3] += 100.0                                              # frame 2: wholly outside the grid, status 1 as well
        return _case(key, grid, (p, m), start, truth)
    if key == "sphere":
        grid = mcs.sdf_grid("sphere")
        dims, voxel = grid.dims, grid.voxel
        centre = np.array([d * voxel / 2 for d in dims]) - np.array([0.013, -0.007, 0.003])
        H, W = 9, 61
        d = rc.local_directions(H, W, [-1.2, 1.2], "KITTI", None).numpy().astype(np.float64)
        o = np.array([0.11, -0.07, 0.05])                                    # the sensor, off the centre
        b = d @ o
        t = -b + np.sqrt(b * b - (o @ o - 1.2 ** 2))                         # |o + t d| = 1.2
        p = (d * t[..., None]).astype(np.float32)
        X = np.eye(4)[:3].copy()
        X[:, 3] = centre + o
        c = _case(key, grid, (torch.from_numpy(p)[None], torch.ones((1, H, W), dtype=torch.bool)), torch.from_numpy(X[None]))
        c.centre = centre
        return c
    if key in ("thin2", "thin1"):
        dims = (12, 9, 2 if key == "thin2" else 1)
        grid = plane_grid(dims)
        return _case(key, grid, random_points(7, dims, grid.voxel, 3, 50), _eye(1))
    if key == "holes":
        dims = (11, 12, 9)
        grid = plane_grid(dims)
        grid.weight[2:4, 3:6, 1:8] = 0                                       # unobserved voxels
        grid.weight[9, 10, 4] = 0
        grid.tsdf[6:10, 1:5, 0:9] = 1.0                                      # an all-ones block: free space
        return _case(key, grid, random_points(8, dims, grid.voxel, 5, 60), _eye(1))
    if key == "last_centre":
        dims = (6, 5, 4)
        grid = plane_grid(dims)
        last = [float(mesh.centres(grid.voxel, n)[-1]) for n in dims]
        inner = [float(mesh.centres(grid.voxel, n)[1]) + 0.011 for n in dims]
        p = np.array([[last[a] if (k >> a) & 1 else inner[a] for a in range(3)] for k in range(8)], np.float32)
        return _case(key, grid, (torch.from_numpy(p.reshape(1, 1, 8, 3)), torch.ones((1, 1, 8), dtype=torch.bool)), _eye(1))
    raise KeyError(key)


def linearize_points(c):
    """The X at which linearize_to_grid is compared: the start and (where there is one) the truth of every frame."""
    return [("start", c.X_start)] + ([("truth", c.X_true)] if c.X_true is not None else [])


@functools.lru_cache(maxsize=None)
def linearize_reference(key, at):
    """(sums, cell, abs_sums, margin) of the twin, computed once and shared."""
    c = case(key)
    return mr.linearize_to_grid_reference(c.grid, c.src, dict(linearize_points(c))[at], c.huber, return_abs=True)


@functools.lru_cache(maxsize=None)
def reference(key):
    """align_to_grid_reference on the case from its start, computed once and shared."""
    c = case(key)
    return mr.align_to_grid_reference(c.grid, c.src, c.X_start, c.iters, c.huber, min_pairs=c.min_pairs)


def to_device(c, dev):
    return c.grid.to(dev), tuple(t.to(dev) for t in c.src)


def sphere_normals():
    """(the twin's n (N, 3), the analytic unit normals (N, 3), the bound) over the sphere case's pixels that have a term.

    The bound.  f = |x - centre| - r is sampled at the voxel centres; the cell's corners lie within h sqrt(3) of q, so that (q on the surface,
    rho = r) every corner has rho >= r - h sqrt(3) =: rho_min and |f| <= h sqrt(3) < trunc: no corner is clipped.  A difference quotient along an
    edge parallel to axis a is d_a f at some point xi of that edge (mean value theorem), the twin's n_a is a convex combination of four of them,
    and |d_a f(xi) - d_a f(q)| <= M |xi - q| <= M h sqrt(3), where M = 1 / rho_min bounds the second derivative of a distance to a point -- the
    second difference of the sampled distance, over h^2.  Three components: |n - n_true| <= sqrt(3) sqrt(3) h / rho_min = 3 h / (r - h sqrt(3)),
    plus the float32 rounding of the samples, 2^-24 trunc / h per quotient."""
    c = case("sphere")
    ts, wt = mr._grid_np(c.grid)
    o = mr.pixels_reference(ts, wt, c.grid.voxel, c.grid.trunc, 1, c.X_start[0].numpy(), c.src[0][0].numpy(), c.src[1][0].numpy(), 1e9)
    has = o.cell >= 0
    X = c.X_start[0].numpy()
    q = c.src[0][0].numpy().reshape(-1, 3).astype(np.float64) + X[:, 3]
    true = (q - c.centre) / np.linalg.norm(q - c.centre, axis=1, keepdims=True)
    h, r = c.grid.voxel, 1.2
    bound = 3.0 * h / (r - h * math.sqrt(3.0)) + math.sqrt(3.0) * 2.0 ** -24 * c.grid.trunc / h * 2.0
    return o.n[has], true[has], bound, int(has.sum()), int(has.size)


# ---- tracking -----------------------------------------------------------------------------------------------------------------------------------------------

def trajectory(n, H, W):
    """n frames of the room along a seeded trajectory of about 0.35 m and 1.5 degrees per step: ({id: geometry}, {id: (depth, mask)}, {id: true pose},
    the sensor model)."""
    inc = list(rc.BOUNDS)
    poses, T = {}, np.eye(4)
    for k in range(n):
        poses[k] = T.copy()
        T = T @ rc.exp4(rc.twist(20, 0.35, 1.5) * (1.0 + 0.1 * (k % 3)))
    d_local = rc.local_directions(H, W, inc, "KITTI", None)
    frames, images = {}, {}
    for i, P in poses.items():
        d = rc.room_depth(d_local, P)
        m = torch.isfinite(d) & (d > 0)
        d = torch.where(m, d, torch.zeros_like(d))
        frames[i] = rg.frame_geometry(d, m, inc, H, W, "KITTI", None)
        images[i] = (d, m)
    return frames, images, poses, dict(inclination=inc, data_type="KITTI", sensor2ego=None)


def tracking_grid(frames, chain, voxel, trunc, device="cpu"):
    """The grid ``ingest --map-tracking`` makes: sized by mesh.grid_bounds from the chain's poses."""
    world = [dict(world=frames[i][0].numpy().astype(np.float64) @ chain[i][:3, :3].T + chain[i][:3, 3], mask=frames[i][2].numpy()) for i in sorted(frames)]
    origin, dims = mesh.grid_bounds(world, voxel, trunc)
    return mesh.TsdfGrid(origin, voxel, dims, trunc, device=device, intensity=False)


@functools.lru_cache(maxsize=None)
def tracking(n=12, H=32, W=256, voxel=0.2, trunc=0.8):
    """The twins on the trajectory: namespace(chain, tracked: {id: (4, 4)}, truth, steps, report, errors of the last frame, the grid)."""
    frames, images, truth, kw = trajectory(n, H, W)
    chain, rep = rg.odometry(frames, return_steps=True, **kw)
    steps = {s["source"]: np.vstack([s["X"], [0.0, 0.0, 0.0, 1.0]]) for s in rep["steps"]}
    grid = tracking_grid(frames, chain, voxel, trunc)
    tracked, report = mr.track_and_fuse(grid, frames, images, steps=steps, **kw)
    last = max(truth)
    return SimpleNamespace(frames=frames, images=images, truth=truth, chain=chain, tracked=tracked, steps=steps, report=report, grid=grid, kw=kw,
                           map_error=rc.pose_error(tracked[last][:3], truth[last][:3]), chain_error=rc.pose_error(chain[last][:3], truth[last][:3]))
