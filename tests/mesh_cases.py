"""Seeded cases of the surface meshes (lidar_rt_amd/mesh.py), shared by tests/test_mesh.py and tests/test_mesh_gpu.py.

* Random-sign grids of 9 x 10 x 11 with a positive border layer, all voxels observed: every surface is closed.  SEEDS is enough seeds for all 256
  configurations to occur (tests/test_mesh.py asserts the coverage).
* Posed range images of the analytic room of tests/registration_cases.py (the same ray grids, ranges and conventions, unchanged): integrated into
  grids of 3 x 5 x 7 (fewer voxels than one workgroup), 17 x 19 x 23 (several workgroups, not a multiple of 256) and 1 x 9 x 40, with masks that
  have holes and grids partly outside every frame.
* The analytic sphere: a sensor at the centre of a sphere of radius R, depth R in every pixel, in two orientations (identity and a 90 degree roll).

Every integrated case asserts the twin's ``margin >= 1e-9`` as a condition on its inputs (the grid origins carry small offsets for it).
"""
import functools
import math

import numpy as np
import torch

from lidar_rt_amd import mesh
from tests import registration_cases as rc

MARGIN = 1e-9
SEEDS = tuple(range(12))
RANDOM_DIMS = (9, 10, 11)
CONVENTIONS = ("kitti_bounds", "waymo_table")
SIZES = ((5, 37), (8, 64), (16, 128))
# dims -> (voxel, origin): placed across the walls of the room (x = 9, y = 7, the floor z = -1.8), partly outside every frame's view or range
GRIDS = {
    (3, 5, 7): (0.6, (7.9013, -1.4027, -2.3031)),
    (17, 19, 23): (0.9, (-6.6017, -11.4021, -2.5029)),
    (1, 9, 40): (0.35, (8.8011, -1.5023, -2.6019)),
}
SPHERE_R, SPHERE_S = 2.0, 0.25
SPHERE_SHIFT = (0.0123, -0.0071, 0.0037)


def random_grid(seed, dims=RANDOM_DIMS, border=True, intensity=True):
    """A CPU grid of random tsdf in [-1, 1] (a positive border layer), weight 1 everywhere, random intensity."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-1.0, 1.0, dims).astype(np.float32)
    if border:
        t[[0, -1]] = 1.0
        t[:, [0, -1]] = 1.0
        t[:, :, [0, -1]] = 1.0
    g = mesh.TsdfGrid((0.25, -0.5, 1.0), 0.5, dims, intensity=intensity)
    g.tsdf[:] = torch.from_numpy(t)
    g.weight[:] = 1
    if intensity:
        g.intensity[:] = torch.from_numpy(rng.uniform(0.0, 1.0, dims).astype(np.float32))
    return g


def configurations(g):
    """The set of configurations of a grid's cells (all observed)."""
    neg = g.tsdf.numpy() < 0
    X, Y, Z = g.dims
    cfg = np.zeros((X - 1, Y - 1, Z - 1), np.int64)
    for n in range(8):
        cfg |= neg[n & 1:X - 1 + (n & 1), n >> 1 & 1:Y - 1 + (n >> 1 & 1), n >> 2 & 1:Z - 1 + (n >> 2 & 1)].astype(np.int64) << n
    return set(np.unique(cfg).tolist())


def sdf_grid(kind, dims=(14, 15, 13), voxel=0.25):
    """A sampled analytic signed distance, positive outside: a sphere or a torus, weight 1 everywhere."""
    g = mesh.TsdfGrid((0.0, 0.0, 0.0), voxel, dims, intensity=False)
    c = [mesh.centres(voxel, n).astype(np.float64) for n in dims]
    x, y, z = np.meshgrid(*c, indexing="ij")
    x, y, z = x - dims[0] * voxel / 2 + 0.013, y - dims[1] * voxel / 2 - 0.007, z - dims[2] * voxel / 2 + 0.003
    if kind == "sphere":
        f = np.sqrt(x * x + y * y + z * z) - 1.2
    else:
        f = np.sqrt((np.sqrt(x * x + y * y) - 1.0) ** 2 + z * z) - 0.45
    g.tsdf[:] = torch.from_numpy(np.clip(f / (3 * voxel), -1, 1).astype(np.float32))
    g.weight[:] = 1
    return g


def convention(name, H):
    if name == "kitti_bounds":
        return dict(inclination=list(rc.BOUNDS), data_type="KITTI", sensor2ego=None)
    return dict(inclination=rc.waymo_table(H), data_type="Waymo", sensor2ego=rc.WAYMO_S2E)


@functools.lru_cache(maxsize=None)
def room_frames(F, H, W, conv, seed=0):
    """F posed range images of the room: depth, mask (with holes), intensity (F, H, W), sensor2world (F, 4, 4) float64, and the convention."""
    kw = convention(conv, H)
    d_local = rc.local_directions(H, W, kw["inclination"], kw["data_type"], kw["sensor2ego"])
    rng = np.random.default_rng(100 + seed)
    depth, mask, inten, poses = [], [], [], []
    for f in range(F):
        P = rc.exp4(rc.twist(40 + 7 * seed + f, 0.6 + 0.2 * f, 4.0 + f))
        d = rc.room_depth(d_local, P)
        m = torch.isfinite(d) & (d > 0) & torch.from_numpy(rng.uniform(size=(H, W)) > 0.2)      # holes
        depth.append(torch.where(m, d, torch.zeros_like(d)))
        mask.append(m)
        inten.append(torch.from_numpy(rng.uniform(0.0, 1.0, (H, W)).astype(np.float32)))
        poses.append(P)
    st = lambda xs, shape, dt: torch.stack(xs) if xs else torch.zeros(shape, dtype=dt)
    return dict(depth=st(depth, (0, H, W), torch.float32), mask=st(mask, (0, H, W), torch.bool), intensity=st(inten, (0, H, W), torch.float32),
                sensor2world=np.stack(poses) if poses else np.zeros((0, 4, 4)), **kw)


def room_grid(dims, intensity=True, device="cpu"):
    voxel, origin = GRIDS[dims]
    return mesh.TsdfGrid(origin, voxel, dims, device=device, intensity=intensity)


def frames_to(fr, dev, intensity=True):
    return dict(depth=fr["depth"].to(dev), mask=fr["mask"].to(dev), sensor2world=fr["sensor2world"], inclination=fr["inclination"],
                data_type=fr["data_type"], sensor2ego=fr["sensor2ego"], intensity=fr["intensity"].to(dev) if intensity else None)


@functools.lru_cache(maxsize=None)
def room_reference(dims, F, H, W, conv, intensity=True, calls=1):
    """The twin's grid after `calls` integrate calls of F frames each (the second call with the frames of seed 1), and the smallest margin."""
    g = room_grid(dims, intensity)
    margin = math.inf
    for c in range(calls):
        margin = min(margin, mesh.integrate_reference(g, **frames_to(room_frames(F, H, W, conv, c), "cpu", intensity)))
    return g, margin


def sphere_frames(H=16, W=32, intensity=(0.25, 0.75)):
    """Two frames of a sensor at the world origin inside a sphere of radius R: identity and a 90 degree roll about x; inclination bounds +-1.2."""
    roll = np.eye(4)
    roll[1:3, 1:3] = [[0.0, -1.0], [1.0, 0.0]]
    depth = torch.full((2, H, W), SPHERE_R, dtype=torch.float32)
    inten = torch.stack([torch.full((H, W), v, dtype=torch.float32) for v in intensity])
    return dict(depth=depth, mask=torch.ones((2, H, W), dtype=torch.bool), sensor2world=np.stack([np.eye(4), roll]), inclination=[-1.2, 1.2],
                data_type="KITTI", sensor2ego=None, intensity=inten)


def sphere_grid(device="cpu"):
    s, R = SPHERE_S, SPHERE_R
    half = int(math.ceil((R + 3 * s + s) / s)) + 1                              # the sphere, the truncation band and one voxel more
    origin = np.array([-half * s, -half * s, -half * s]) + np.array(SPHERE_SHIFT)
    return mesh.TsdfGrid(origin, s, (2 * half, 2 * half, 2 * half), trunc=3 * s, device=device, intensity=True)


@functools.lru_cache(maxsize=None)
def sphere_reference():
    g = sphere_grid()
    margin = mesh.integrate_reference(g, **sphere_frames())
    return g, margin
