"""Seeded cases of the ray casting (lidar_rt_amd/raycast.py), shared by tests/test_raycast.py and tests/test_raycast_gpu.py.

* The hand case: a (2, 2, 8) grid with a linear tsdf along z, one z-layer of weight 1 that min_weight 2 leaves unobserved.
* A plane x = PLANE_X0 in an axis-aligned grid: voxel 0.25, the plane at a dyadic offset and trunc a power of two, so that every tsdf is exact in
  float32; rays that cross it from inside and from outside the grid, rays parallel to it and rays pointing away.
* Oblique planes: trunc = 3 voxels (clipped), random normals, rays with |n.u| >= 0.35 whose plane hit lies at least 0.3 m inside the box of centres.
* The sphere of tests/mesh_cases.py (sdf_grid("sphere"): R = 1.2, h = 0.25, trunc 3 h) and rays aimed at its centre from distances in
  [R + trunc + step, 4], inside and outside the grid.
* The room grids of tests/mesh_cases.py (integrate's twin on the analytic room), cast with the rays of room frames of another seed.
* Rays that must miss with 0 samples: a non-finite origin or direction, a zero direction.
"""
import functools
import math

import numpy as np
import torch

from lidar_rt_amd import mesh
from lidar_rt_amd.training import RangeFrames
from tests import mesh_cases as mcs
from tests import registration_cases as rc

U23 = 2.0 ** -23

# ---- the hand case ------------------------------------------------------------------------------------------------------------------------------------------
HAND_CROSS = 4.25                                                            # tsdf (4.25 - z) / 4 on the centres z = 0.5 ... 7.5


def hand_grid(unobserved_layer=1):
    """(2, 2, 8), voxel 1, trunc 4, origin 0: tsdf[.., k] = (4.25 - c_k) / 4, intensity c_k / 8, weight 2 but 1 in z-layer `unobserved_layer`."""
    g = mesh.TsdfGrid((0.0, 0.0, 0.0), 1.0, (2, 2, 8), trunc=4.0, intensity=True)
    c = mesh.centres(1.0, 8).astype(np.float64)
    g.tsdf[:] = torch.from_numpy(((HAND_CROSS - c) / 4.0).astype(np.float32))
    g.intensity[:] = torch.from_numpy((c / 8.0).astype(np.float32))
    g.weight[:] = 2
    g.weight[:, :, unobserved_layer] = 1
    return g


# ---- planes -------------------------------------------------------------------------------------------------------------------------------------------------
PLANE_DIMS, PLANE_VOXEL, PLANE_TRUNC, PLANE_X0 = (12, 16, 16), 0.25, 0.5, 1.3125
PLANE_ORIGIN = (10.0, -3.0, 0.5)


def planar_grid(intensity=True, device="cpu"):
    """tsdf = clip((c_x - PLANE_X0) / trunc, -1, 1): exact in float32; intensity c_y / 4, weight 1."""
    g = mesh.TsdfGrid(PLANE_ORIGIN, PLANE_VOXEL, PLANE_DIMS, trunc=PLANE_TRUNC, intensity=intensity)
    c = [mesh.centres(PLANE_VOXEL, n).astype(np.float64) for n in PLANE_DIMS]
    x, y, _ = np.meshgrid(*c, indexing="ij")
    g.tsdf[:] = torch.from_numpy(np.clip((x - PLANE_X0) / PLANE_TRUNC, -1.0, 1.0).astype(np.float32))
    if intensity:
        g.intensity[:] = torch.from_numpy((y / 4.0).astype(np.float32))
    g.weight[:] = 1
    return g.to(device)


def rule_ray(ro, rd, origin):
    """The rule's o and u in float64 (lrt_raycast_math.h) of float32 world rays."""
    o = ro.astype(np.float64) - np.asarray(origin, np.float64)[None]
    d = rd.astype(np.float64)
    return o, d / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]


def slab(o, u, dims, voxel):
    """(t_in, t_out) of the box of centres, unclipped by the depths (u has no zero component here)."""
    lo = np.array([mesh.centres(voxel, n)[0] for n in dims], np.float64)
    hi = np.array([mesh.centres(voxel, n)[-1] for n in dims], np.float64)
    t1, t2 = (lo - o) / u, (hi - o) / u
    return np.minimum(t1, t2).max(1), np.maximum(t1, t2).min(1)


@functools.lru_cache(maxsize=None)
def planar_rays(seed=0, n=400):
    """(rays_o, rays_d (n, 3) float32 world, t_exact (n,) float64) crossing the plane: hit points in the middle of the plane, directions with
    -u_x >= 0.5, origins 0.4 to 3 m before the hit -- inside the grid and outside it (x beyond the box); kept where the entry lies at least 0.3 m
    before the hit, so that the first sample is positive."""
    rng = np.random.default_rng(seed)
    hitp = np.stack([np.full(4 * n, PLANE_X0), rng.uniform(1.0, 3.0, 4 * n), rng.uniform(1.0, 3.0, 4 * n)], 1)
    ux = -rng.uniform(0.5, 1.0, 4 * n)
    ang = rng.uniform(0, 2 * math.pi, 4 * n)
    lat = np.sqrt(1 - ux * ux)
    u = np.stack([ux, lat * np.cos(ang), lat * np.sin(ang)], 1)
    o = hitp - rng.uniform(0.4, 3.0, 4 * n)[:, None] * u
    ro = (o + np.asarray(PLANE_ORIGIN)).astype(np.float32)
    rd = u.astype(np.float32)
    o64, u64 = rule_ray(ro, rd, PLANE_ORIGIN)
    t_exact = (o64[:, 0] - PLANE_X0) / -u64[:, 0]
    t_in, t_out = slab(o64, u64, PLANE_DIMS, PLANE_VOXEL)
    keep = (t_exact - np.maximum(t_in, 0.0) >= 0.3) & (t_exact + 0.3 <= t_out)
    idx = np.nonzero(keep)[0][:n]
    return ro[idx], rd[idx], t_exact[idx]


def planar_missing_rays():
    """Rays parallel to the plane (on its positive side) and rays pointing away from it: (rays_o, rays_d) float32 world."""
    og = np.asarray(PLANE_ORIGIN)
    o = np.array([[2.0, 0.5, 0.5], [2.5, 3.0, 1.0], [2.6, 2.0, 2.0], [2.0, 2.0, 2.0], [0.5, 2.0, 2.0], [1.9, -1.0, 1.5]])
    d = np.array([[0.0, 0.6, 0.8], [0.0, -1.0, 0.0], [0.0, 0.3, -0.2], [0.9, 0.3, 0.1], [-1.0, 0.1, 0.0], [0.0, 1.0, 0.0]])
    return (o + og).astype(np.float32), d.astype(np.float32)


OBLIQUE_DIMS, OBLIQUE_ORIGIN = (12, 13, 11), (-1.5, 2.25, 0.75)


@functools.lru_cache(maxsize=None)
def oblique_case(seed):
    """(grid (trunc 3 voxels, clipped), rays_o, rays_d, t_exact, |n.u|) of one random plane through the box: rays with |n.u| >= 0.35 whose plane
    hit lies at least 0.3 m inside the box of centres."""
    rng = np.random.default_rng(1000 + seed)
    v = 0.25
    g = mesh.TsdfGrid(OBLIQUE_ORIGIN, v, OBLIQUE_DIMS, trunc=3 * v, intensity=True)
    c = [mesh.centres(v, n).astype(np.float64) for n in OBLIQUE_DIMS]
    x, y, z = np.meshgrid(*c, indexing="ij")
    nrm = rng.normal(size=3)
    nrm /= np.linalg.norm(nrm)
    p0 = np.array([1.5, 1.6, 1.4]) + rng.uniform(-0.2, 0.2, 3)
    fp = (x - p0[0]) * nrm[0] + (y - p0[1]) * nrm[1] + (z - p0[2]) * nrm[2]
    g.tsdf[:] = torch.from_numpy(np.clip(fp / g.trunc, -1, 1).astype(np.float32))
    g.intensity[:] = torch.from_numpy(rng.uniform(0, 1, OBLIQUE_DIMS).astype(np.float32))
    g.weight[:] = 1
    m = 200
    o = p0 + nrm * rng.uniform(1.0, 1.3, (m, 1)) + rng.uniform(-0.3, 0.3, (m, 3))
    w = rng.normal(size=(m, 3))
    w -= (w @ nrm)[:, None] * nrm
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    a = rng.uniform(0.35, 1.0, (m, 1))
    u = -a * nrm + np.sqrt(1 - a * a) * w
    ro = (o + np.asarray(OBLIQUE_ORIGIN)).astype(np.float32)
    rd = u.astype(np.float32)
    o64, u64 = rule_ray(ro, rd, OBLIQUE_ORIGIN)
    nu = -(u64 @ nrm)
    t_exact = ((o64 - p0) @ nrm) / nu
    pe = o64 + t_exact[:, None] * u64
    lo = np.array([cc[0] for cc in c]) + 0.3
    hi = np.array([cc[-1] for cc in c]) - 0.3
    keep = (nu >= 0.35) & np.all((pe > lo) & (pe < hi), 1)
    return g, ro[keep], rd[keep], t_exact[keep], nu[keep]


# ---- the sphere ---------------------------------------------------------------------------------------------------------------------------------------------
SPHERE_R, SPHERE_H = 1.2, 0.25


def sphere_centre(dims=(14, 15, 13), voxel=0.25):
    """The centre of mesh_cases.sdf_grid("sphere") in its grid frame (origin 0)."""
    return np.array([dims[0] * voxel / 2 - 0.013, dims[1] * voxel / 2 + 0.007, dims[2] * voxel / 2 - 0.003])


def sphere_delta(step=0.5 * SPHERE_H, trunc=3 * SPHERE_H):
    return 3 * SPHERE_H ** 2 / (8 * (SPHERE_R - step - math.sqrt(3) * SPHERE_H)) + U23 * trunc


@functools.lru_cache(maxsize=None)
def sphere_rays(seed=0, n=500):
    """(rays_o, rays_d float32, t_exact float64): rays aimed at the centre from distances in [R + trunc + step, 4]; t_exact the rule's ray's
    intersection with the sphere.  Uniform directions and distances put few origins inside the box of centres (its corners lie 2.8 m from the
    centre), so candidates are drawn until half the rays start inside it and half outside, alternating."""
    rng = np.random.default_rng(seed)
    ctr = sphere_centre()
    dims = np.array((14, 15, 13))
    d = rng.normal(size=(16 * n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dist = rng.uniform(SPHERE_R + 3 * SPHERE_H + 0.5 * SPHERE_H, 4.0, (16 * n, 1))
    ro, rd = (ctr + dist * d).astype(np.float32), (-d).astype(np.float32)
    o, _ = rule_ray(ro, rd, (0.0, 0.0, 0.0))
    inside = np.all((o >= 0.5 * SPHERE_H) & (o <= (dims - 0.5) * SPHERE_H), 1)
    pick = np.stack([np.nonzero(inside)[0][:n // 2], np.nonzero(~inside)[0][:n // 2]], 1).reshape(-1)
    ro, rd = ro[pick], rd[pick]
    o, u = rule_ray(ro, rd, (0.0, 0.0, 0.0))
    b = np.einsum("ij,ij->i", u, o - ctr)
    cc = np.einsum("ij,ij->i", o - ctr, o - ctr) - SPHERE_R ** 2
    return ro, rd, -b - np.sqrt(b * b - cc)


# ---- the room -----------------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def room_rays(F, H, W, conv, seed=1):
    """(rays_o, rays_d) (F, H, W, 3) float32: the range rays of the room frames of `seed` (other poses than the fused frames of seed 0)."""
    fr = mcs.room_frames(F, H, W, conv, seed)
    s2e = None if fr["sensor2ego"] is None else torch.as_tensor(np.asarray(fr["sensor2ego"]), dtype=torch.float32)
    o, d = [], []
    for P in fr["sensor2world"]:
        a, b = RangeFrames.range_rays(H, W, fr["inclination"], torch.as_tensor(P, dtype=torch.float32), fr["data_type"], s2e)
        o.append(a)
        d.append(b)
    if not o:
        return torch.zeros((0, H, W, 3)), torch.zeros((0, H, W, 3))
    return torch.stack(o).contiguous(), torch.stack(d).contiguous()


def room_grid(dims, conv, intensity=True):
    """The twin's room grid of mesh_cases (3 frames of 8 x 64 of seed 0), and its margin."""
    return mcs.room_reference(dims, 3, 8, 64, conv, intensity)


def bad_rays():
    """Rays that miss with 0 samples: a NaN or infinite origin or direction component, a zero direction."""
    nan, inf = float("nan"), float("inf")
    o = np.array([[nan, 0, 0], [0, inf, 0], [1, 1, 1], [1, 1, 1], [1, 1, 1], [1, 1, 1]], np.float32)
    d = np.array([[1, 0, 0], [1, 0, 0], [0, 0, -inf], [nan, 1, 0], [0, 0, 0], [-0.0, 0.0, -0.0]], np.float32)
    return o, d
