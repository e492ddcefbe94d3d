"""Seeded cases of the TSDF fusion under the sweep model (lidar_rt_amd/sweep_fuse.py), shared by tests/test_sweep_fuse.py and
tests/test_sweep_fuse_gpu.py.

* The bit-exact cases: the grids, conventions, sizes and room images of tests/mesh_cases.py (unchanged) fused under the motions MOTIONS of
  tests/sweep_project_cases.py.  A case is the twin's grid and its report, computed once on the CPU and left unchanged.  Every builder asserts
  the twin's ``margin >= MARGIN`` and ``range_margin >= RANGE_MARGIN`` (the constants of sweep_project_cases): conditions on the inputs, never
  filters -- no voxel is left out of a comparison.  Every three-frame case has fused voxel-frames, every 17 x 19 x 23 one has unseen
  voxel-frames (the search that does not converge), and over the cases every evaluation count from 1 to 8 occurs (``all_evals``).
* The accuracy case: three frames of a sensor that MOVES through the analytic room while it turns (every pixel's range is measured along its own
  sweep ray), fused into a grid across the wall x = 9; the error of a mesh is the distance of its world vertices to the nearest plane.
* A room sequence with stored twists for the command lines.
"""
import functools
import math

import numpy as np
import torch

from lidar_rt_amd import mesh, sequence, sweep, sweep_fuse as sf
from tests import mesh_cases as mcs
from tests import registration_cases as rc
from tests import sweep_project_cases as spc

MARGIN, RANGE_MARGIN = spc.MARGIN, spc.RANGE_MARGIN
MOTIONS = ("moderate_cw", "moderate_ccw", "table", "strong_ccw", "closed")
GRIDS, CONVENTIONS, SIZES = tuple(mcs.GRIDS), mcs.CONVENTIONS, mcs.SIZES
WALL_GRID = dict(origin=(8.4013, -2.0027, -1.6031), voxel=0.1, dims=(11, 40, 16))


def motion(name, W, F=3):
    """dict(twist (F, 6) or (6,), tau, t_ref, direction) of a named motion for F of the three frames."""
    mo = dict(spc.motion(name, W, 3))
    tw = np.asarray(mo["twist"], np.float64)
    mo["twist"] = tw[:F] if tw.ndim == 2 else tw
    return mo


def fuse_kw(fr, mo, dev="cpu", intensity=True):
    """The arguments of integrate_sweep behind the grid: the frames of mesh_cases on `dev` and a motion."""
    return dict(mcs.frames_to(fr, dev, intensity), **mo)


@functools.lru_cache(maxsize=None)
def reference(dims, F, H, W, conv, mo_name, intensity=True, calls=1):
    """The twin's grid after `calls` integrate_sweep calls of F frames each (the second call with the frames of seed 1) and the reports."""
    g = mcs.room_grid(dims, intensity)
    reports = []
    for c in range(calls):
        r = sf.integrate_sweep_reference(g, **fuse_kw(mcs.room_frames(F, H, W, conv, c), motion(mo_name, W, F), "cpu", intensity))
        key = (dims, F, H, W, conv, mo_name, c)
        if F:
            assert r.margin >= MARGIN, (key, r.margin)
            assert r.range_margin >= RANGE_MARGIN, (key, r.range_margin)
        if F == 3:
            assert r.fused > 0, key
            assert r.unseen > 0 or dims != (17, 19, 23), key
        reports.append(r)
    return g, reports


def all_cases():
    return [(d, c, s, m) for d in GRIDS for c in CONVENTIONS for s in SIZES for m in MOTIONS]


@functools.lru_cache(maxsize=None)
def all_evals():
    """The histogram of the evaluations over the 90 three-frame cases."""
    h = np.zeros(sf.MAX_EVAL + 1, np.int64)
    for dims, conv, (H, W), mo in all_cases():
        h += reference(dims, 3, H, W, conv, mo)[1][0].evals
    assert np.all(h[1:] > 0), h
    return h


# ---- the accuracy case --------------------------------------------------------------------------------------------------------------------------------------

def ray_room_depth(o, d):
    """(H, W) float64: the nearest positive intersection of every ray o + t d (world, (H, W, 3) float64) with the eight planes of the room."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (rc.PLANES[:, 3][None, None, :] - o @ rc.PLANES[:, :3].T) / (d @ rc.PLANES[:, :3].T)
    return np.where(t > 0.0, t, np.inf).min(-1)


def moving_scan(poses, twists, H, W, conv, tau):
    """The frames a sensor records that moves by twists[f] over the sweep around poses[f]: every pixel's range along its own sweep ray.  No holes.
    twists None: a static sensor."""
    kw = mcs.convention(conv, H)
    s2e = None if kw["sensor2ego"] is None else torch.as_tensor(np.asarray(kw["sensor2ego"], np.float32))
    o, d = sweep.sweep_rays_reference(torch.from_numpy(np.ascontiguousarray(np.asarray(poses, np.float64)[:, :3])),
                                      None if twists is None else torch.from_numpy(np.asarray(twists, np.float64)), H, W, kw["inclination"],
                                      kw["data_type"], s2e, tau=torch.from_numpy(np.asarray(tau, np.float64)))
    depth = torch.from_numpy(np.stack([ray_room_depth(o[f].numpy(), d[f].numpy()) for f in range(len(poses))]).astype(np.float32))
    m = torch.isfinite(depth) & (depth > 0)
    return dict(depth=torch.where(m, depth, torch.zeros_like(depth)), mask=m, sensor2world=np.asarray(poses, np.float64), **kw)


def plane_distance(points):
    """(N,) the distance of world points to the nearest plane of the room."""
    return np.abs(points @ rc.PLANES[:, :3].T - rc.PLANES[:, 3][None]).min(1) if len(points) else np.zeros(0)


@functools.lru_cache(maxsize=None)
def accuracy(conv, H=16, W=128):
    """{name: (max, median)} of e_s (the static scan, integrate_reference), e_u (the moving scan, integrate_reference) and e_c (the moving scan,
    integrate_sweep_reference) on the wall grid."""
    poses = np.stack([rc.exp4(rc.twist(40 + f, 0.6 + 0.2 * f, 4.0 + f)) for f in range(3)])
    twists = np.array(spc.PER_FRAME, np.float64)
    tau = sweep.column_times(W, 0.0, "cw").numpy()
    static, moving = moving_scan(poses, None, H, W, conv, tau), moving_scan(poses, twists, H, W, conv, tau)
    out = {}
    for name, scan, fuse in (("e_s", static, None), ("e_u", moving, None), ("e_c", moving, twists)):
        g = mesh.TsdfGrid(WALL_GRID["origin"], WALL_GRID["voxel"], WALL_GRID["dims"], intensity=False)
        if fuse is None:
            mesh.integrate_reference(g, **scan)
        else:
            sf.integrate_sweep_reference(g, twist=fuse, tau=tau, **scan)
        e = plane_distance(mesh.extract_reference(g).world())
        assert e.size > 100, (name, e.size)
        out[name] = (float(e.max()), float(np.median(e)))
    return out


# ---- a sequence with stored twists --------------------------------------------------------------------------------------------------------------------------

SEQ_H, SEQ_W = 16, 128


def write_sweep_sequence(root, stored=True, tau=False):
    """Three frames of a sensor moving through the room (KITTI bounds), written through sequence.write_sequence with each frame's twist (and, with
    `tau`, its column times).  Poses and twists are rounded to float32 first, as the file stores them, so the scan is the one the file describes.
    stored=False: the same scan without twists."""
    H, W, inc = SEQ_H, SEQ_W, list(rc.BOUNDS)
    poses = np.stack([rc.exp4(rc.twist(60 + f, 0.5 + 0.3 * f, 3.0)) for f in range(3)]).astype(np.float32).astype(np.float64)
    twists = np.array(spc.PER_FRAME, np.float32).astype(np.float64)
    taus = np.stack([(spc.tau_table(W, 7 + f) if tau else sweep.column_times(W).numpy()).astype(np.float32).astype(np.float64) for f in range(3)])
    rng = np.random.default_rng(3)
    frames = []
    for f in range(3):
        scan = moving_scan(poses[f:f + 1], twists[f:f + 1], H, W, "kitti_bounds", taus[f])
        frames.append(dict(id=f, depth=scan["depth"][0], intensity=torch.from_numpy(rng.uniform(0, 1, (H, W)).astype(np.float32)), mask=scan["mask"][0],
                           inclination=inc, sensor2world=poses[f], **(dict(twist=twists[f], **({"tau": taus[f]} if tau else {})) if stored else {})))
    sequence.write_sequence(root, frames, "KITTI")
    return root


def check_sequence_margins(root, out_dir):
    """The conditions of the byte-for-byte comparison of the command line on two devices: the twin's two margins over every fused frame, on the
    grid the run chose (read from its mesh.json).  Returns the twin's mesh."""
    import json
    import os
    rep = json.load(open(os.path.join(out_dir, "mesh.json")))
    meta, frames, inc = mesh.load_frames(root, "train", False, "stored")
    gr = rep["grid"]
    g = mesh.TsdfGrid(gr["origin"], gr["voxel"], gr["dims"], gr["trunc"], "cpu", intensity=True)
    st = lambda k, dt: torch.from_numpy(np.stack([f[k] for f in frames]).astype(dt))
    r = sf.integrate_sweep_reference(g, st("depth", np.float32), st("mask", np.bool_), np.stack([f["sensor2world"] for f in frames]),
                                     (float(inc[0]), float(inc[1])), np.stack([f["twist"] for f in frames]), "KITTI", None, st("intensity", np.float32),
                                     0.0, 80.0, tau=frames[0]["tau"])
    assert r.margin >= MARGIN and r.range_margin >= RANGE_MARGIN, (r.margin, r.range_margin)
    return mesh.extract_reference(g), r, rep
