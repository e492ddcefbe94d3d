"""TSDF fusion of range images of a MOVING sensor through ``csrc/liblrt_sweepfuse.so``: ``mesh.integrate`` with every voxel centre projected under
the sweep model, so that the grid of a driving sequence is not sheared by the sensor's motion within a sweep.

    integrate_sweep(grid, depth, mask, sensor2world, inclination, twist, data_type="KITTI", sensor2ego=None, intensity=None, min_depth=0.0,
                    max_depth=80.0, tau=None, t_ref=0.5, direction="cw", workspace=None)
    twin = integrate_sweep_reference(...)        # the float64 numpy twin: namespace(margin, range_margin, unseen, fused, evals)
    pts = sweep_points(depth, sensor2world, twist, inclination, ...)          # (F, H, W, 3) float64 world points o + d depth of the sweep grid

``include/lrt_sweepfuse.h`` states the rule and ``csrc/lrt_sweepfuse_math.h`` is its text for the device and the host.

* The grid, the images, the poses and the inclination are ``mesh.integrate``'s, checked by ``mesh._frames`` as it is.  ``sensor2world[f]`` is the
  sensor's pose at the frame's REFERENCE instant (``tau == 0``).
* ``twist``: ``(6,)``, ``(F, 6)`` float64 HOST data ``(rho, phi)`` -- the sensor's motion over one sweep in the sensor frame, the convention of
  ``sweep.sweep_rays`` and ``project_points_sweep`` -- or ``None`` for a static sensor.  A tensor on a HIP device is refused: reading it would be
  a host wait.  ``tau``: ``(W,)`` float64 host data, or ``None`` for ``sweep.column_times(W, t_ref, direction)``.  Both are checked by
  ``sweep_project._motion``.
* Per voxel and frame: the centre goes to the sensor frame of the reference instant, ``project_points_sweep``'s search finds the column that, at
  its own instant, has the centre inside its azimuth bin, and the range is measured from THAT column's origin; the update is ``mesh.integrate``'s,
  operation for operation.  A centre that no column sees (``unseen``) is skipped for the frame, like one out of view or out of range.
* With ``twist=None`` or zeros (also for single frames) the result equals ``mesh.integrate``'s bit for bit.
* A HIP grid goes through the library: two launches (the column table, the voxels), none for ``F == 0``.  A missing library is a ``MeshError``, not
  a quiet fall-back.  A CPU grid goes to the twin, which calls ``project_points_sweep_reference`` as it is on the voxel centres and is equal to the
  device bit for bit while ``margin >= 1e-9`` and ``range_margin >= 1e-13`` (``sweep_project``'s two conditions on the inputs).
"""
from __future__ import annotations

import ctypes as C
import math
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import mesh, range_image as ri, sweep, sweep_project as sp
from .mesh import MeshError

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LRT_SWEEPFUSE_LIB") or os.path.join(HERE, "csrc", "liblrt_sweepfuse.so")
EXPORTS = ("lrt_sweepfuse_abi_version", "lrt_sweepfuse_last_error", "lrt_sweepfuse_work_bytes", "lrt_sweepfuse_integrate")     # include/lrt_sweepfuse.h
ABI_VERSION = 1
BLOCK = 256                                                                  # LRT_SWEEPFUSE_BLOCK
MAX_EVAL = 8                                                                 # LRT_SWEEPFUSE_MAX_EVAL
TABLE = 12                                                                   # LRT_SWEEPFUSE_TABLE
MAX_FRAMES = 65536                                                           # LRT_SWEEPFUSE_MAX_FRAMES

_lib = None


def load():
    """Load liblrt_sweepfuse.so (after torch, so that both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MeshError(f"{LIB_PATH} is missing: build it with `python -m lidar_rt_amd.build` (hipcc --offload-arch=gfx950). "
                        "integrate_sweep has no fall-back on a HIP device.")
    lib = C.CDLL(LIB_PATH)
    vp, ci, ll, d = C.c_void_p, C.c_int, C.c_longlong, C.c_double
    lib.lrt_sweepfuse_abi_version.restype = ci
    lib.lrt_sweepfuse_last_error.restype = C.c_char_p
    lib.lrt_sweepfuse_work_bytes.restype = ll
    lib.lrt_sweepfuse_work_bytes.argtypes = [ll, ci]
    lib.lrt_sweepfuse_integrate.restype = ci
    lib.lrt_sweepfuse_integrate.argtypes = [ci, ci, ci, ci, d, d, vp, vp, vp, ll, vp, ci, ci, vp, vp, vp, vp, ci, d, d, d, d, vp, vp, vp, ll, vp]
    if lib.lrt_sweepfuse_abi_version() != ABI_VERSION:
        raise MeshError("liblrt_sweepfuse.so ABI version mismatch; rebuild with `python -m lidar_rt_amd.build --force`")
    _lib = lib
    return lib


def work_bytes(F: int, W: int) -> int:
    """Bytes of the workspace of one call: the column table."""
    n = int(load().lrt_sweepfuse_work_bytes(int(F), int(W)))
    if n < 0:
        raise MeshError(f"integrate_sweep: {F} frames of {W} columns (at most {MAX_FRAMES} frames, at least 1 column)")
    return n


def _motion(twist, tau, F, W, t_ref, direction):
    """``sweep_project._motion``'s checks, as they are: (xi (F, 6) float64 or None, tau (W,) float64)."""
    try:
        return sp._motion(twist, tau, F, W, t_ref, direction)
    except ri.ProjectionError as e:
        raise MeshError(str(e).replace("project_points_sweep:", "integrate_sweep:").replace("project_points:", "integrate_sweep:")) from None


# ---- the twin -----------------------------------------------------------------------------------------------------------------------------------------------

@torch.no_grad()
def integrate_sweep_reference(grid, depth, mask, sensor2world, inclination, twist, data_type="KITTI", sensor2ego=None, intensity=None, min_depth=0.0,
                              max_depth=80.0, tau=None, t_ref=0.5, direction="cw"):
    """The numpy twin of ``integrate_sweep`` on a grid of CPU tensors, updated in place.  Returns namespace(margin, range_margin: the smallest of
    ``project_points_sweep_reference``'s over the frames of the call; unseen: the voxel-frames whose search did not converge; fused: the
    voxel-frames that took part; evals (MAX_EVAL + 1,) int64: the voxel-frames by the evaluations their search used)."""
    if not isinstance(grid, mesh.TsdfGrid) or grid.device.type != "cpu":
        raise MeshError("integrate_sweep_reference: the twin works on a TsdfGrid of CPU tensors")
    depth, mask, intensity, T, inc, off, yaw, min_depth, max_depth = mesh._frames(grid, depth, mask, sensor2world, inclination, data_type, sensor2ego,
                                                                                  intensity, min_depth, max_depth)
    F, H, W = depth.shape
    xi, tau = _motion(twist, tau, F, W, t_ref, direction)
    X, Y, Z = grid.dims
    cx, cy, cz = mesh.centres(grid.voxel, X), mesh.centres(grid.voxel, Y), mesh.centres(grid.voxel, Z)
    cen = np.stack(np.meshgrid(cx, cy, cz, indexing="ij"), -1).reshape(-1, 3)
    D = grid.tsdf.numpy().reshape(-1).astype(np.float64)
    Wt = grid.weight.numpy().reshape(-1).astype(np.float64)
    I = grid.intensity.numpy().reshape(-1).astype(np.float64) if intensity is not None else None
    seen = np.zeros(D.shape, bool)
    out = SimpleNamespace(margin=math.inf, range_margin=math.inf, unseen=0, fused=0, evals=np.zeros(MAX_EVAL + 1, np.int64))
    trunc = float(grid.trunc)
    for f in range(F):
        r = sp.project_points_sweep_reference(cen, H, W, inc, None if xi is None else xi[f], None, data_type, sensor2ego, T[f], tau, t_ref, direction,
                                              max_depth, min_depth, True)
        pix, r32, drop = r.pixel.numpy(), r.range_bits.view(np.float32), r.drop.numpy()
        out.margin, out.range_margin = min(out.margin, r.margin), min(out.range_margin, r.range_margin)
        out.unseen += int((drop == sp.UNSEEN).sum())
        out.evals += np.bincount(r.evals.numpy(), minlength=MAX_EVAL + 1)
        kept = np.nonzero(drop == ri.KEEP)[0]
        p = pix[kept, 1].astype(np.int64) * W + pix[kept, 0]
        dimg = depth[f].numpy().reshape(-1)[p]
        ok = (mask[f].numpy().reshape(-1)[p] != 0) & (dimg > 0)
        sdf = dimg.astype(np.float64) - r32[kept].astype(np.float64)
        ok &= ~(sdf < -trunc)
        v, sdf, p = kept[ok], sdf[ok], p[ok]
        s = sdf / trunc
        d = np.where(s < 1.0, s, 1.0)
        wt = Wt[v]
        D[v] = (wt * D[v] + d) / (wt + 1.0)
        if I is not None:
            I[v] = (wt * I[v] + intensity[f].numpy().reshape(-1)[p].astype(np.float64)) / (wt + 1.0)
        Wt[v] = wt + 1.0
        seen[v] = True
        out.fused += int(v.size)
    ts, we = grid.tsdf.numpy().reshape(-1), grid.weight.numpy().reshape(-1)
    ts[seen] = D[seen].astype(np.float32)
    we[seen] = Wt[seen].astype(np.int32)
    if I is not None:
        grid.intensity.numpy().reshape(-1)[seen] = I[seen].astype(np.float32)
    return out


# ---- the operator -------------------------------------------------------------------------------------------------------------------------------------------

@torch.no_grad()
def integrate_sweep(grid, depth, mask, sensor2world, inclination, twist, data_type="KITTI", sensor2ego=None, intensity=None, min_depth=0.0,
                    max_depth=80.0, tau=None, t_ref=0.5, direction="cw", workspace=None):
    """Fuse F posed range images of a moving sensor into ``grid`` in place (see the module text).  Two launches on a HIP device (none for F == 0),
    no host wait; None is returned.  A CPU grid goes to ``integrate_sweep_reference`` and its namespace is returned.  ``workspace``: a uint8 tensor
    on the grid's device of at least ``work_bytes(F, W)`` bytes to use instead of a fresh one; its contents do not matter."""
    if isinstance(grid, mesh.TsdfGrid) and grid.device.type != "cuda":
        if workspace is not None:
            raise MeshError("integrate_sweep: a workspace with a grid on the CPU")
        return integrate_sweep_reference(grid, depth, mask, sensor2world, inclination, twist, data_type, sensor2ego, intensity, min_depth, max_depth,
                                         tau, t_ref, direction)
    depth, mask, intensity, T, inc, off, yaw, min_depth, max_depth = mesh._frames(grid, depth, mask, sensor2world, inclination, data_type, sensor2ego,
                                                                                  intensity, min_depth, max_depth)
    F, H, W = depth.shape
    xi, tau_arr = _motion(twist, tau, F, W, t_ref, direction)
    lib = load()
    dev = grid.device
    X, Y, Z = grid.dims
    for name in ("tsdf", "weight") + (("intensity",) if grid.intensity is not None else ()):
        if not getattr(grid, name).is_contiguous():
            raise MeshError(f"integrate_sweep: the grid's {name} must be contiguous")
    nbytes = work_bytes(F, W)
    if workspace is not None:
        if not (torch.is_tensor(workspace) and workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.device == dev
                and workspace.numel() >= nbytes and workspace.data_ptr() % 256 == 0):
            raise MeshError(f"integrate_sweep: the workspace must be a contiguous uint8 tensor of at least {nbytes} bytes on {dev}, 256-byte aligned")
    if F == 0:
        return None                                                            # nothing to fuse: no launch
    ws = workspace if workspace is not None else torch.empty(nbytes, dtype=torch.uint8, device=dev)    # the caching allocator's blocks are 512-byte aligned
    d_T, d_inc = mesh._upload(T, dev), mesh._upload(inc, dev)
    d_xi = None if xi is None else mesh._upload(xi, dev)
    d_tau = None if xi is None else mesh._upload(tau_arr, dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        rc = lib.lrt_sweepfuse_integrate(dev.index, X, Y, Z, grid.voxel, grid.trunc, grid.tsdf.data_ptr(), grid.weight.data_ptr(), ptr(grid.intensity), F,
                                         d_T.data_ptr(), H, W, depth.data_ptr(), mask.data_ptr(), ptr(intensity), d_inc.data_ptr(), int(inc.size), off, yaw,
                                         min_depth, max_depth, ptr(d_xi), ptr(d_tau), ws.data_ptr(), ws.numel(),
                                         C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise MeshError(f"lrt_sweepfuse_integrate failed ({rc}): {lib.lrt_sweepfuse_last_error().decode()}")
    return None


# ---- the points of a sweep scan -----------------------------------------------------------------------------------------------------------------------------

@torch.no_grad()
def sweep_points(depth, sensor2world, twist, inclination, data_type="KITTI", sensor2ego=None, tau=None, t_ref=0.5, direction="cw"):
    """The world points ``o + d depth`` of F frames on their ``sweep.sweep_rays_reference`` grid, on the host in float64: (F, H, W, 3), or (H, W, 3)
    for an (H, W) depth.  ``sensor2world`` (F, 4, 4) or (4, 4) and ``twist`` (F, 6), (6,) or None are host data."""
    dep = depth.detach().cpu().numpy() if torch.is_tensor(depth) else np.asarray(depth)
    if dep.ndim not in (2, 3):
        raise MeshError(f"sweep_points: depth must be (H, W) or (F, H, W) (it is {tuple(dep.shape)})")
    batched = dep.ndim == 3
    dep = (dep if batched else dep[None]).astype(np.float64)
    F, H, W = dep.shape
    S = np.asarray(sensor2world.detach().cpu().numpy() if torch.is_tensor(sensor2world) else sensor2world, np.float64).reshape(-1, 4, 4)
    if S.shape[0] != F:
        raise MeshError(f"sweep_points: {S.shape[0]} poses for {F} frames")
    xi, tau_arr = _motion(twist, tau, F, W, t_ref, direction)
    if F == 0:
        return np.zeros((0, H, W, 3))
    inc = ri._host_array("inclination", inclination, np.float64).reshape(-1)
    try:
        o, d = sweep.sweep_rays_reference(torch.from_numpy(np.ascontiguousarray(S[:, :3])), None if xi is None else torch.from_numpy(xi), H, W,
                                          inc.tolist(), data_type, None if sensor2ego is None else torch.as_tensor(np.asarray(sensor2ego, np.float32)),
                                          tau=torch.from_numpy(tau_arr))
    except sweep.SweepError as e:
        raise MeshError(f"sweep_points: {e}") from None
    pts = o.numpy() + d.numpy() * dep[..., None]
    return pts if batched else pts[0]
