"""Scan-to-map registration: range images aligned directly to the fused TSDF grid of ``mesh.py`` (Bylow et al., RSS 2013), through
``csrc/liblrt_mapreg.so``.  ``registration.odometry`` aligns every scan to the scan before it, so its error adds up along the chain; here every
scan is aligned to everything fused so far and then fused itself -- tracking -- and any scan can be localised in a finished map.

    sums, cell = linearize_to_grid(grid, src, X, huber=0.1, min_weight=1)
    reg        = align_to_grid(grid, src, init, iters=20, huber=0.1, lam=1e-6, min_pairs=50, tol_t=1e-5, tol_r=1e-6, min_weight=1)
                                                           # MapRegistration: X, G (F, 3, 4) float64, log (F, K, 8), hessian (F, 6, 6), status (F)
    poses, report = track_and_fuse(grid, frames, images, first_pose=None, steps=None, inclination=..., ...)

``grid`` is a ``mesh.TsdfGrid``; ``src`` is a frame geometry ``(points (H, W, 3) float32, mask (H, W))`` or ``(points, normals, mask)`` of
``registration.frame_geometry`` (the normals are not read), or batched with a leading frame axis ``F``.  ``X`` is the pose of the source frame in
the GRID frame -- the world minus ``grid.origin`` (``grid_pose`` / ``world_pose`` convert) -- as float64 ``(3, 4)`` / ``(4, 4)`` or batched.
``include/lrt_mapreg.h`` states the rule: one trilinear sample of the grid per source pixel gives the residual ``e = trunc D`` and its gradient
``n = trunc g``; the Huber weight, the Jacobian of the right perturbation ``X <- X Exp(delta)``, the 30 sums, their order and the solve are
``registration``'s.  No correspondence search, no normals, no rendered view.  ``G = X^-1`` is what ``lrt_mesh_integrate`` takes as grid2sensor.

* HIP tensors go through the library: ``linearize_to_grid`` is two launches, ``align_to_grid`` ``2 K`` launches for ``K <= 32`` iterations and all
  ``F`` frames, with no host wait and no atomics.  A missing library is an error, not a quiet fall-back.  CPU tensors go to the float64 numpy
  twins ``linearize_to_grid_reference`` and ``align_to_grid_reference``, which also return ``margin``: the smallest distance [m] of any sample
  from a decision boundary of the rule (the domain's faces, a cell's faces, the Huber threshold), as ``mesh.integrate_reference`` does.
* ``status`` per frame: 0 ok, 1 fewer than ``min_pairs`` terms, 2 a pivot that is not positive, 3 converged.  From the first non-zero status on
  ``X`` keeps its bits.  The basin is the truncation band: a start further than ``trunc`` from the surface samples free space and has no term.
* THE IMAGE MUST BE FINE ENOUGH FOR THE MAP.  The grid is fused projectively, so a voxel between two beams takes the range of the nearest
  pixel.  Measured on the analytic room (12 frames, 0.35 m and 1.5 degrees per step, voxel 0.2 m, trunc 0.8 m): at 32 x 256 map tracking stays
  at a few millimetres while the odometry chain drifts to centimetres; at 16 x 128 the image is too coarse, map tracking is WORSE than the chain
  for about the first ten frames (profiles/map_registration.md has the figures).
* ``track_and_fuse`` handles ``frames`` ({id: geometry}) in id order: frame k starts from ``est[k - 1] @ step[k]`` (``steps`` {id: (4, 4)}: the
  chain's relative pose ``T_{k-1}^-1 T_k``; without them the last step found -- constant velocity), is aligned to the grid, and its image
  (``images`` {id: (depth, mask[, intensity])}) is fused at the pose found with ``G`` handed to ``lrt_mesh_integrate`` on the device (the twin on
  the CPU).  The lowest id is fused at ``first_pose`` without an alignment when the grid is given empty (``fuse_first``).  A frame whose status
  is 1 or 2 keeps its start pose and is fused there.  The host reads once, at the end.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import mesh, registration as rg

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LRT_MAPREG_LIB") or os.path.join(HERE, "csrc", "liblrt_mapreg.so")
EXPORTS = ("lrt_mapreg_abi_version", "lrt_mapreg_last_error", "lrt_mapreg_work_bytes", "lrt_mapreg_linearize", "lrt_mapreg_align")   # include/lrt_mapreg.h
ABI_VERSION = 1
BLOCK = 256                                                                  # LRT_MAPREG_BLOCK
NSUM = 30                                                                    # LRT_MAPREG_NSUM
NLOG = 8                                                                     # LRT_MAPREG_NLOG
MAX_ITER, MAX_FRAMES = 32, 65535
MAX_PIXELS = (2 ** 31 - 1) // 3                                              # LRT_MAPREG_MAX_PIXELS
OK, FEW, PIVOT, CONVERGED = rg.OK, rg.FEW, rg.PIVOT, rg.CONVERGED
DEFAULT_ITERS = 20

_lib = None


class MapRegistrationError(RuntimeError):
    pass


class MapRegistration(SimpleNamespace):
    """X, G (F, 3, 4) float64, log (F, K, 8) float64, hessian (F, 6, 6) float64, status (F) int32 (the twin adds margin); without a frame axis in
    the inputs, without one here."""

    def __iter__(self):
        return iter((self.X, self.G, self.log, self.hessian, self.status))


def load():
    """Load liblrt_mapreg.so (after torch, so that both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MapRegistrationError(f"{LIB_PATH} is missing: build it with `python -m lidar_rt_amd.build` (hipcc --offload-arch=gfx950). "
                                   "map_registration has no fall-back on a HIP device.")
    lib = C.CDLL(LIB_PATH)
    vp, ci, ll, d = C.c_void_p, C.c_int, C.c_longlong, C.c_double
    lib.lrt_mapreg_abi_version.restype = ci
    lib.lrt_mapreg_last_error.restype = C.c_char_p
    lib.lrt_mapreg_work_bytes.restype = ll
    lib.lrt_mapreg_work_bytes.argtypes = [ll, ci, ci]
    common = [ci, ci, ci, ci, d, d, vp, vp, ci, ll, ci, ci, vp, vp]
    lib.lrt_mapreg_linearize.restype = ci
    lib.lrt_mapreg_linearize.argtypes = common + [vp, d, vp, vp, vp, ll, vp]
    lib.lrt_mapreg_align.restype = ci
    lib.lrt_mapreg_align.argtypes = common + [vp, ci, d, d, ll, d, d, vp, vp, vp, vp, vp, vp, ll, vp]
    if lib.lrt_mapreg_abi_version() != ABI_VERSION:
        raise MapRegistrationError("liblrt_mapreg.so ABI version mismatch; rebuild with `python -m lidar_rt_amd.build --force`")
    _lib = lib
    return lib


# ---- the arguments ------------------------------------------------------------------------------------------------------------------------------------------

def grid_pose(grid, sensor2world):
    """(..., 4, 4) float64 numpy: world poses in the grid frame, the translation minus ``grid.origin``."""
    T = np.array(sensor2world.detach().cpu().numpy() if torch.is_tensor(sensor2world) else sensor2world, np.float64)
    T[..., :3, 3] = T[..., :3, 3] - np.asarray(grid.origin, np.float64)
    return T


def world_pose(grid, X):
    """(..., 4, 4) float64 numpy: grid-frame poses (..., 3, 4) or (..., 4, 4) in the world."""
    X = np.asarray(X.detach().cpu().numpy() if torch.is_tensor(X) else X, np.float64)
    T = np.zeros(X.shape[:-2] + (4, 4))
    T[..., 3, 3] = 1.0
    T[..., :3, :] = X[..., :3, :]
    T[..., :3, 3] = T[..., :3, 3] + np.asarray(grid.origin, np.float64)
    return T


def _arguments(fn, grid, src, min_weight):
    if not isinstance(grid, mesh.TsdfGrid):
        raise MapRegistrationError(f"{fn}: grid must be a mesh.TsdfGrid")
    try:
        sp, _, sm, batched = rg._geometry("src", src, False)
    except rg.RegistrationError as e:
        raise MapRegistrationError(str(e).replace("registration:", fn + ":")) from None
    if sp.device != grid.device:
        raise MapRegistrationError(f"{fn}: the grid is on {grid.device}, src on {sp.device}")
    F, H, W = (int(x) for x in sp.shape[:3])
    if F < 1 or F > MAX_FRAMES or H < 1 or W < 1 or F * H * W > MAX_PIXELS:
        raise MapRegistrationError(f"{fn}: {F} frames of {H} x {W} pixels (each at least 1, at most {MAX_FRAMES} frames, F H W at most {MAX_PIXELS})")
    mw = int(min_weight)
    if mw < 1:
        raise MapRegistrationError(f"{fn}: min_weight {mw} (at least 1: weight 0 is unobserved)")
    for name in ("tsdf", "weight"):
        if not getattr(grid, name).is_contiguous():
            raise MapRegistrationError(f"{fn}: the grid's {name} must be contiguous")
    return sp, sm, batched, F, H, W, mw


def _poses(fn, name, X, F, batched, dev):
    try:
        return rg._poses(name, X, F, batched, dev)
    except rg.RegistrationError as e:
        raise MapRegistrationError(str(e).replace("registration:", fn + ":")) from None


def _solver(fn, iters, huber, lam, min_pairs, tol_t, tol_r):
    try:
        huber, lam, min_pairs, tol_t, tol_r = rg._solver(huber, lam, min_pairs, tol_t, tol_r)
    except rg.RegistrationError as e:
        raise MapRegistrationError(str(e).replace("registration:", fn + ":")) from None
    K = int(iters)
    if K != iters or not 1 <= K <= MAX_ITER:
        raise MapRegistrationError(f"{fn}: {iters} iterations (1 to {MAX_ITER})")
    return K, huber, lam, min_pairs, tol_t, tol_r


# ---- the twin -----------------------------------------------------------------------------------------------------------------------------------------------

def _lerp(a, b, f):
    return a + f * (b - a)


def sample_reference(ts, wt, voxel, min_weight, q):
    """mr_sample on (N, 3) float64 points of the grid frame: (cell (N,) int64, -1 without a term; D (N,); g (N, 3); margin [m]).  ``ts`` (X, Y, Z)
    float32 and ``wt`` int32 numpy arrays."""
    dims = ts.shape
    N = q.shape[0]
    cell = np.full(N, -1, np.int64)
    D, g = np.zeros(N), np.zeros((N, 3))
    margin = math.inf
    if min(dims) < 2 or N == 0:
        return cell, D, g, margin
    voxel = float(voxel)
    with np.errstate(all="ignore"):
        ok = np.isfinite(q).all(1)
        idx, f, h = np.zeros((N, 3), np.int64), np.zeros((N, 3)), np.zeros((N, 3))
        cen = [mesh.centres(voxel, n).astype(np.float64) for n in dims]
        for a in range(3):
            c, n = cen[a], dims[a]
            inside = (c[0] <= q[:, a]) & (q[:, a] <= c[n - 1])
            if ok.any():
                margin = min(margin, float(np.minimum(np.abs(q[ok, a] - c[0]), np.abs(q[ok, a] - c[n - 1])).min()))
            ok &= inside
        for a in range(3):
            c, n = cen[a], dims[a]
            u = np.where(ok, q[:, a], c[0]) / voxel - 0.5
            fi = np.floor(u)
            idx[:, a] = np.where(fi > 0.0, np.minimum(fi, float(n - 2)), 0.0).astype(np.int64)
            if ok.any() and n > 2:                                           # the faces between two cells: the whole numbers 1 .. n - 2 of u
                k = np.clip(np.rint(u[ok]), 1.0, float(n - 2))
                margin = min(margin, float(np.abs(u[ok] - k).min()) * voxel)
            ca, cb = c[idx[:, a]], c[idx[:, a] + 1]
            h[:, a] = cb - ca
            f[:, a] = np.clip((np.where(ok, q[:, a], ca) - ca) / h[:, a], 0.0, 1.0)
        v, known, ones = [], ok.copy(), np.ones(N, bool)
        for n in range(8):
            i, j, k = idx[:, 0] + (n & 1), idx[:, 1] + (n >> 1 & 1), idx[:, 2] + (n >> 2 & 1)
            t = ts[i, j, k]
            known &= wt[i, j, k] >= min_weight
            ones &= t == np.float32(1.0)
            v.append(t.astype(np.float64))
        fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
        c00, c10, c01, c11 = _lerp(v[0], v[1], fx), _lerp(v[2], v[3], fx), _lerp(v[4], v[5], fx), _lerp(v[6], v[7], fx)
        c0, c1 = _lerp(c00, c10, fy), _lerp(c01, c11, fy)
        D = _lerp(c0, c1, fz)
        g = np.stack([_lerp(_lerp(v[1] - v[0], v[3] - v[2], fy), _lerp(v[5] - v[4], v[7] - v[6], fy), fz) / h[:, 0],
                      _lerp(c10 - c00, c11 - c01, fz) / h[:, 1], (c1 - c0) / h[:, 2]], 1)
        has = known & ~ones & (g != 0.0).any(1)
    cell[has] = ((idx[has, 0] * dims[1] + idx[has, 1]) * dims[2] + idx[has, 2])
    return cell, np.where(has, D, 0.0), np.where(has[:, None], g, 0.0), margin


def pixels_reference(ts, wt, voxel, trunc, min_weight, X, sp, sm, huber):
    """mr_pixel on one frame, numpy: namespace(cell (H W,) int32, e (H W,), n (H W, 3), terms (H W, 30) -- zero rows without a term --, margin)."""
    HW = sm.size
    sp, sm = sp.reshape(HW, 3), sm.reshape(HW) != 0
    idx = np.nonzero(sm)[0]
    p = sp[idx].astype(np.float64)
    with np.errstate(all="ignore"):
        q = np.stack([X[k, 0] * p[:, 0] + X[k, 1] * p[:, 1] + X[k, 2] * p[:, 2] + X[k, 3] for k in range(3)], 1) if idx.size else np.zeros((0, 3))
    c, D, g, margin = sample_reference(ts, wt, voxel, min_weight, q)
    has = c >= 0
    cell = np.full(HW, -1, np.int32)
    cell[idx[has]] = c[has].astype(np.int32)
    e_all, n_all, terms = np.zeros(HW), np.zeros((HW, 3)), np.zeros((HW, NSUM))
    e = float(trunc) * D[has]
    n = float(trunc) * g[has]
    ph = p[has]
    m = [X[0, j] * n[:, 0] + X[1, j] * n[:, 1] + X[2, j] * n[:, 2] for j in range(3)]
    J = np.stack(m + [ph[:, 1] * m[2] - ph[:, 2] * m[1], ph[:, 2] * m[0] - ph[:, 0] * m[2], ph[:, 0] * m[1] - ph[:, 1] * m[0]], 1)
    ae = np.abs(e)
    with np.errstate(all="ignore"):
        w = np.where(ae <= huber, 1.0, huber / ae)
    if ae.size:
        margin = min(margin, float(np.abs(ae - huber).min()))
    t = np.empty((e.size, NSUM))
    k = 0
    for i in range(6):
        wj = w * J[:, i]
        for j in range(i, 6):
            t[:, k] = wj * J[:, j]
            k += 1
    for i in range(6):
        t[:, 21 + i] = (w * J[:, i]) * e
    t[:, 27] = (w * e) * e
    t[:, 28] = w
    t[:, 29] = 1.0
    sel = idx[has]
    e_all[sel], n_all[sel], terms[sel] = e, n, t
    return SimpleNamespace(cell=cell, e=e_all, n=n_all, terms=terms, margin=margin)


def inverse_reference(X):
    """mr_inverse: G (3, 4) = X^-1 of a rigid X (3, 4), R^T and -(R^T t) with the rows summed left to right."""
    G = np.empty((3, 4))
    G[:, :3] = X[:, :3].T
    for i in range(3):
        G[i, 3] = -(X[0, i] * X[0, 3] + X[1, i] * X[1, 3] + X[2, i] * X[2, 3])
    return G


def _np(t):
    return t.detach().cpu().numpy()


def _grid_np(grid):
    X, Y, Z = grid.dims
    return _np(grid.tsdf).reshape(X, Y, Z), _np(grid.weight).reshape(X, Y, Z)


@torch.no_grad()
def linearize_to_grid_reference(grid, src, X, huber=0.1, min_weight=1, return_abs=False):
    """The float64 numpy twin of ``linearize_to_grid``: (sums (F, 30) float64, cell (F, H, W) int32, margin) as CPU tensors and a float;
    ``return_abs=True`` adds the sums of the terms' magnitudes (F, 30), the scale of the summation bound, before the margin."""
    fn = "linearize_to_grid"
    sp, sm, batched, F, H, W, mw = _arguments(fn, grid, src, min_weight)
    huber = _solver(fn, 1, huber, 0.0, 1, 0.0, 0.0)[1]
    Xn = _np(_poses(fn, "X", X, F, batched, X.device if torch.is_tensor(X) else torch.device("cpu")))
    ts, wt = _grid_np(grid)
    sp, sm = _np(sp), _np(sm)
    out = [pixels_reference(ts, wt, grid.voxel, grid.trunc, mw, Xn[f], sp[f], sm[f], huber) for f in range(F)]
    sums = torch.from_numpy(np.stack([o.terms.sum(0) for o in out]))
    ab = torch.from_numpy(np.stack([np.abs(o.terms).sum(0) for o in out]))
    cell = torch.from_numpy(np.stack([o.cell for o in out]).reshape(F, H, W))
    margin = min(o.margin for o in out)
    sums, cell, ab = rg._sq(batched, sums, cell, ab)
    return (sums, cell, ab, margin) if return_abs else (sums, cell, margin)


@torch.no_grad()
def align_to_grid_reference(grid, src, init=None, iters=DEFAULT_ITERS, huber=0.1, lam=1e-6, min_pairs=50, tol_t=1e-5, tol_r=1e-6,
                            min_weight=1) -> MapRegistration:
    """The float64 numpy twin of ``align_to_grid`` (see the module text); the results are CPU tensors, ``margin`` the smallest over all iterations."""
    fn = "align_to_grid"
    sp, sm, batched, F, H, W, mw = _arguments(fn, grid, src, min_weight)
    K, huber, lam, min_pairs, tol_t, tol_r = _solver(fn, iters, huber, lam, min_pairs, tol_t, tol_r)
    X = _np(_poses(fn, "init", init, F, batched, init.device if torch.is_tensor(init) else torch.device("cpu"))).copy()
    ts, wt = _grid_np(grid)
    sp, sm = _np(sp), _np(sm)
    log, hess, status, G = np.zeros((F, K, NLOG)), np.zeros((F, 6, 6)), np.zeros(F, np.int32), np.zeros((F, 3, 4))
    margin = math.inf
    for f in range(F):
        st = OK
        for it in range(K):
            o = pixels_reference(ts, wt, grid.voxel, grid.trunc, mw, X[f], sp[f], sm[f], huber)
            margin = min(margin, o.margin)
            s = o.terms.sum(0)
            nr = nf = 0.0
            if st == OK:
                st, X[f], nr, nf = rg.solve_reference(s, lam, float(min_pairs), tol_t, tol_r, X[f])
            log[f, it] = (s[29], s[27], s[28], nr, nf, float(st), 0.0, 0.0)
        hess[f], status[f], G[f] = rg._hessian(s), st, inverse_reference(X[f])
    X, G, log, hess, status = rg._sq(batched, *(torch.from_numpy(a) for a in (X, G, log, hess, status)))
    return MapRegistration(X=X, G=G, log=log, hessian=hess, status=status, margin=margin)


# ---- the operators ------------------------------------------------------------------------------------------------------------------------------------------

def work_bytes(F: int, H: int, W: int) -> int:
    """Bytes of the workspace of one call: the workgroups' partial rows and the running status."""
    n = int(load().lrt_mapreg_work_bytes(int(F), int(H), int(W)))
    if n < 0:
        raise MapRegistrationError(f"map_registration: {F} frames of {H} x {W} pixels (each at least 1, at most {MAX_FRAMES} frames, F H W at most {MAX_PIXELS})")
    return n


def _workspace(workspace, nbytes, dev):
    if workspace is None:
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)              # the caching allocator's blocks are 512-byte aligned
    if not (torch.is_tensor(workspace) and workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.device == dev
            and workspace.numel() >= nbytes and workspace.data_ptr() % 256 == 0):
        raise MapRegistrationError(f"lrt_mapreg: the workspace must be a contiguous uint8 tensor of at least {nbytes} bytes on {dev}, 256-byte aligned")
    return workspace


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _grid_args(grid, mw, F, H, W, sp, sm):
    X, Y, Z = grid.dims
    return (grid.device.index, X, Y, Z, grid.voxel, grid.trunc, grid.tsdf.data_ptr(), grid.weight.data_ptr(), mw, F, H, W, sp.data_ptr(), sm.data_ptr())


@torch.no_grad()
def linearize_to_grid(grid, src, X, huber=0.1, min_weight=1, want_cell=True, workspace=None):
    """(sums (F, 30) float64, cell (F, H, W) int32 or None) of F frames at X (see the module text).  CPU tensors go to the twin."""
    fn = "linearize_to_grid"
    sp, sm, batched, F, H, W, mw = _arguments(fn, grid, src, min_weight)
    dev = sp.device
    if dev.type != "cuda":
        if workspace is not None:
            raise MapRegistrationError(f"{fn}: a workspace with tensors on {dev}")
        sums, cell, _ = linearize_to_grid_reference(grid, src, X, huber, min_weight)
        return sums, (cell if want_cell else None)
    lib = load()
    huber = _solver(fn, 1, huber, 0.0, 1, 0.0, 0.0)[1]
    Xd = _poses(fn, "X", X, F, batched, dev)
    ws = _workspace(workspace, work_bytes(F, H, W), dev)
    sums = torch.empty((F, NSUM), dtype=torch.float64, device=dev)
    cell = torch.empty((F, H, W), dtype=torch.int32, device=dev) if want_cell else None
    with torch.cuda.device(dev):
        rc = lib.lrt_mapreg_linearize(*_grid_args(grid, mw, F, H, W, sp, sm), Xd.data_ptr(), huber, sums.data_ptr(), None if cell is None else cell.data_ptr(),
                                      ws.data_ptr(), ws.numel(), _stream(dev))
    if rc != 0:
        raise MapRegistrationError(f"lrt_mapreg_linearize failed ({rc}): {lib.lrt_mapreg_last_error().decode()}")
    if not batched:
        sums, cell = sums[0], (None if cell is None else cell[0])
    return sums, cell


@torch.no_grad()
def align_to_grid(grid, src, init=None, iters=DEFAULT_ITERS, huber=0.1, lam=1e-6, min_pairs=50, tol_t=1e-5, tol_r=1e-6, min_weight=1,
                  workspace=None) -> MapRegistration:
    """Align F source frames to the grid (see the module text).  ``init``: X to start from, float64 on the grid's device (the ``X`` of an earlier call
    is used as it is, without a host read); ``None`` is the identity.  CPU tensors go to the twin."""
    fn = "align_to_grid"
    sp, sm, batched, F, H, W, mw = _arguments(fn, grid, src, min_weight)
    dev = sp.device
    if dev.type != "cuda":
        if workspace is not None:
            raise MapRegistrationError(f"{fn}: a workspace with tensors on {dev}")
        return align_to_grid_reference(grid, src, init, iters, huber, lam, min_pairs, tol_t, tol_r, min_weight)
    lib = load()
    K, huber, lam, min_pairs, tol_t, tol_r = _solver(fn, iters, huber, lam, min_pairs, tol_t, tol_r)
    X0 = _poses(fn, "init", init, F, batched, dev)
    ws = _workspace(workspace, work_bytes(F, H, W), dev)
    X = torch.empty((F, 3, 4), dtype=torch.float64, device=dev)
    G = torch.empty((F, 3, 4), dtype=torch.float64, device=dev)
    log = torch.empty((F, K, NLOG), dtype=torch.float64, device=dev)
    hess = torch.empty((F, 6, 6), dtype=torch.float64, device=dev)
    status = torch.empty((F,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.lrt_mapreg_align(*_grid_args(grid, mw, F, H, W, sp, sm), X0.data_ptr(), K, huber, lam, min_pairs, tol_t, tol_r, X.data_ptr(), G.data_ptr(),
                                  log.data_ptr(), hess.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev))
    if rc != 0:
        raise MapRegistrationError(f"lrt_mapreg_align failed ({rc}): {lib.lrt_mapreg_last_error().decode()}")
    X, G, log, hess, status = rg._sq(batched, X, G, log, hess, status)
    return MapRegistration(X=X, G=G, log=log, hessian=hess, status=status)


# ---- tracking -----------------------------------------------------------------------------------------------------------------------------------------------

def _fuse(grid, image, G, inclination, data_type, sensor2ego, min_depth, max_depth):
    """One frame into the grid at grid2sensor G (3, 4) float64 on the grid's device: lrt_mesh_integrate with G as it lies on the device, the twin
    on the CPU.  Returns the twin's margin (None on the device)."""
    depth, mask = image[0], image[1]
    inten = image[2] if len(image) > 2 and grid.intensity is not None else None
    if grid.device.type != "cuda":
        return mesh.integrate_reference(grid, depth, mask, None, inclination, data_type, sensor2ego, inten, min_depth, max_depth, transforms=_np(G)[None])
    depth, mask, inten, _, inc, off, yaw, lo, hi = mesh._frames(grid, depth, mask, None, inclination, data_type, sensor2ego, inten, min_depth, max_depth,
                                                                np.zeros((1, 3, 4)))
    lib = mesh.load()
    dev = grid.device
    _, H, W = depth.shape
    X, Y, Z = grid.dims
    d_inc = mesh._upload(inc, dev)
    G = G.contiguous()
    with torch.cuda.device(dev):
        rc = lib.lrt_mesh_integrate(dev.index, X, Y, Z, grid.voxel, grid.trunc, grid.tsdf.data_ptr(), grid.weight.data_ptr(),
                                    None if grid.intensity is None else grid.intensity.data_ptr(), 1, G.data_ptr(), H, W, depth.data_ptr(), mask.data_ptr(),
                                    None if inten is None else inten.data_ptr(), d_inc.data_ptr(), int(inc.size), off, yaw, lo, hi, mesh._stream(dev))
    if rc != 0:
        raise mesh.MeshError(f"lrt_mesh_integrate failed ({rc}): {lib.lrt_mesh_last_error().decode()}")
    return None


def _mul(A, B):
    """(3, 4) = A B of two rigid (3, 4) float64 tensors, on their device."""
    return torch.cat([A[:, :3] @ B[:, :3], (A[:, :3] @ B[:, 3] + A[:, 3])[:, None]], 1)


@torch.no_grad()
def track_and_fuse(grid, frames, images, first_pose=None, steps=None, iters=DEFAULT_ITERS, huber=0.1, lam=1e-6, min_pairs=50, tol_t=1e-5, tol_r=1e-6,
                   min_weight=1, inclination=None, data_type="KITTI", sensor2ego=None, min_depth=0.0, max_depth=80.0, fuse_first=True):
    """({id: (4, 4) float64 sensor2world}, report): track ``frames`` against ``grid`` and fuse ``images`` into it, in id order (see the module text).
    The report: ``iterations``, ``huber``, per frame ``id``, ``status``, the final number of ``terms`` and ``cond``, the condition number of the last
    hessian (all None for a first frame that was fused without an alignment); ``failed`` names the frames that kept their start pose; ``margin``: the twins' smallest, on the CPU."""
    fn = "track_and_fuse"
    if not isinstance(grid, mesh.TsdfGrid):
        raise MapRegistrationError(f"{fn}: grid must be a mesh.TsdfGrid")
    if inclination is None:
        raise MapRegistrationError(f"{fn}: inclination is required (two bounds or a per-beam table)")
    ids = sorted(int(i) for i in frames)
    if not ids:
        raise MapRegistrationError(f"{fn}: no frames")
    missing = [i for i in ids if i not in images]
    if missing:
        raise MapRegistrationError(f"{fn}: no image for the frames {missing}")
    K = _solver(fn, iters, huber, lam, min_pairs, tol_t, tol_r)[0]
    dev = grid.device
    T0 = np.eye(4) if first_pose is None else np.asarray(first_pose.detach().cpu() if torch.is_tensor(first_pose) else first_pose, np.float64).reshape(-1)
    if T0.size == 12:
        T0 = np.concatenate([T0, [0.0, 0.0, 0.0, 1.0]])
    if T0.size != 16:
        raise MapRegistrationError(f"{fn}: first_pose must be a (4, 4) or (3, 4) matrix")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
    X0 = np.ascontiguousarray(grid_pose(grid, T0.reshape(4, 4))[:3])
    X_prev, G_prev, X_prev2, G_prev2 = up(X0), None, None, None
    est, stat, terms, hess = [], [], [], []
    margin = math.inf
    for n, i in enumerate(ids):
        if n == 0 and fuse_first:
            X, G, st, nt, hs = X_prev, up(inverse_reference(X0)), None, None, None
        else:
            if n == 0:
                start = X_prev
            elif steps is not None:
                if i not in steps:
                    raise MapRegistrationError(f"{fn}: no step for frame {i}")
                start = _mul(X_prev, up(np.asarray(steps[i], np.float64).reshape(4, 4)[:3]))
            elif G_prev2 is not None:
                start = _mul(X_prev, _mul(G_prev2, X_prev))                     # constant velocity: the last step found, once more
            else:
                start = X_prev
            reg = align_to_grid(grid, frames[i], start.contiguous(), K, huber, lam, min_pairs, tol_t, tol_r, min_weight)
            X, G, st, nt, hs = reg.X, reg.G, reg.status, reg.log[-1, 0], reg.hessian
            margin = min(margin, getattr(reg, "margin", math.inf))
        m = _fuse(grid, images[i], G, inclination, data_type, sensor2ego, min_depth, max_depth)
        margin = min(margin, math.inf if m is None else m)
        est.append(X); stat.append(st); terms.append(nt); hess.append(hs)
        X_prev2, G_prev2, X_prev, G_prev = X_prev, G_prev, X, G
    Xs = torch.stack(est).cpu().numpy()                                     # the one host read
    tracked = [k for k, s in enumerate(stat) if s is not None]
    sv = torch.stack([stat[k] for k in tracked]).cpu().numpy() if tracked else np.zeros(0, np.int32)
    tv = torch.stack([terms[k] for k in tracked]).cpu().numpy() if tracked else np.zeros(0)
    hv = torch.stack([hess[k] for k in tracked]).cpu().numpy() if tracked else np.zeros((0, 6, 6))
    T = world_pose(grid, Xs)
    poses = {i: T[k] for k, i in enumerate(ids)}
    rows = [{"id": i, "status": None, "terms": None, "cond": None} for i in ids]
    for j, k in enumerate(tracked):
        cond = float(np.linalg.cond(hv[j])) if hv[j].any() and np.all(np.isfinite(hv[j])) else None
        rows[k] = {"id": ids[k], "status": int(sv[j]), "terms": int(tv[j]), "cond": cond}
    report = {"iterations": K, "huber": float(huber), "frames": rows, "failed": [r["id"] for r in rows if r["status"] in (FEW, PIVOT)]}
    if dev.type != "cuda":
        report["margin"] = margin
    return poses, report
