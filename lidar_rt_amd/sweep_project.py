"""Range images of a MOVING sensor from point clouds: the projection under the sweep model, through ``csrc/liblrt_sweepproj.so``.

    img = project_points_sweep(points, H, W, inclination, twist, offsets=None, data_type="KITTI", sensor2ego=None, points2sensor=None,
                               tau=None, t_ref=0.5, direction="cw", max_depth=80.0, min_depth=0.0, wrap=True)     # a RangeImages, counts (F, 7)
    twin = project_points_sweep_reference(...)           # the float64 numpy twin, plus evals, margin, range_margin and the per-point decisions

It is the inverse of ``sweep.sweep_rays`` as ``range_image.project_points`` is the inverse of ``RangeFrames.range_rays``: column ``w`` of a moving
sensor is fired from its own pose ``P Exp(tau[w] twist)``, so a point belongs to the column that, at its own instant, has the point inside its
azimuth bin, and its range is measured from that column's origin.  ``include/lrt_sweepproj.h`` states the rule; ``csrc/lrt_sweepproj_math.h``
is its text for the device and the host.

* ``points``, ``offsets``, ``inclination``, ``data_type``, ``sensor2ego``, ``points2sensor``, the depths and ``wrap`` are
  ``range_image.project_points``'s, with its checks and refusals.  The points are given in the sensor frame of the frame's REFERENCE instant
  (``tau == 0``) -- a motion-compensated scan -- or are taken there by ``points2sensor`` (the inverse pose, for world points).  The frame's pose
  itself never enters.
* ``twist``: ``(6,)`` or ``(F, 6)`` float64 HOST data ``(rho, phi)``, the sensor's motion over one sweep in the sensor frame (the convention of
  ``sweep.sweep_rays`` and ``poses.se3_exp``); ``(6,)`` serves every frame; ``None`` is a static sensor.  A tensor on a HIP device is refused:
  reading it would be a host wait.  ``tau``: ``(W,)`` float64 host data, the instant of every column in sweeps; ``None`` means
  ``sweep.column_times(W, t_ref, direction)``.
* The search: from the static column of the point, at most ``MAX_EVAL`` evaluations of "which column does the column I stand on see the point
  in".  A converged column has the point inside its bin at its own instant.  When the sensor turns or translates, the bins of consecutive
  columns, taken at their own instants, leave gaps -- an adjacent pair can point at each other -- and such points are counted as ``unseen``;
  they are real.  At the seam the first and the last column are a whole sweep apart: there is a gap or an overlap, and in an overlap the rule
  keeps the sighting that the search from the static column reaches.  A point becomes at most one pixel.
* With ``twist=None`` or zeros every output equals ``range_image.project_points`` on the same arguments bit for bit, and ``unseen`` is 0.
* ``project_points_sweep_reference``: the twin, the same operations in the header's order.  Unlike the static rule the point passes through
  ``Exp``, whose multiply-adds the device may fuse: a column's pose, and with it ``u`` and ``r``, can differ from the host's in the last bits.
  ``evals (N,)``: the evaluations used per point (0 for a point that is not finite).  ``margin``: the smallest distance of ANY evaluated ``u`` --
  the static one and every evaluation of every finite point -- and of the row coordinate of every point that reached the row test from its
  rounding boundary (``range_image``'s units); a point on the z axis (x == y == 0, where ``atan2`` is exact in every library) has no ``u`` to
  guard.  ``range_margin``: the smallest relative distance of a kept point's float64 ``r`` from the
  midpoint between two neighbouring float32 values.  Bit-for-bit comparisons hold on inputs that keep both far above 1e-15.
* ``project_points_sweep``: HIP float32 tensors go through the library -- four launches, no host wait.  A missing library is an error, and so is
  any other tensor on a HIP device: there is no quiet fall-back.  CPU tensors go to the twin.
"""
from __future__ import annotations

import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import sweep
from .range_image import (INVALID, KEEP, OUT_OF_RANGE, OUT_OF_VIEW, TWO_PI, ProjectionError, RangeImages, _arguments, _host_array, _table_rows,
                          _upload)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LRT_SWEEPPROJ_LIB") or os.path.join(HERE, "csrc", "liblrt_sweepproj.so")
EXPORTS = ("lrt_sweepproj_abi_version", "lrt_sweepproj_last_error", "lrt_sweepproj_work_bytes", "lrt_sweepproj_points")     # include/lrt_sweepproj.h
ABI_VERSION = 1
N_COUNTS = 7                                                                 # LRT_SWEEPPROJ_N_COUNTS
MAX_EVAL = 8                                                                 # LRT_SWEEPPROJ_MAX_EVAL
TABLE = 12                                                                   # LRT_SWEEPPROJ_TABLE
BLOCK = 256                                                                  # LRT_SWEEPPROJ_BLOCK
MAX_POINTS = 2 ** 31 - 1                                                     # LRT_SWEEPPROJ_MAX_POINTS
MAX_PIXELS = 2 ** 31 - 1                                                     # LRT_SWEEPPROJ_MAX_PIXELS
COUNT_NAMES = ("points", "invalid", "out_of_range", "out_of_view", "unseen", "hidden", "pixels")
UNSEEN = 4                                                                   # SP_UNSEEN, after range_image's KEEP .. OUT_OF_VIEW
CONVERGED, EDGE, CYCLE = 0, 1, 2                                             # how a search ended (SP_CONVERGED, SP_EDGE, SP_CYCLE)

_lib = None


def load():
    """Load liblrt_sweepproj.so (after torch, so that both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ProjectionError(f"{LIB_PATH} is missing: build it with `python -m lidar_rt_amd.build` (hipcc --offload-arch=gfx950). "
                              "project_points_sweep has no fall-back on a HIP device.")
    lib = C.CDLL(LIB_PATH)
    lib.lrt_sweepproj_abi_version.restype = C.c_int
    lib.lrt_sweepproj_last_error.restype = C.c_char_p
    lib.lrt_sweepproj_work_bytes.restype = C.c_longlong
    lib.lrt_sweepproj_work_bytes.argtypes = [C.c_longlong, C.c_int, C.c_int]
    lib.lrt_sweepproj_points.restype = C.c_int
    lib.lrt_sweepproj_points.argtypes = [C.c_int, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                         C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int] + [C.c_void_p] * 6 + [C.c_longlong, C.c_void_p]
    if lib.lrt_sweepproj_abi_version() != ABI_VERSION:
        raise ProjectionError("liblrt_sweepproj.so ABI version mismatch; rebuild with `python -m lidar_rt_amd.build --force`")
    _lib = lib
    return lib


# ---- the arguments, checked on the host ----------------------------------------------------------------------------------------------------------------

def _motion(twist, tau, F, W, t_ref, direction):
    """(xi (F, 6) float64 or None, tau (W,) float64): host data, finite."""
    xi = None
    if twist is not None:
        xi = _host_array("twist", twist, np.float64)
        if xi.shape == (6,):
            xi = np.array(np.broadcast_to(xi, (F, 6)))                        # a copy: a broadcast view is read-only
        if xi.shape != (F, 6):
            raise ProjectionError(f"project_points_sweep: twist must be (6,) or ({F}, 6) (it is {tuple(xi.shape)})")
        if not np.all(np.isfinite(xi)):
            raise ProjectionError("project_points_sweep: a non-finite twist")
        xi = np.ascontiguousarray(xi)
    if tau is None:
        try:
            t = sweep.column_times(W, t_ref, direction).numpy()
        except sweep.SweepError as e:
            raise ProjectionError(f"project_points_sweep: {e}") from None
    else:
        t = _host_array("tau", tau, np.float64).reshape(-1)
        if t.size != W:
            raise ProjectionError(f"project_points_sweep: tau must hold {W} column times (it holds {t.size})")
    if not np.all(np.isfinite(t)):
        raise ProjectionError("project_points_sweep: a non-finite tau")
    return xi, np.ascontiguousarray(t, np.float64)


# ---- the twin ------------------------------------------------------------------------------------------------------------------------------------------

def _nested(u, j):
    v = np.ones_like(u)
    for k in range(sweep.SERIES_TERMS - 1, -1, -1):
        v = 1.0 - u * v / float((2 * k + 2 + j) * (2 * k + 3 + j))
    return v


def column_table_reference(xi, tau):
    """(F, W, 12) float64: the inverse of Exp(tau[w] xi[f]) as a row-major 3 x 4, in the order of sw_exp and sp_column_entry."""
    x = tau[None, :, None] * xi[:, None, :]
    rho, phi = [x[..., k] for k in range(3)], [x[..., 3 + k] for k in range(3)]
    u = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]
    small = u < sweep.SERIES_TH2
    us = np.where(small, 1.0, u)                                             # keeps the unused branch finite
    t = np.sqrt(us)
    sn, cs = np.sin(t), np.cos(t)
    A = np.where(small, _nested(u, 0), sn / t)
    B = np.where(small, _nested(u, 1) * 0.5, (1.0 - cs) / us)
    Cc = np.where(small, _nested(u, 2) / 6.0, (t - sn) / (us * t))
    z = np.zeros_like(u)
    K = [[z, -phi[2], phi[1]], [phi[2], z, -phi[0]], [-phi[1], phi[0], z]]
    K2 = [[K[i][0] * K[0][j] + K[i][1] * K[1][j] + K[i][2] * K[2][j] for j in range(3)] for i in range(3)]
    Re = [[(1.0 if i == j else 0.0) + A * K[i][j] + B * K2[i][j] for j in range(3)] for i in range(3)]
    te = []
    for i in range(3):
        s = np.zeros_like(u)
        for j in range(3):
            s = s + ((1.0 if i == j else 0.0) + B * K[i][j] + Cc * K2[i][j]) * rho[j]
        te.append(s)
    E = np.empty(u.shape + (TABLE,), np.float64)
    for i in range(3):
        for j in range(3):
            E[..., 4 * i + j] = Re[j][i]
        E[..., 4 * i + 3] = -(Re[0][i] * te[0] + Re[1][i] * te[1] + Re[2][i] * te[2])
    return E


_IDENTITY = np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0])


def _column_of(c, W, wrap):
    """sp_column_of: a rounded u as a column of [0, W), whatever it holds."""
    Wf = float(W)
    if wrap:
        c = c - np.floor(c / Wf) * Wf
        return np.where((c >= 0.0) & (c < Wf), c, 0.0).astype(np.int64)
    return np.where(c < Wf, np.where(c >= 0.0, c, 0.0), Wf - 1.0).astype(np.int64)


def _range_margin(r):
    """The smallest relative distance of r (float64, positive, finite) from a midpoint between two neighbouring float32 values."""
    if r.size == 0:
        return float("inf")
    r32 = r.astype(np.float32)
    up = np.nextafter(r32, np.float32(np.inf)).astype(np.float64)
    dn = np.nextafter(r32, np.float32(-np.inf)).astype(np.float64)
    c = r32.astype(np.float64)
    return float((np.minimum(np.abs(0.5 * (c + up) - r), np.abs(r - 0.5 * (c + dn))) / r).min())


def _twin(pts, N, F, off_arr, inc, T, off, yaw, min_depth, max_depth, wrap, H, W, xi, tau):
    """numpy, float64.  pts (N, 4) float32.  The operations and their order are those of lrt_sweepproj_math.h."""
    frame = np.repeat(np.arange(F, dtype=np.int64), np.diff(off_arr))
    local = np.arange(N, dtype=np.int64) - off_arr[frame]
    table = None if xi is None else column_table_reference(xi, tau)
    Wf, Hf = float(W), float(H)
    u_of = lambda a: (np.pi - (np.arctan2(a[:, 1], a[:, 0]) + yaw)) * Wf / TWO_PI - off
    dist = lambda u, a: np.where((a[:, 0] == 0.0) & (a[:, 1] == 0.0), np.inf, np.abs(np.abs(u - np.rint(u)) - 0.5))     # atan2(+-0, +-0) is exact everywhere
    margins = [np.inf]
    with np.errstate(all="ignore"):
        p = np.stack([pts[:, k].astype(np.float64) for k in range(3)], 1)
        if T is not None:
            R = T[frame]
            p = np.stack([R[:, k, 0] * p[:, 0] + R[:, k, 1] * p[:, 1] + R[:, k, 2] * p[:, 2] + R[:, k, 3] for k in range(3)], 1)
        valid = np.isfinite(p).all(1)
        idx = np.flatnonzero(valid)                                          # the points whose search goes on
        q = p.copy()
        col = np.zeros(N, np.int64)
        evals = np.zeros(N, np.int32)
        state = np.full(N, CYCLE, np.int8)
        u0 = u_of(p[idx])
        col[idx] = _column_of(np.rint(u0), W, wrap)
        if idx.size:
            margins.append(dist(u0, p[idx]).min())
        for k in range(MAX_EVAL):
            if idx.size == 0:
                break
            pk = p[idx]
            if table is None:
                qk = pk
            else:
                E = table[frame[idx], col[idx]]
                moved = np.stack([E[:, 4 * i] * pk[:, 0] + E[:, 4 * i + 1] * pk[:, 1] + E[:, 4 * i + 2] * pk[:, 2] + E[:, 4 * i + 3] for i in range(3)], 1)
                qk = np.where((E == _IDENTITY).all(1)[:, None], pk, moved)
            q[idx] = qk
            evals[idx] += 1
            u = u_of(qk)
            margins.append(dist(u, qk).min())
            c = np.rint(u)
            nxt = _column_of(c, W, wrap)
            same = nxt == col[idx]
            inside = np.ones(idx.size, bool) if wrap else (c >= 0.0) & (c < Wf)
            state[idx[same & inside]] = CONVERGED
            state[idx[same & ~inside]] = EDGE
            if k + 1 < MAX_EVAL:
                col[idx[~same]] = nxt[~same]
            idx = idx[~same]
        x, y, z = q[:, 0], q[:, 1], q[:, 2]
        finite = valid & np.isfinite(q).all(1)
        r = np.sqrt(x * x + y * y + z * z)
        invalid = ~finite | (r == 0.0)
        r32 = r.astype(np.float32)
        rd = r32.astype(np.float64)
        in_range = (rd > min_depth) & (rd <= max_depth)
        el = np.arctan2(z, np.hypot(x, y))
        if inc.size == 2:
            t = (el - inc[0]) / (inc[1] - inc[0]) * Hf
            v = Hf - off - t
            h = np.rint(v)
            h_ok = (h >= 0.0) & (h < Hf)
            dist_v = np.abs(np.abs(v - h) - 0.5)
        else:
            safe = np.where(np.isfinite(el), el, 0.0)
            h, dist_v = _table_rows(safe, inc, H)
            h_ok = h >= 0
            h = h.astype(np.float64)
    seen = ~invalid & in_range
    at_row = seen & (state == CONVERGED)                                     # the points that reach the row test
    drop = np.full(N, KEEP, np.uint8)
    drop[at_row & ~h_ok] = OUT_OF_VIEW
    drop[seen & (state == CYCLE)] = UNSEEN
    drop[seen & (state == EDGE)] = OUT_OF_VIEW
    drop[~invalid & ~in_range] = OUT_OF_RANGE
    drop[invalid] = INVALID
    kept = drop == KEEP
    if at_row.any():
        margins.append(dist_v[at_row].min())
    margin = float(min(margins))
    wi = np.where(kept, col, -1).astype(np.int64)
    hi = np.where(kept, h, -1.0).astype(np.int64)
    bits = np.where(invalid, np.float32(0), r32).astype(np.float32).view(np.uint32)
    n_pix = F * H * W
    keys = np.full(n_pix, np.iinfo(np.uint64).max, np.uint64)
    pix = (frame[kept] * H + hi[kept]) * W + wi[kept]
    key = (bits[kept].astype(np.uint64) << np.uint64(32)) | local[kept].astype(np.uint64)
    np.minimum.at(keys, pix, key)
    hit = keys != np.iinfo(np.uint64).max
    depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0)).astype(np.float32)
    index = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    fpix = np.arange(n_pix, dtype=np.int64) // (H * W)
    rows = off_arr[fpix] + np.where(hit, index, 0)
    intensity = np.where(hit, pts[np.clip(rows, 0, max(N - 1, 0)), 3] if N else np.float32(0), np.float32(0)).astype(np.float32)
    counts = np.zeros((F, N_COUNTS), np.int64)
    counts[:, 0] = np.diff(off_arr)
    for c_, cls in ((1, INVALID), (2, OUT_OF_RANGE), (3, OUT_OF_VIEW), (4, UNSEEN)):
        counts[:, c_] = np.bincount(frame[drop == cls], minlength=F)
    counts[:, 6] = hit.reshape(F, -1).sum(1)
    counts[:, 5] = np.bincount(frame[kept], minlength=F) - counts[:, 6]
    sh = (F, H, W)
    return SimpleNamespace(depth=depth.reshape(sh), intensity=intensity.reshape(sh), mask=hit.reshape(sh), index=index.reshape(sh), counts=counts, margin=margin,
                           range_margin=_range_margin(r[kept]), pixel=np.stack([wi, hi], 1).astype(np.int32), range_bits=bits, drop=drop, evals=evals)


def project_points_sweep_reference(points, H, W, inclination, twist, offsets=None, data_type="KITTI", sensor2ego=None, points2sensor=None, tau=None,
                                   t_ref=0.5, direction="cw", max_depth=80.0, min_depth=0.0, wrap=True) -> RangeImages:
    """The float64 numpy twin (see the module text).  ``points``: a tensor on any device or a numpy array; the results are CPU tensors."""
    pts = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
    N, Cc, F, off_arr, inc, T, off, yaw, min_depth, max_depth, wrap = _arguments(pts.shape, H, W, inclination, offsets, data_type, sensor2ego, points2sensor,
                                                                                  max_depth, min_depth, wrap)
    xi, tau = _motion(twist, tau, F, int(W), t_ref, direction)
    pts = np.ascontiguousarray(pts, np.float32)
    if Cc == 3:
        pts = np.concatenate([pts, np.zeros((N, 1), np.float32)], 1)
    r = _twin(pts, N, F, off_arr, inc, T, off, yaw, min_depth, max_depth, wrap, int(H), int(W), xi, tau)
    sq = (lambda a: a[0]) if offsets is None else (lambda a: a)
    return RangeImages(depth=torch.from_numpy(sq(r.depth)), intensity=torch.from_numpy(sq(r.intensity)), mask=torch.from_numpy(sq(r.mask)),
                       index=torch.from_numpy(sq(r.index)), counts=torch.from_numpy(sq(r.counts)), margin=r.margin, range_margin=r.range_margin,
                       pixel=torch.from_numpy(r.pixel), range_bits=r.range_bits, drop=torch.from_numpy(r.drop), evals=torch.from_numpy(r.evals))


# ---- the operator ----------------------------------------------------------------------------------------------------------------------------------------

def work_bytes(F: int, H: int, W: int) -> int:
    """Bytes of the workspace of one call: the key image and the column table."""
    n = int(load().lrt_sweepproj_work_bytes(int(F), int(H), int(W)))
    if n < 0:
        raise ProjectionError(f"project_points_sweep: {F} frames of {H} x {W} pixels (each at least 1, F H W at most {MAX_PIXELS})")
    return n


@torch.no_grad()
def project_points_sweep(points, H, W, inclination, twist, offsets=None, data_type="KITTI", sensor2ego=None, points2sensor=None, tau=None, t_ref=0.5,
                         direction="cw", max_depth=80.0, min_depth=0.0, wrap=True, workspace=None) -> RangeImages:
    """F frames of points into the F range images a moving sensor records (see the module text).  The inputs are not changed.  ``workspace``: a
    uint8 tensor on the points' device of at least ``work_bytes(F, H, W)`` bytes to use instead of a fresh one; its contents do not matter."""
    if not torch.is_tensor(points):
        raise ProjectionError(f"project_points_sweep: points must be a tensor (it is {type(points).__name__}); numpy arrays go to project_points_sweep_reference")
    N, Cc, F, off_arr, inc, T, off, yaw, min_depth, max_depth, wrap = _arguments(tuple(points.shape), H, W, inclination, offsets, data_type, sensor2ego,
                                                                                  points2sensor, max_depth, min_depth, wrap)
    H, W = int(H), int(W)
    xi, tau_arr = _motion(twist, tau, F, W, t_ref, direction)
    dev = points.device
    if dev.type != "cuda":
        if workspace is not None:
            raise ProjectionError(f"project_points_sweep: a workspace with points on {dev}")
        r = project_points_sweep_reference(points, H, W, inclination, xi, offsets, data_type, sensor2ego, points2sensor, tau_arr, t_ref, direction, max_depth,
                                           min_depth, wrap)
        return RangeImages(depth=r.depth, intensity=r.intensity, mask=r.mask, index=r.index, counts=r.counts, margin=r.margin, range_margin=r.range_margin)
    lib = load()
    if points.dtype != torch.float32 or not points.is_contiguous():
        raise ProjectionError(f"lrt_sweepproj: points must be a contiguous float32 tensor (they are {points.dtype}, {'contiguous' if points.is_contiguous() else 'not contiguous'}); "
                              "there is no fall-back to PyTorch on a HIP device")
    nbytes = work_bytes(F, H, W)
    if workspace is not None:
        if not (torch.is_tensor(workspace) and workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.device == dev
                and workspace.numel() >= nbytes and workspace.data_ptr() % 256 == 0):
            raise ProjectionError(f"lrt_sweepproj: the workspace must be a contiguous uint8 tensor of at least {nbytes} bytes on {dev}, 256-byte aligned")
        ws = workspace
    else:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)                # the caching allocator's blocks are 512-byte aligned
    pts = points.detach()
    if Cc == 3:
        pts = torch.cat([pts, torch.zeros((N, 1), dtype=torch.float32, device=dev)], 1)
    d_off, d_inc = _upload(off_arr, dev), _upload(inc, dev)
    d_T = None if T is None else _upload(T, dev)
    d_xi = None if xi is None else _upload(xi, dev)
    d_tau = None if xi is None else _upload(tau_arr, dev)
    depth = torch.empty((F, H, W), dtype=torch.float32, device=dev)
    intensity = torch.empty((F, H, W), dtype=torch.float32, device=dev)
    mask = torch.empty((F, H, W), dtype=torch.uint8, device=dev)
    index = torch.empty((F, H, W), dtype=torch.int32, device=dev)
    counts = torch.empty((F, N_COUNTS), dtype=torch.int64, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        rc = lib.lrt_sweepproj_points(dev.index, N, pts.data_ptr() if N else None, F, d_off.data_ptr(), ptr(d_T), ptr(d_xi), ptr(d_tau), H, W,
                                      d_inc.data_ptr(), int(inc.size), off, yaw, min_depth, max_depth, int(wrap), depth.data_ptr(), intensity.data_ptr(),
                                      mask.data_ptr(), index.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
                                      C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise ProjectionError(f"lrt_sweepproj_points failed ({rc}): {lib.lrt_sweepproj_last_error().decode()}")
    mask = mask.view(torch.bool)
    if offsets is None:
        depth, intensity, mask, index, counts = depth[0], intensity[0], mask[0], index[0], counts[0]
    return RangeImages(depth=depth, intensity=intensity, mask=mask, index=index, counts=counts)
