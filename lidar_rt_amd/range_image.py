"""Range images from point clouds: the spherical projection that keeps the nearest return of every pixel, through ``csrc/liblrt_project.so``.

    img = project_points(points, H, W, inclination, offsets=None, data_type="KITTI", sensor2ego=None, points2sensor=None,
                         max_depth=80.0, min_depth=0.0, wrap=True)          # a RangeImages: depth, intensity, mask, index, counts
    twin = project_points_reference(...)                                     # the float64 numpy twin, plus margin and the per-point decisions

It is the inverse of ``RangeFrames.range_rays`` (``lidar_rt_amd/training.py``): the pixel of every ray of that grid is the pixel the ray was
made for.  ``include/lrt_project.h`` states the rule; ``csrc/lrt_project_math.h`` is its text for the device and the host.

* ``points``: ``(N, 4)`` float32 ``[x, y, z, intensity]`` or ``(N, 3)`` (the intensity is 0 then), all frames back to back.  ``offsets``: ``F + 1``
  ascending row numbers, frame ``f`` owns rows ``offsets[f] .. offsets[f + 1]`` (an empty frame is legal); ``None`` means one frame, and the
  results lose their leading frame axis.  ``points2sensor``: ``(F, 3, 4)`` or ``(F, 4, 4)`` float64, applied in float64 first; ``None``: the
  points are in the sensor frame.  ``inclination``: two bounds ``[inc0, inc1]`` or a strictly monotonic table of ``H >= 3`` beams
  (row ``h`` has ``inclination[H - 1 - h]``, as ``range_rays`` flips it).  ``data_type`` and ``sensor2ego`` give the half-pixel offset and the
  yaw exactly as ``range_rays`` derives them (0.5 and ``atan2`` of the sensor-to-ego rotation in float32 for Waymo, 0 and 0 for KITTI).
* ``offsets``, ``inclination``, ``points2sensor`` and ``sensor2ego`` are HOST data (sequences, numpy arrays, CPU tensors): a few numbers that
  are checked on the host -- ascending offsets, a monotonic table -- before anything is launched, and uploaded without a host wait.
* ``wrap=True`` takes the column modulo ``W``.  ``wrap=False`` is what the reference's loader does
  (lib/dataloader/kitti_loader/__init__.py:222-226): a column index outside ``[0, W)`` is dropped, which loses the half of the column that
  straddles azimuth +-pi (all of column 0 in the KITTI convention on this repository's ray grid).  It is kept as an option for comparisons.
* ``project_points_reference``: the twin.  It is the yardstick: vectorised numpy on the same 64-bit keys (``np.minimum.at``).  ``margin`` is
  the smallest distance of the column coordinate ``u`` and the row coordinate ``v`` of any point that reached the view test from a rounding
  boundary (a half-integer), in pixels; with a beam table the row's distance is measured in radians from the nearest midpoint between two
  beams or outer limit.  Two evaluations of the rule whose ``atan2`` differ in the last bit agree on every pixel while ``margin`` is far
  above 1e-15.
* ``project_points``: HIP float32 tensors go through the library -- three launches, no host wait.  A missing library is an error, and so is
  any other tensor on a HIP device: there is no quiet fall-back.  CPU tensors go to the twin.
"""
from __future__ import annotations

import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LRT_PROJECT_LIB") or os.path.join(HERE, "csrc", "liblrt_project.so")
EXPORTS = ("lrt_project_abi_version", "lrt_project_last_error", "lrt_project_work_bytes", "lrt_project_points")     # include/lrt_project.h
ABI_VERSION = 1
N_COUNTS = 6                                                                 # LRT_PROJECT_N_COUNTS
BLOCK = 256                                                                  # LRT_PROJECT_BLOCK
MAX_POINTS = 2 ** 31 - 1                                                     # LRT_PROJECT_MAX_POINTS
MAX_PIXELS = 2 ** 31 - 1                                                     # LRT_PROJECT_MAX_PIXELS
COUNT_NAMES = ("points", "invalid", "out_of_range", "out_of_view", "hidden", "pixels")
KEEP, INVALID, OUT_OF_RANGE, OUT_OF_VIEW = 0, 1, 2, 3                        # the drop classes of lrt_project_math.h
TWO_PI = 6.28318530717958647692
FLT_MAX = float(np.finfo(np.float32).max)

_lib = None


class ProjectionError(RuntimeError):
    pass


class RangeImages(SimpleNamespace):
    """depth (F, H, W) float32 [m, 0 = no return], intensity (F, H, W) float32, mask (F, H, W) bool, index (F, H, W) int32 (the winner's row
    within its frame, -1 = none), counts (F, 6) int64 (COUNT_NAMES).  Without ``offsets`` the frame axis is dropped.  The twin adds margin,
    pixel (N, 2) int32 (w, h; -1 for a dropped point), range_bits (N) uint32 and drop (N) uint8."""

    def __iter__(self):
        return iter((self.depth, self.intensity, self.mask, self.index, self.counts))


def load():
    """Load liblrt_project.so (after torch, so that both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ProjectionError(f"{LIB_PATH} is missing: build it with `python -m lidar_rt_amd.build` (hipcc --offload-arch=gfx950). "
                              "project_points has no fall-back on a HIP device.")
    lib = C.CDLL(LIB_PATH)
    lib.lrt_project_abi_version.restype = C.c_int
    lib.lrt_project_last_error.restype = C.c_char_p
    lib.lrt_project_work_bytes.restype = C.c_longlong
    lib.lrt_project_work_bytes.argtypes = [C.c_longlong, C.c_int, C.c_int]
    lib.lrt_project_points.restype = C.c_int
    lib.lrt_project_points.argtypes = [C.c_int, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                       C.c_double, C.c_double, C.c_double, C.c_double, C.c_int] + [C.c_void_p] * 6 + [C.c_longlong, C.c_void_p]
    if lib.lrt_project_abi_version() != ABI_VERSION:
        raise ProjectionError("liblrt_project.so ABI version mismatch; rebuild with `python -m lidar_rt_amd.build --force`")
    _lib = lib
    return lib


# ---- the arguments, checked on the host ----------------------------------------------------------------------------------------------------------------

def _host_array(name, x, dtype):
    """A small argument as a numpy array; a tensor on a HIP device is refused (it would have to be read back: a host wait)."""
    if torch.is_tensor(x):
        if x.device.type != "cpu":
            raise ProjectionError(f"project_points: {name} is host data (a sequence, a numpy array or a CPU tensor), it is on {x.device}")
        x = x.detach().numpy()
    try:
        return np.ascontiguousarray(np.asarray(x), dtype=dtype)
    except (TypeError, ValueError) as e:
        raise ProjectionError(f"project_points: {name} is not numeric: {e}") from None


def convention(data_type: str = "KITTI", sensor2ego=None):
    """(off, yaw) of a data type as ``RangeFrames.range_rays`` derives them."""
    if data_type not in ("KITTI", "Waymo"):
        raise ProjectionError(f"project_points: data_type {data_type!r} (KITTI or Waymo)")
    if data_type != "Waymo":
        return 0.0, 0.0
    if sensor2ego is None:
        return 0.5, 0.0
    s = torch.as_tensor(_host_array("sensor2ego", sensor2ego, np.float32))
    if s.dim() != 2 or s.shape[0] < 2 or s.shape[1] < 1:
        raise ProjectionError(f"project_points: sensor2ego must be a (4, 4) matrix (it is {tuple(s.shape)})")
    return 0.5, float(torch.atan2(s[1, 0], s[0, 0]))


def _arguments(shape, H, W, inclination, offsets, data_type, sensor2ego, points2sensor, max_depth, min_depth, wrap):
    """Everything but the points: (N, C, F, offsets int64, inc float64, T float64 or None, off, yaw, min_depth, max_depth, wrap)."""
    if len(shape) != 2 or shape[1] not in (3, 4):
        raise ProjectionError(f"project_points: points must be (N, 4) [x, y, z, intensity] or (N, 3) (they are {tuple(shape)})")
    N, Cc = int(shape[0]), int(shape[1])
    if N > MAX_POINTS:
        raise ProjectionError(f"project_points: {N} points, the in-frame index is int32 (at most {MAX_POINTS})")
    if not (isinstance(H, (int, np.integer)) and isinstance(W, (int, np.integer)) and H >= 1 and W >= 1):
        raise ProjectionError(f"project_points: an image of {H!r} x {W!r} pixels")
    H, W = int(H), int(W)
    if offsets is None:
        off_arr = np.array([0, N], np.int64)
    else:
        off_arr = _host_array("offsets", offsets, np.int64).reshape(-1)
        if off_arr.size < 2:
            raise ProjectionError(f"project_points: offsets holds F + 1 >= 2 row numbers (it holds {off_arr.size})")
        if off_arr[0] != 0 or off_arr[-1] != N or np.any(np.diff(off_arr) < 0):
            raise ProjectionError(f"project_points: offsets must ascend from 0 to {N} (it is {off_arr[:8].tolist()}{' ...' if off_arr.size > 8 else ''})")
    F = off_arr.size - 1
    if F * H * W > MAX_PIXELS:
        raise ProjectionError(f"project_points: {F} frames of {H} x {W} pixels, the pixel index is int32 (F H W at most {MAX_PIXELS})")
    inc = _host_array("inclination", inclination, np.float64).reshape(-1)
    if inc.size != 2 and (inc.size != H or H < 3):
        raise ProjectionError(f"project_points: inclination holds 2 bounds or one angle per row of at least 3 ({H}); it holds {inc.size}")
    if not np.all(np.isfinite(inc)):
        raise ProjectionError("project_points: a non-finite inclination")
    d = np.diff(inc)
    if not (np.all(d > 0) or np.all(d < 0)):
        raise ProjectionError("project_points: the two bounds differ" if inc.size == 2 else "project_points: the inclination table must be strictly monotonic")
    T = None
    if points2sensor is not None:
        T = _host_array("points2sensor", points2sensor, np.float64)
        if T.ndim == 2 and F == 1:
            T = T[None]
        if T.ndim != 3 or T.shape[0] != F or T.shape[1] not in (3, 4) or T.shape[2] != 4:
            raise ProjectionError(f"project_points: points2sensor must be ({F}, 3, 4) or ({F}, 4, 4) (it is {tuple(T.shape)})")
        T = np.ascontiguousarray(T[:, :3, :])
    off, yaw = convention(data_type, sensor2ego)
    min_depth, max_depth = float(min_depth), float(max_depth)
    if not (0.0 <= min_depth < max_depth <= FLT_MAX):
        raise ProjectionError(f"project_points: depths ({min_depth}, {max_depth}] (0 <= min < max <= FLT_MAX)")
    return N, Cc, F, off_arr, inc, T, off, yaw, min_depth, max_depth, bool(wrap)


# ---- the twin ------------------------------------------------------------------------------------------------------------------------------------------

def _table_rows(el, inc, H):
    """Rows of the elevations el in a strictly monotonic table (row h <-> inc[H - 1 - h]): (row or -1, distance to the nearest decision boundary)."""
    asc = inc[H - 1] > inc[0]
    s = inc if asc else inc[::-1]
    lo = np.searchsorted(s, el, side="right")
    row = np.full(el.shape, -1, np.int64)
    k = np.zeros(el.shape, np.int64)
    below, above = lo == 0, lo == H
    mid = ~below & ~above
    ok = np.zeros(el.shape, bool)
    ok[below] = (s[0] - el[below]) <= 0.5 * (s[1] - s[0])
    ok[above] = (el[above] - s[H - 1]) <= 0.5 * (s[H - 1] - s[H - 2])
    k[above] = H - 1
    lm = lo[mid]
    dl, dh = el[mid] - s[lm - 1], s[lm] - el[mid]
    k[mid] = np.where(dl < dh, lm - 1, np.where(dh < dl, lm, lm if asc else lm - 1))
    ok[mid] = True
    t = k if asc else H - 1 - k
    row[ok] = (H - 1 - t)[ok]
    bnd = np.concatenate([[s[0] - 0.5 * (s[1] - s[0])], 0.5 * (s[:-1] + s[1:]), [s[H - 1] + 0.5 * (s[H - 1] - s[H - 2])]])
    j = np.searchsorted(bnd, el)
    dist = np.minimum(np.abs(el - bnd[np.clip(j - 1, 0, H)]), np.abs(el - bnd[np.clip(j, 0, H)]))
    return row, dist


def _twin(pts, N, F, off_arr, inc, T, off, yaw, min_depth, max_depth, wrap, H, W):
    """numpy, float64.  pts (N, 4) float32.  The operations and their order are those of lrt_project_math.h."""
    frame = np.repeat(np.arange(F, dtype=np.int64), np.diff(off_arr))
    local = np.arange(N, dtype=np.int64) - off_arr[frame]
    x, y, z = (pts[:, k].astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        if T is not None:
            R = T[frame]
            x, y, z = (R[:, k, 0] * x + R[:, k, 1] * y + R[:, k, 2] * z + R[:, k, 3] for k in range(3))
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        r = np.sqrt(x * x + y * y + z * z)
        invalid = ~finite | (r == 0.0)
        r32 = r.astype(np.float32)
        rd = r32.astype(np.float64)
        in_range = (rd > min_depth) & (rd <= max_depth)
        az = np.arctan2(y, x)
        el = np.arctan2(z, np.hypot(x, y))
        u = (np.pi - (az + yaw)) * float(W) / TWO_PI - off
        w = np.rint(u)
        if wrap:
            w = w - np.floor(w / float(W)) * float(W)
        w_ok = (w >= 0.0) & (w < float(W))
        if inc.size == 2:
            t = (el - inc[0]) / (inc[1] - inc[0]) * float(H)
            v = float(H) - off - t
            h = np.rint(v)
            h_ok = (h >= 0.0) & (h < float(H))
            dist_v = np.abs(np.abs(v - h) - 0.5)
        else:
            safe = np.where(np.isfinite(el), el, 0.0)
            h, dist_v = _table_rows(safe, inc, H)
            h_ok = h >= 0
            h = h.astype(np.float64)
        dist_u = np.abs(np.abs(u - np.rint(u)) - 0.5)
    seen = ~invalid & in_range                                               # the points that reach the view test
    drop = np.full(N, KEEP, np.uint8)
    drop[seen & ~(w_ok & h_ok)] = OUT_OF_VIEW
    drop[~invalid & ~in_range] = OUT_OF_RANGE
    drop[invalid] = INVALID
    kept = drop == KEEP
    margin = float(min(dist_u[seen].min(), dist_v[seen].min())) if seen.any() else float("inf")
    wi = np.where(kept, w, -1.0).astype(np.int64)
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
    for c, sel in ((1, drop == INVALID), (2, drop == OUT_OF_RANGE), (3, drop == OUT_OF_VIEW)):
        counts[:, c] = np.bincount(frame[sel], minlength=F)
    counts[:, 5] = hit.reshape(F, -1).sum(1)
    counts[:, 4] = np.bincount(frame[kept], minlength=F) - counts[:, 5]
    sh = (F, H, W)
    return SimpleNamespace(depth=depth.reshape(sh), intensity=intensity.reshape(sh), mask=hit.reshape(sh), index=index.reshape(sh), counts=counts, margin=margin,
                           pixel=np.stack([wi, hi], 1).astype(np.int32), range_bits=bits, drop=drop)


def project_points_reference(points, H, W, inclination, offsets=None, data_type="KITTI", sensor2ego=None, points2sensor=None, max_depth=80.0,
                             min_depth=0.0, wrap=True) -> RangeImages:
    """The float64 numpy twin (see the module text).  ``points``: a tensor on any device or a numpy array; the results are CPU tensors."""
    pts = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
    N, Cc, F, off_arr, inc, T, off, yaw, min_depth, max_depth, wrap = _arguments(pts.shape, H, W, inclination, offsets, data_type, sensor2ego, points2sensor,
                                                                                  max_depth, min_depth, wrap)
    pts = np.ascontiguousarray(pts, np.float32)
    if Cc == 3:
        pts = np.concatenate([pts, np.zeros((N, 1), np.float32)], 1)
    r = _twin(pts, N, F, off_arr, inc, T, off, yaw, min_depth, max_depth, wrap, int(H), int(W))
    sq = (lambda a: a[0]) if offsets is None else (lambda a: a)
    return RangeImages(depth=torch.from_numpy(sq(r.depth)), intensity=torch.from_numpy(sq(r.intensity)), mask=torch.from_numpy(sq(r.mask)),
                       index=torch.from_numpy(sq(r.index)), counts=torch.from_numpy(sq(r.counts)), margin=r.margin,
                       pixel=torch.from_numpy(r.pixel), range_bits=r.range_bits, drop=torch.from_numpy(r.drop))


# ---- the operator ----------------------------------------------------------------------------------------------------------------------------------------

def work_bytes(F: int, H: int, W: int) -> int:
    """Bytes of the workspace of one call: the key image."""
    n = int(load().lrt_project_work_bytes(int(F), int(H), int(W)))
    if n < 0:
        raise ProjectionError(f"project_points: {F} frames of {H} x {W} pixels (each at least 1, F H W at most {MAX_PIXELS})")
    return n


def _upload(a: np.ndarray, dev) -> torch.Tensor:
    """A small host array on the device without a host wait: through pinned memory, which the allocator keeps until the copy has run."""
    return torch.from_numpy(a).pin_memory().to(dev, non_blocking=True)


@torch.no_grad()
def project_points(points, H, W, inclination, offsets=None, data_type="KITTI", sensor2ego=None, points2sensor=None, max_depth=80.0, min_depth=0.0,
                   wrap=True, workspace=None) -> RangeImages:
    """F frames of points into F range images (see the module text).  The inputs are not changed.  ``workspace``: a uint8 tensor on the points'
    device of at least ``work_bytes(F, H, W)`` bytes to use instead of a fresh one; its contents do not matter."""
    if not torch.is_tensor(points):
        raise ProjectionError(f"project_points: points must be a tensor (it is {type(points).__name__}); numpy arrays go to project_points_reference")
    N, Cc, F, off_arr, inc, T, off, yaw, min_depth, max_depth, wrap = _arguments(tuple(points.shape), H, W, inclination, offsets, data_type, sensor2ego,
                                                                                  points2sensor, max_depth, min_depth, wrap)
    dev = points.device
    if dev.type != "cuda":
        if workspace is not None:
            raise ProjectionError(f"project_points: a workspace with points on {dev}")
        r = project_points_reference(points, H, W, inclination, offsets, data_type, sensor2ego, points2sensor, max_depth, min_depth, wrap)
        return RangeImages(depth=r.depth, intensity=r.intensity, mask=r.mask, index=r.index, counts=r.counts, margin=r.margin)
    lib = load()
    if points.dtype != torch.float32 or not points.is_contiguous():
        raise ProjectionError(f"lrt_project: points must be a contiguous float32 tensor (they are {points.dtype}, {'contiguous' if points.is_contiguous() else 'not contiguous'}); "
                              "there is no fall-back to PyTorch on a HIP device")
    H, W = int(H), int(W)
    nbytes = work_bytes(F, H, W)
    if workspace is not None:
        if not (torch.is_tensor(workspace) and workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.device == dev
                and workspace.numel() >= nbytes and workspace.data_ptr() % 256 == 0):
            raise ProjectionError(f"lrt_project: the workspace must be a contiguous uint8 tensor of at least {nbytes} bytes on {dev}, 256-byte aligned")
        ws = workspace
    else:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)                # the caching allocator's blocks are 512-byte aligned
    pts = points.detach()
    if Cc == 3:
        pts = torch.cat([pts, torch.zeros((N, 1), dtype=torch.float32, device=dev)], 1)
    d_off, d_inc = _upload(off_arr, dev), _upload(inc, dev)
    d_T = None if T is None else _upload(T, dev)
    depth = torch.empty((F, H, W), dtype=torch.float32, device=dev)
    intensity = torch.empty((F, H, W), dtype=torch.float32, device=dev)
    mask = torch.empty((F, H, W), dtype=torch.uint8, device=dev)
    index = torch.empty((F, H, W), dtype=torch.int32, device=dev)
    counts = torch.empty((F, N_COUNTS), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.lrt_project_points(dev.index, N, pts.data_ptr() if N else None, F, d_off.data_ptr(), None if d_T is None else d_T.data_ptr(), H, W,
                                    d_inc.data_ptr(), int(inc.size), off, yaw, min_depth, max_depth, int(wrap), depth.data_ptr(), intensity.data_ptr(),
                                    mask.data_ptr(), index.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
                                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise ProjectionError(f"lrt_project_points failed ({rc}): {lib.lrt_project_last_error().decode()}")
    mask = mask.view(torch.bool)
    if offsets is None:
        depth, intensity, mask, index, counts = depth[0], intensity[0], mask[0], index[0], counts[0]
    return RangeImages(depth=depth, intensity=intensity, mask=mask, index=index, counts=counts)
