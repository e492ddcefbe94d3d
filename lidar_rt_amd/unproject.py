"""Point clouds from range images: the kept pixels' points, compacted in the order boolean indexing gives, through ``csrc/liblrt_unproject.so``.

    pc = points_from_range_images(depth, rays_o, rays_d, intensity=None, keep=None, raydrop=None, raydrop_ratio=0.4,
                                  world2out=None, min_depth=0.0, max_depth=FLT_MAX, workspace=None)     # a PointClouds
    twin = points_from_range_images_reference(...)                            # numpy, runs anywhere

It is the inverse of ``range_image.project_points`` / ``sweep_project.project_points_sweep``: a render (a depth per ray) becomes the scan a
downstream stack reads.  ``include/lrt_unproject.h`` states the rule; ``csrc/lrt_unproject_math.h`` is its text for the device and the host.

* ``depth``, ``intensity``, ``raydrop``: float32 ``(F, H, W)``; ``keep``: bool or uint8 ``(F, H, W)``; ``rays_o``, ``rays_d``: float32
  ``(F, H, W, 3)``.  Without the frame axis (``(H, W)`` and ``(H, W, 3)``) ``counts`` loses it too and ``trim()`` returns one cloud.
* A pixel gets exactly one class, the first that applies: ``invalid`` (a non-finite depth, origin or direction), ``masked`` (``keep == 0``, or
  not ``raydrop < raydrop_ratio``: ``evaluation.evaluate``'s rule; the ratio is read as float32, as torch compares a float32 tensor with a
  number), ``out_of_range`` (not ``min_depth < depth <= max_depth``; a depth of 0, "no return", falls here), else kept.
* ``world2out=None``: ``p = o + d * r`` in float32, product and sum rounded on their own -- bit for bit what
  ``RangeFrames.inverse_projection_with_range`` returns.  ``world2out``: HOST float64 (a numpy array, a CPU tensor), ``(F, 3|4, 4)`` one
  transform per frame or ``(F, W, 3|4, 4)`` one per COLUMN (the frame of a moving sensor); ``(x, y, z) = o + d * r`` and ``q = T (x, y, z, 1)``
  are formed in float64, each row summed left to right, and rounded to float32 once.  That is the accurate path: far from the origin the
  float32 sum loses the low bits of ``d * r``, and the range recomputed from the point is off by ``|o| / r`` ulps.
* ``PointClouds``: ``points (cap, 4)`` float32 ``[x, y, z, intensity]`` (intensity 0 without one), ``pixel (cap,)`` int32 ``h * W + w`` (ring
  ``pixel // W``, column ``pixel % W``), ``offsets (F + 1,)`` int64, ``counts (F, 5)`` int64 (``COUNT_NAMES``); ``cap = F H W``, rows ordered by
  frame, then row-major pixel; rows from ``offsets[-1]`` on are not written.  ``trim()`` is the one place that waits: it reads ``offsets`` and
  returns per-frame views.
* ``points_from_range_images``: HIP float32 tensors go through the library -- three launches, no atomics, no host wait.  A missing library is an
  error, and so is a tensor that is not contiguous float32: there is no quiet fall-back.  CPU tensors go to the twin.
"""
from __future__ import annotations

import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LRT_UNPROJECT_LIB") or os.path.join(HERE, "csrc", "liblrt_unproject.so")
EXPORTS = ("lrt_unproject_abi_version", "lrt_unproject_last_error", "lrt_unproject_work_bytes", "lrt_unproject_points")     # include/lrt_unproject.h
ABI_VERSION = 1
N_COUNTS = 5                                                                 # LRT_UNPROJECT_N_COUNTS
BLOCK = 256                                                                  # LRT_UNPROJECT_BLOCK
MAX_PIXELS = 2 ** 31 - 1                                                     # LRT_UNPROJECT_MAX_PIXELS
MAX_WORKGROUPS = 2 ** 24 - 1                                                 # LRT_UNPROJECT_MAX_WORKGROUPS: F * ceil(H W / BLOCK)
COUNT_NAMES = ("pixels", "invalid", "masked", "out_of_range", "points")
KEEP, INVALID, MASKED, OUT_OF_RANGE = 0, 1, 2, 3                             # the classes of lrt_unproject_math.h
FLT_MAX = float(np.finfo(np.float32).max)

_lib = None


class UnprojectError(RuntimeError):
    pass


class PointClouds(SimpleNamespace):
    """points (cap, 4) float32, pixel (cap,) int32, offsets (F + 1,) int64, counts (F, 5) int64 (COUNT_NAMES; (5,) without a frame axis).  The
    twin adds cls (F, H, W) uint8: every pixel's class."""

    def __iter__(self):
        return iter((self.points, self.pixel, self.offsets, self.counts))

    def trim(self):
        """[namespace(points (n_f, 4), pixel (n_f,))] per frame -- views; one namespace without a frame axis.  Reads ``offsets``: a host wait."""
        off = self.offsets.cpu().tolist()
        out = [SimpleNamespace(points=self.points[a:b], pixel=self.pixel[a:b]) for a, b in zip(off[:-1], off[1:])]
        return out[0] if self.counts.dim() == 1 else out


def load():
    """Load liblrt_unproject.so (after torch, so that both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise UnprojectError(f"{LIB_PATH} is missing: build it with `python -m lidar_rt_amd.build` (hipcc --offload-arch=gfx950). "
                             "points_from_range_images has no fall-back on a HIP device.")
    lib = C.CDLL(LIB_PATH)
    lib.lrt_unproject_abi_version.restype = C.c_int
    lib.lrt_unproject_last_error.restype = C.c_char_p
    lib.lrt_unproject_work_bytes.restype = C.c_longlong
    lib.lrt_unproject_work_bytes.argtypes = [C.c_longlong, C.c_int, C.c_int]
    lib.lrt_unproject_points.restype = C.c_int
    lib.lrt_unproject_points.argtypes = [C.c_int, C.c_longlong, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_double, C.c_void_p, C.c_int, C.c_double, C.c_double] \
        + [C.c_void_p] * 5 + [C.c_longlong, C.c_void_p]
    if lib.lrt_unproject_abi_version() != ABI_VERSION:
        raise UnprojectError("liblrt_unproject.so ABI version mismatch; rebuild with `python -m lidar_rt_amd.build --force`")
    _lib = lib
    return lib


# ---- the arguments, checked on the host ----------------------------------------------------------------------------------------------------------------

def _shape_of(x):
    return tuple(x.shape) if hasattr(x, "shape") else None


def _arguments(depth, rays_o, rays_d, intensity, keep, raydrop, raydrop_ratio, world2out, min_depth, max_depth):
    """Everything that does not read an image: (batched, F, H, W, T float64 (F, 3, 4) / (F, W, 3, 4) or None, ratio, min_depth, max_depth)."""
    fn = "points_from_range_images"
    sh = _shape_of(depth)
    if sh is None or len(sh) not in (2, 3):
        raise UnprojectError(f"{fn}: depth must be (F, H, W) or (H, W) (it is {sh})")
    batched = len(sh) == 3
    F, H, W = (sh if batched else (1,) + sh)
    if F < 1 or H < 1 or W < 1:
        raise UnprojectError(f"{fn}: {F} frames of {H} x {W} pixels (each at least 1)")
    if F * H * W > MAX_PIXELS:
        raise UnprojectError(f"{fn}: {F} frames of {H} x {W} pixels, the row index is int32 (F H W at most {MAX_PIXELS})")
    if F * ((H * W + BLOCK - 1) // BLOCK) > MAX_WORKGROUPS:
        raise UnprojectError(f"{fn}: {F} frames of {H} x {W} pixels are {F * ((H * W + BLOCK - 1) // BLOCK)} workgroups of {BLOCK} pixels of one frame "
                             f"(at most {MAX_WORKGROUPS}: one launch)")
    for name, x, want in (("rays_o", rays_o, sh + (3,)), ("rays_d", rays_d, sh + (3,)), ("intensity", intensity, sh), ("keep", keep, sh), ("raydrop", raydrop, sh)):
        if x is None and name in ("intensity", "keep", "raydrop"):
            continue
        if _shape_of(x) != want:
            raise UnprojectError(f"{fn}: {name} must be {want} (it is {_shape_of(x)})")
    T = None
    if world2out is not None:
        if torch.is_tensor(world2out):
            if world2out.device.type != "cpu":
                raise UnprojectError(f"{fn}: world2out is host data (a numpy array or a CPU tensor), it is on {world2out.device}")
            world2out = world2out.detach().numpy()
        try:
            T = np.asarray(world2out, dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise UnprojectError(f"{fn}: world2out is not numeric: {e}") from None
        if not batched and T.ndim in (2, 3):
            T = T[None]
        if not ((T.ndim == 3 and T.shape[0] == F or T.ndim == 4 and T.shape[:2] == (F, W)) and T.shape[-2] in (3, 4) and T.shape[-1] == 4):
            raise UnprojectError(f"{fn}: world2out must be ({F}, 3|4, 4), one transform per frame, or ({F}, {W}, 3|4, 4), one per column (it is {tuple(T.shape)})")
        T = np.ascontiguousarray(T[..., :3, :])
    ratio = float(raydrop_ratio)
    if raydrop is not None and ratio != ratio:
        raise UnprojectError(f"{fn}: a NaN raydrop_ratio")
    min_depth, max_depth = float(min_depth), float(max_depth)
    if not (0.0 <= min_depth < max_depth <= FLT_MAX):
        raise UnprojectError(f"{fn}: depths ({min_depth}, {max_depth}] (0 <= min < max <= FLT_MAX)")
    return batched, int(F), int(H), int(W), T, ratio, min_depth, max_depth


# ---- the twin ------------------------------------------------------------------------------------------------------------------------------------------

def _np(x, dtype):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x, dtype)


def _twin(r, o, d, it, keep, drop, ratio, T, min_depth, max_depth, F, H, W):
    """numpy.  r (F, H, W) float32, o and d (F, H, W, 3) float32.  The operations and their order are those of lrt_unproject_math.h."""
    with np.errstate(all="ignore"):
        finite = np.isfinite(r) & np.isfinite(o).all(-1) & np.isfinite(d).all(-1)
        masked = np.zeros(r.shape, bool)
        if keep is not None:
            masked |= keep == 0
        if drop is not None:
            masked |= ~(drop < np.float32(ratio))
        rd = r.astype(np.float64)
        in_range = (rd > min_depth) & (rd <= max_depth)
        cls = np.full(r.shape, KEEP, np.uint8)
        cls[~in_range] = OUT_OF_RANGE
        cls[masked] = MASKED
        cls[~finite] = INVALID
        kept = cls == KEEP
        if T is None:
            m = d * r[..., None]                                             # float32: the product rounded ...
            p = o + m                                                        # ... then the sum
        else:
            m = d.astype(np.float64) * rd[..., None]
            q = o.astype(np.float64) + m
            x, y, z = q[..., 0], q[..., 1], q[..., 2]
            R = T[:, None, None] if T.ndim == 3 else T[:, None]              # (F, 1, 1, 3, 4) / (F, 1, W, 3, 4)
            p = np.stack([R[..., k, 0] * x + R[..., k, 1] * y + R[..., k, 2] * z + R[..., k, 3] for k in range(3)], -1).astype(np.float32)
    flat = kept.reshape(-1)
    n_f = kept.reshape(F, -1).sum(1).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(n_f)]).astype(np.int64)
    cap = F * H * W
    points = np.zeros((cap, 4), np.float32)
    pixel = np.zeros(cap, np.int32)
    n = int(offsets[-1])
    points[:n, :3] = p.reshape(-1, 3)[flat]
    if it is not None:
        points[:n, 3] = it.reshape(-1)[flat]
    pixel[:n] = (np.nonzero(flat)[0] % (H * W)).astype(np.int32)
    counts = np.zeros((F, N_COUNTS), np.int64)
    counts[:, 0] = H * W
    for c, k in ((1, INVALID), (2, MASKED), (3, OUT_OF_RANGE), (4, KEEP)):
        counts[:, c] = (cls == k).reshape(F, -1).sum(1)
    return points, pixel, offsets, counts, cls


def points_from_range_images_reference(depth, rays_o, rays_d, intensity=None, keep=None, raydrop=None, raydrop_ratio=0.4, world2out=None,
                                       min_depth=0.0, max_depth=FLT_MAX) -> PointClouds:
    """The numpy twin (see the module text).  Tensors on any device or numpy arrays; the results are CPU tensors, rows from ``offsets[-1]`` on
    are zero."""
    batched, F, H, W, T, ratio, min_depth, max_depth = _arguments(depth, rays_o, rays_d, intensity, keep, raydrop, raydrop_ratio, world2out, min_depth, max_depth)
    sh = (F, H, W)
    r = _np(depth, np.float32).reshape(sh)
    o, d = _np(rays_o, np.float32).reshape(sh + (3,)), _np(rays_d, np.float32).reshape(sh + (3,))
    it = None if intensity is None else _np(intensity, np.float32).reshape(sh)
    kp = None if keep is None else _np(keep, np.uint8).reshape(sh)
    dr = None if raydrop is None else _np(raydrop, np.float32).reshape(sh)
    points, pixel, offsets, counts, cls = _twin(r, o, d, it, kp, dr, ratio, T, min_depth, max_depth, F, H, W)
    return PointClouds(points=torch.from_numpy(points), pixel=torch.from_numpy(pixel), offsets=torch.from_numpy(offsets),
                       counts=torch.from_numpy(counts if batched else counts[0]), cls=torch.from_numpy(cls if batched else cls[0]))


# ---- the operator ----------------------------------------------------------------------------------------------------------------------------------------

def work_bytes(F: int, H: int, W: int) -> int:
    """Bytes of the workspace of one call: the per-workgroup counts and bases and the per-frame running totals."""
    n = int(load().lrt_unproject_work_bytes(int(F), int(H), int(W)))
    if n < 0:
        raise UnprojectError(f"points_from_range_images: {F} frames of {H} x {W} pixels (each at least 1, F H W at most {MAX_PIXELS}, "
                             f"F ceil(H W / {BLOCK}) at most {MAX_WORKGROUPS})")
    return n


def _upload(a: np.ndarray, dev) -> torch.Tensor:
    """A small host array on the device without a host wait: through pinned memory, which the allocator keeps until the copy has run."""
    return torch.from_numpy(a).pin_memory().to(dev, non_blocking=True)


@torch.no_grad()
def points_from_range_images(depth, rays_o, rays_d, intensity=None, keep=None, raydrop=None, raydrop_ratio=0.4, world2out=None, min_depth=0.0,
                             max_depth=FLT_MAX, workspace=None) -> PointClouds:
    """F range images into F point clouds (see the module text).  The inputs are not changed.  ``workspace``: a uint8 tensor on the images'
    device of at least ``work_bytes(F, H, W)`` bytes to use instead of a fresh one; its contents do not matter."""
    fn = "points_from_range_images"
    given = [("depth", depth), ("rays_o", rays_o), ("rays_d", rays_d), ("intensity", intensity), ("keep", keep), ("raydrop", raydrop)]
    for name, x in given:
        if x is not None and not torch.is_tensor(x):
            raise UnprojectError(f"{fn}: {name} must be a tensor (it is {type(x).__name__}); numpy arrays go to points_from_range_images_reference")
    batched, F, H, W, T, ratio, min_depth, max_depth = _arguments(depth, rays_o, rays_d, intensity, keep, raydrop, raydrop_ratio, world2out, min_depth, max_depth)
    dev = depth.device
    for name, x in given:
        if x is not None and x.device != dev:
            raise UnprojectError(f"{fn}: {name} is on {x.device}, depth on {dev}")
    if dev.type != "cuda":
        if workspace is not None:
            raise UnprojectError(f"{fn}: a workspace with images on {dev}")
        r = points_from_range_images_reference(depth, rays_o, rays_d, intensity, keep, raydrop, raydrop_ratio, world2out, min_depth, max_depth)
        return PointClouds(points=r.points, pixel=r.pixel, offsets=r.offsets, counts=r.counts)
    lib = load()
    for name, x in given:
        if x is None:
            continue
        ok = (torch.bool, torch.uint8) if name == "keep" else (torch.float32,)
        if x.dtype not in ok or not x.is_contiguous():
            raise UnprojectError(f"lrt_unproject: {name} must be a contiguous {' or '.join(str(t).replace('torch.', '') for t in ok)} tensor (it is {x.dtype}, "
                                 f"{'contiguous' if x.is_contiguous() else 'not contiguous'}); there is no fall-back to PyTorch on a HIP device")
    nbytes = work_bytes(F, H, W)
    if workspace is not None:
        if not (torch.is_tensor(workspace) and workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.device == dev
                and workspace.numel() >= nbytes and workspace.data_ptr() % 256 == 0):
            raise UnprojectError(f"lrt_unproject: the workspace must be a contiguous uint8 tensor of at least {nbytes} bytes on {dev}, 256-byte aligned")
        ws = workspace
    else:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)                # the caching allocator's blocks are 512-byte aligned
    kp = None if keep is None else keep.detach().view(torch.uint8)
    d_T = None if T is None else _upload(T, dev)
    cap = F * H * W
    points = torch.empty((cap, 4), dtype=torch.float32, device=dev)
    pixel = torch.empty((cap,), dtype=torch.int32, device=dev)
    offsets = torch.empty((F + 1,), dtype=torch.int64, device=dev)
    counts = torch.empty((F, N_COUNTS), dtype=torch.int64, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        rc = lib.lrt_unproject_points(dev.index, F, H, W, depth.data_ptr(), rays_o.data_ptr(), rays_d.data_ptr(), ptr(intensity), ptr(kp), ptr(raydrop), ratio,
                                      ptr(d_T), int(T is not None and T.ndim == 4), min_depth, max_depth, points.data_ptr(), pixel.data_ptr(),
                                      offsets.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise UnprojectError(f"lrt_unproject_points failed ({rc}): {lib.lrt_unproject_last_error().decode()}")
    return PointClouds(points=points, pixel=pixel, offsets=offsets, counts=counts if batched else counts[0])
