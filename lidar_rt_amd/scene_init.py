"""Scene initialisation from the range images of a sequence: what the reference does with Open3D on the CPU before its loop starts
(lib/dataloader/gs_loader.py:82-215), restated on the ray grid.

    normals, nbr                         = estimate_normals(rays_o, rays_d, depth, mask, k=6)
    label, local_points, local_normals   = assign_to_boxes(points, normals, mask, poses, sizes, present)
    points, intensity, normals, count    = voxel_downsample(points, intensity, normals, voxel_size)
    clouds                               = init_clouds(seq, k=6, voxel_size=0.15, use_voxel_init=True, obj_pt_num=2000, seed=0)

* ``estimate_normals``: per valid pixel the ``k`` nearest valid pixels of the frame (the pixel itself included, ties to the lower pixel index:
  exactly a brute-force scan) and the unit normal of their covariance, turned to face the sensor; ``(0, 0, 1)`` for fewer than 3 listed points
  or a covariance of rank < 2.  ``nbr`` is (H, W, 8) int32, -1 where there is no entry.
* ``assign_to_boxes``: -1 (invalid pixel), 0 (background) or ``a + 1`` for the FIRST present actor whose box strictly contains the point, and the
  point / normal in that actor's frame (the inputs unchanged elsewhere).
* ``voxel_downsample``: Open3D's ``voxel_down_sample`` (origin = minimum - voxel_size / 2, one row per occupied voxel, means of point, intensity
  and normal -- the last not renormalised) with a DEFINED row order: ascending 63-bit voxel key, 21 bits per axis.  A cloud that needs more
  bits raises ``SceneInitError``.

Each of the three runs from ``csrc/liblrt_init.so`` (``include/lrt_init.h``) on HIP float32 tensors -- a missing library is an error, there is
no quiet fall-back -- and has a ``*_reference`` twin in float64 numpy / torch that runs on any device: the yardstick of the tests, and what CPU
tensors get.  ``init_clouds`` builds the ``seq.init`` layout (``points``, ``intensity``, ``normals`` per asset) from the training frames.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, Optional

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LRT_INIT_LIB") or os.path.join(HERE, "csrc", "liblrt_init.so")
EXPORTS = ("lrt_init_abi_version", "lrt_init_last_error", "lrt_init_normals_work_bytes", "lrt_init_voxel_work_bytes", "lrt_init_normals",
           "lrt_init_assign", "lrt_init_voxel_keys", "lrt_init_voxel_mean")                                   # include/lrt_init.h
ABI_VERSION = 1
KMAX = 8
KEY_BITS = 21
KEY_RANGE = 1            # info[1] of lrt_init_voxel_keys
RANK_TOL = 1e-14         # the twin's rank rule: lambda_1 <= RANK_TOL * lambda_2 is rank < 2 (lrt_init_math.h tests the same product of the scaled matrix)

_lib = None


class SceneInitError(RuntimeError):
    pass


def load():
    """Load liblrt_init.so (after torch, so that both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SceneInitError(f"{LIB_PATH} is missing: build it with `python -m lidar_rt_amd.build` (hipcc --offload-arch=gfx950). "
                             "scene_init has no fall-back on HIP tensors; the *_reference functions are the numpy / torch expressions.")
    lib = C.CDLL(LIB_PATH)
    vp, ci, ll = C.c_void_p, C.c_int, C.c_longlong
    lib.lrt_init_abi_version.restype = ci
    lib.lrt_init_last_error.restype = C.c_char_p
    lib.lrt_init_normals_work_bytes.restype = C.c_size_t; lib.lrt_init_normals_work_bytes.argtypes = [ci, ci]
    lib.lrt_init_voxel_work_bytes.restype = C.c_size_t; lib.lrt_init_voxel_work_bytes.argtypes = [ll]
    lib.lrt_init_normals.restype = ci
    lib.lrt_init_normals.argtypes = [ci, ci, ci, vp, vp, vp, vp, ci, vp, vp, vp, C.c_size_t, vp]
    lib.lrt_init_assign.restype = ci
    lib.lrt_init_assign.argtypes = [ci, ll, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp]
    lib.lrt_init_voxel_keys.restype = ci
    lib.lrt_init_voxel_keys.argtypes = [ci, ll, vp, C.c_double, vp, vp, vp, C.c_size_t, vp]
    lib.lrt_init_voxel_mean.restype = ci
    lib.lrt_init_voxel_mean.argtypes = [ci, ll, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    if lib.lrt_init_abi_version() != ABI_VERSION:
        raise SceneInitError("liblrt_init.so ABI version mismatch; rebuild with `python -m lidar_rt_amd.build --force`")
    _lib = lib
    return lib


def _check(rc: int, what: str):
    if rc != 0:
        raise SceneInitError(f"{what} failed ({rc}): {load().lrt_init_last_error().decode()}")


def _mask8(mask: torch.Tensor) -> torch.Tensor:
    if mask.dtype == torch.bool:
        return mask.contiguous().view(torch.uint8)
    if mask.dtype == torch.uint8:
        return mask.contiguous()
    return (mask != 0).view(torch.uint8)


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _f32(name: str, t, dev, shape) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
        raise SceneInitError(f"scene_init: {name} must be a float32 {tuple(shape)} tensor on {dev}")
    return t.detach().contiguous()


# ---- the HIP operators ----------------------------------------------------------------------------------------------------------------------------

@torch.no_grad()
def estimate_normals(rays_o, rays_d, depth, mask, k: int = 6):
    """(normals (H, W, 3) float32, nbr (H, W, 8) int32) of one frame; see the module docstring.  CPU tensors go to the reference twin."""
    if isinstance(depth, torch.Tensor) and not depth.is_cuda:
        return estimate_normals_reference(rays_o, rays_d, depth, mask, k)
    if not (isinstance(depth, torch.Tensor) and depth.dtype == torch.float32 and depth.dim() == 2):
        raise SceneInitError("estimate_normals: depth must be a float32 (H, W) tensor")
    if not 3 <= int(k) <= KMAX:
        raise SceneInitError(f"estimate_normals: k = {k}, need 3 <= k <= {KMAX}")
    H, W = depth.shape
    dev = depth.device
    o, d, r = _f32("rays_o", rays_o, dev, (H, W, 3)), _f32("rays_d", rays_d, dev, (H, W, 3)), depth.detach().contiguous()
    if not isinstance(mask, torch.Tensor) or mask.device != dev or tuple(mask.shape) != (H, W):
        raise SceneInitError(f"estimate_normals: mask must be a ({H}, {W}) tensor on {dev}")
    m = _mask8(mask)
    lib = load()
    nb = int(lib.lrt_init_normals_work_bytes(H, W))
    if nb == 0:
        raise SceneInitError(f"estimate_normals: unsupported image size {H} x {W}")
    work = torch.empty((nb + 7) // 8, dtype=torch.float64, device=dev)
    nbr = torch.empty((H, W, KMAX), dtype=torch.int32, device=dev)
    normals = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _check(lib.lrt_init_normals(dev.index, H, W, o.data_ptr(), d.data_ptr(), r.data_ptr(), m.data_ptr(), int(k), nbr.data_ptr(), normals.data_ptr(),
                                    work.data_ptr(), work.numel() * 8, _stream(dev)), "lrt_init_normals")
    return normals, nbr


@torch.no_grad()
def assign_to_boxes(points, normals, mask, poses, sizes, present):
    """(label int32, local_points, local_normals) with the shapes of ``mask`` / ``points``.  poses (A, 7) [t, q_wxyz], sizes (A, 3), present (A)."""
    if isinstance(points, torch.Tensor) and not points.is_cuda:
        return assign_to_boxes_reference(points, normals, mask, poses, sizes, present)
    if not (isinstance(points, torch.Tensor) and points.dtype == torch.float32 and points.shape[-1:] == (3,)):
        raise SceneInitError("assign_to_boxes: points must be a float32 (..., 3) tensor")
    dev, shape = points.device, tuple(points.shape[:-1])
    p, nrm = points.detach().contiguous(), _f32("normals", normals, dev, points.shape)
    if not isinstance(mask, torch.Tensor) or mask.device != dev or tuple(mask.shape) != shape:
        raise SceneInitError(f"assign_to_boxes: mask must be a {shape} tensor on {dev}")
    m = _mask8(mask)
    n = m.numel()
    A = 0 if poses is None else int(poses.shape[0])
    label = torch.empty(shape, dtype=torch.int32, device=dev)
    lp, ln = torch.empty_like(p), torch.empty_like(p)
    if n == 0:
        return label, lp, ln
    if A:
        ps, sz = _f32("poses", poses, dev, (A, 7)), _f32("sizes", sizes, dev, (A, 3))
        pr = _mask8(present.to(dev).reshape(A))
    with torch.cuda.device(dev):
        _check(load().lrt_init_assign(dev.index, n, p.data_ptr(), nrm.data_ptr(), m.data_ptr(), A, ps.data_ptr() if A else None, sz.data_ptr() if A else None,
                                      pr.data_ptr() if A else None, label.data_ptr(), lp.data_ptr(), ln.data_ptr(), _stream(dev)), "lrt_init_assign")
    return label, lp, ln


@torch.no_grad()
def voxel_downsample(points, intensity, normals, voxel_size: float):
    """(points (M, 3), intensity (M), normals (M, 3), count (M) int32), rows in ascending voxel key order.  The key sort is ``torch.sort(stable=True)``;
    M and the key-range status are read from the device once, after the last launch (the one host wait of the initialisation)."""
    if isinstance(points, torch.Tensor) and not points.is_cuda:
        return voxel_downsample_reference(points, intensity, normals, voxel_size)
    if not (isinstance(points, torch.Tensor) and points.dtype == torch.float32 and points.dim() == 2 and points.shape[1] == 3):
        raise SceneInitError("voxel_downsample: points must be a float32 (N, 3) tensor")
    if not (float(voxel_size) > 0.0 and math.isfinite(float(voxel_size))):
        raise SceneInitError("voxel_downsample: voxel_size must be positive and finite")
    dev, N = points.device, points.shape[0]
    p, it, nrm = points.detach().contiguous(), _f32("intensity", intensity, dev, (N,)), _f32("normals", normals, dev, (N, 3))
    if N == 0:
        return p, it, nrm, torch.zeros(0, dtype=torch.int32, device=dev)
    lib = load()
    nb = int(lib.lrt_init_voxel_work_bytes(N))
    if nb == 0:
        raise SceneInitError(f"voxel_downsample: unsupported point count {N}")
    work = torch.empty((nb + 7) // 8, dtype=torch.float64, device=dev)
    keys = torch.empty(N, dtype=torch.int64, device=dev)
    info = torch.empty(2, dtype=torch.int32, device=dev)
    o_p, o_i, o_n = torch.empty_like(p), torch.empty_like(it), torch.empty_like(nrm)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        st = _stream(dev)
        _check(lib.lrt_init_voxel_keys(dev.index, N, p.data_ptr(), float(voxel_size), keys.data_ptr(), info.data_ptr(), work.data_ptr(), work.numel() * 8, st),
               "lrt_init_voxel_keys")
        skeys, perm = torch.sort(keys, stable=True)
        perm = perm.to(torch.int32)
        _check(lib.lrt_init_voxel_mean(dev.index, N, skeys.data_ptr(), perm.data_ptr(), p.data_ptr(), it.data_ptr(), nrm.data_ptr(), o_p.data_ptr(), o_i.data_ptr(),
                                       o_n.data_ptr(), count.data_ptr(), info.data_ptr(), work.data_ptr(), work.numel() * 8, st), "lrt_init_voxel_mean")
    M, status = (int(x) for x in info.tolist())
    if status & KEY_RANGE:
        raise SceneInitError(f"voxel_downsample: the cloud spans more than 2^{KEY_BITS} voxels of {voxel_size} m on an axis (or holds a non-finite point): "
                             "the 63-bit voxel key would wrap")
    return o_p[:M], o_i[:M], o_n[:M], count[:M]


# ---- the yardsticks -------------------------------------------------------------------------------------------------------------------------------

def _pair_d2(c: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    """(Q, C) float32 squared distances as the kernels form them: d = candidate - query in float32, then fma(dz, dz, fma(dy, dy, dx * dx)) -- each
    product exact in float64, one rounding to float32 per step."""
    dx, dy, dz = (c[None, :, i] - q[:, None, i] for i in range(3))
    t = (dx.double() * dx.double()).float()
    t = (dy.double() * dy.double() + t.double()).float()
    return (dz.double() * dz.double() + t.double()).float()


@torch.no_grad()
def neighbours_reference(points: torch.Tensor, mask: torch.Tensor, k: int = 6, queries: Optional[torch.Tensor] = None, pairs: int = 1 << 22) -> torch.Tensor:
    """Brute force: for each valid pixel (or each of the linear pixel indices ``queries``) the k smallest (float32 squared distance, linear pixel
    index) pairs over all valid pixels, ascending; -1 padded to 8.  points (H, W, 3) float32 -> (H, W, 8) int32, or (len(queries), 8).
    ``pairs``: query x candidate pairs per chunk (memory)."""
    pts = points.reshape(-1, 3).float()
    valid = mask.reshape(-1) != 0
    vi = torch.nonzero(valid).squeeze(1)
    HW, dev = pts.shape[0], pts.device
    qi = vi if queries is None else queries.to(dev).long()
    out = torch.full((qi.shape[0], KMAX), -1, dtype=torch.int32, device=dev)
    n = vi.shape[0]
    if n and qi.shape[0]:
        c = pts.index_select(0, vi)
        kk = min(int(k), n)
        step = max(1, int(pairs) // n)
        for s in range(0, qi.shape[0], step):
            d2 = _pair_d2(c, pts.index_select(0, qi[s:s + step]))
            key = (d2.view(torch.int32).long() << 32) | vi[None, :]          # d2 >= +0: the bit pattern orders like the value; keys are distinct
            best = torch.topk(key, kk, dim=1, largest=False, sorted=True).values
            out[s:s + step, :kk] = (best & 0xffffffff).to(torch.int32)
        if queries is not None:
            out[~valid.index_select(0, qi)] = -1
    if queries is not None:
        return out
    full = torch.full((HW, KMAX), -1, dtype=torch.int32, device=dev)
    full[vi] = out
    return full.reshape(*points.shape[:-1], KMAX)


def _face_sensor(n32: np.ndarray, o32: np.ndarray, p32: np.ndarray) -> np.ndarray:
    """The sign rule on float32 normals: n . (o - p) >= 0 in float64, x then y then z; at exactly 0 the first non-zero component is positive."""
    n, v = n32.astype(np.float64), o32.astype(np.float64) - p32.astype(np.float64)
    s = n[:, 0] * v[:, 0] + n[:, 1] * v[:, 1] + n[:, 2] * v[:, 2]
    first = np.where(n32[:, 0] != 0, n32[:, 0], np.where(n32[:, 1] != 0, n32[:, 1], n32[:, 2]))
    flip = (s < 0) | ((s == 0) & (first < 0))
    return np.where(flip[:, None], -n32, n32)


def normals_from_lists_reference(points, rays_o, mask, nbr, return_eigenvalues: bool = False):
    """Float64 ``numpy.linalg.eigh`` on the covariance of the listed float32 points: (H, W, 3) float32 normals (and the (H, W, 3) eigenvalues)."""
    shape = tuple(points.shape[:-1])
    P = points.detach().reshape(-1, 3).cpu().numpy().astype(np.float32)
    O = rays_o.detach().reshape(-1, 3).cpu().numpy().astype(np.float32)
    L = nbr.detach().reshape(-1, KMAX).cpu().numpy().astype(np.int64)
    valid = mask.detach().reshape(-1).cpu().numpy() != 0
    have = L >= 0
    cnt = have.sum(1)
    G = P[np.where(have, L, 0)].astype(np.float64)                          # (HW, 8, 3)
    w = have[..., None].astype(np.float64)
    mean = (G * w).sum(1) / np.maximum(cnt, 1)[:, None]
    D = (G - mean[:, None, :]) * w
    cov = np.einsum("nki,nkj->nij", D, D) / np.maximum(cnt, 1)[:, None, None]
    lam, vec = np.linalg.eigh(cov)
    n64 = vec[:, :, 0]
    degenerate = (cnt < 3) | ~(lam[:, 1] > RANK_TOL * lam[:, 2])
    n64 = np.where(degenerate[:, None], np.array([0.0, 0.0, 1.0]), n64)
    n32 = _face_sensor(n64.astype(np.float32), O, P)
    n32 = np.where(valid[:, None], n32, np.float32(0)).astype(np.float32)
    out = torch.as_tensor(n32.reshape(*shape, 3), device=points.device)
    if return_eigenvalues:
        return out, torch.as_tensor(np.where(valid[:, None], lam, 0.0).reshape(*shape, 3))
    return out


@torch.no_grad()
def estimate_normals_reference(rays_o, rays_d, depth, mask, k: int = 6, nbr: Optional[torch.Tensor] = None):
    """The twin of ``estimate_normals``: brute-force neighbour lists (or the given ones) and float64 eigh.  Any device."""
    if not 3 <= int(k) <= KMAX:
        raise SceneInitError(f"estimate_normals: k = {k}, need 3 <= k <= {KMAX}")
    o, d, r = rays_o.float(), rays_d.float(), depth.float()
    pts = o + d * r.reshape(*d.shape[:2], 1)                                  # float32: a rounded product, then a rounded sum
    if nbr is None:
        nbr = neighbours_reference(pts, mask, k)
    return normals_from_lists_reference(pts, o, mask, nbr), nbr


def _rotation64(q: np.ndarray) -> np.ndarray:
    q = q.astype(np.float64)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


@torch.no_grad()
def assign_to_boxes_reference(points, normals, mask, poses, sizes, present, return_margin: bool = False):
    """The twin of ``assign_to_boxes`` in float64 numpy: the reference's sequential masking (first present actor wins).  ``return_margin``: also
    the smallest distance of each valid point to a face of a present box it was tested against (the tests exclude the knife edges with it)."""
    shape, dev = tuple(points.shape[:-1]), points.device
    P = points.detach().reshape(-1, 3).cpu().numpy().astype(np.float64)
    Nn = normals.detach().reshape(-1, 3).cpu().numpy().astype(np.float64)
    valid = mask.detach().reshape(-1).cpu().numpy() != 0
    label = np.where(valid, 0, -1).astype(np.int32)
    lp, ln = P.copy(), Nn.copy()
    margin = np.full(P.shape[0], np.inf)
    A = 0 if poses is None else int(poses.shape[0])
    if A:
        ps, sz = poses.detach().cpu().numpy(), sizes.detach().cpu().numpy().astype(np.float64)
        pr = present.detach().cpu().numpy().reshape(-1) != 0
        for a in range(A):
            if not pr[a]:
                continue
            R = _rotation64(ps[a, 3:7])
            loc = (P - ps[a, :3].astype(np.float64)) @ R                      # R^T (p - t), row-wise
            free = label == 0
            margin = np.where(free, np.minimum(margin, np.abs(np.abs(loc) - 0.5 * sz[a]).min(1)), margin)
            inside = free & (np.abs(loc) < 0.5 * sz[a]).all(1)
            label[inside] = a + 1
            lp[inside] = loc[inside]
            ln[inside] = (Nn @ R)[inside]
    t = lambda a, dt: torch.as_tensor(a.astype(dt), device=dev)
    out = (t(label, np.int32).reshape(shape), t(lp, np.float32).reshape(*shape, 3), t(ln, np.float32).reshape(*shape, 3))
    return out + (torch.as_tensor(margin).reshape(shape),) if return_margin else out


def voxel_keys_reference(points, voxel_size: float) -> np.ndarray:
    """int64 voxel keys of a float32 cloud, float64 arithmetic; raises SceneInitError where an index does not fit into 21 bits."""
    P = points.detach().cpu().numpy().astype(np.float32).astype(np.float64).reshape(-1, 3)
    origin = P.min(0) - 0.5 * float(voxel_size)
    idx = np.floor((P - origin) / float(voxel_size))
    if not (np.isfinite(idx).all() and (idx >= 0).all() and (idx < (1 << KEY_BITS)).all()):
        raise SceneInitError(f"voxel_downsample: the cloud spans more than 2^{KEY_BITS} voxels of {voxel_size} m on an axis (or holds a non-finite point): "
                             "the 63-bit voxel key would wrap")
    idx = idx.astype(np.int64)
    return (idx[:, 0] << (2 * KEY_BITS)) | (idx[:, 1] << KEY_BITS) | idx[:, 2]


@torch.no_grad()
def voxel_downsample_reference(points, intensity, normals, voxel_size: float):
    """The twin of ``voxel_downsample``: float64 numpy, sums in ascending input index, one rounding."""
    if not (float(voxel_size) > 0.0 and math.isfinite(float(voxel_size))):
        raise SceneInitError("voxel_downsample: voxel_size must be positive and finite")
    dev, N = points.device, points.shape[0]
    if N == 0:
        return points.float(), intensity.float(), normals.float(), torch.zeros(0, dtype=torch.int32, device=dev)
    keys = voxel_keys_reference(points, voxel_size)
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    heads = np.flatnonzero(np.concatenate(([True], sk[1:] != sk[:-1])))
    count = np.diff(np.concatenate((heads, [N]))).astype(np.int32)
    rows = np.concatenate([points.detach().cpu().numpy().reshape(N, 3), intensity.detach().cpu().numpy().reshape(N, 1),
                           normals.detach().cpu().numpy().reshape(N, 3)], 1).astype(np.float32).astype(np.float64)[order]
    mean = (np.add.reduceat(rows, heads, axis=0) / count[:, None]).astype(np.float32)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    return t(mean[:, :3]), t(mean[:, 3]), t(mean[:, 4:7]), t(count)


# ---- the clouds of a sequence -----------------------------------------------------------------------------------------------------------------------

def frame_pose_table(boxes, frame, device):
    """(poses (A, 7) [t, q_wxyz], sizes (A, 3), present (A) uint8) of the tracking boxes at one frame; an absent box gets the identity pose."""
    A = len(boxes)
    poses = torch.zeros((A, 7), dtype=torch.float32, device=device)
    sizes = torch.zeros((A, 3), dtype=torch.float32, device=device)
    present = torch.zeros(A, dtype=torch.uint8, device=device)
    for a, tb in enumerate(boxes):
        sizes[a] = (tb.max_xyz - tb.min_xyz).float().to(device)
        poses[a, 3] = 1.0
        if frame in tb.frame:
            poses[a, :3] = tb.frame[frame][0].reshape(3).float().to(device)
            poses[a, 3:] = tb.frame[frame][1].reshape(4).float().to(device)
            present[a] = 1
    return poses, sizes, present


def scene_extent(points: torch.Tensor, factor: float = 1.0) -> float:
    """The reference's background extent: 2 |p - centre|, its 0.90 quantile, truncated to an integer, times the extent factor."""
    p = points.detach().double().cpu().numpy()
    if p.shape[0] == 0:
        return float(factor)
    ext = 2.0 * np.linalg.norm(p - p.mean(0), axis=1)
    return float(factor) * float(int(np.quantile(ext, 0.90)))


@torch.no_grad()
def init_clouds(seq, k: int = 6, voxel_size: float = 0.15, use_voxel_init: bool = True, obj_pt_num: int = 2000, seed: int = 0,
                extent_factor: float = 1.0) -> Dict[str, dict]:
    """{"background": {points, intensity, normals, extent}, "actor_00": {points, intensity, normals, real}, ...} in the layout of ``seq.init``
    from the TRAINING frames of a loaded sequence (gs_loader.py:82-215 restated):

    * per frame: normals from the k nearest returns, then the split by that frame's tracking boxes;
    * background: the label-0 returns of all frames, averaged per voxel (``use_voxel_init``) or a seeded random subset of 5 x (N / frames);
    * actors: each actor's local returns of all frames; fewer than ``obj_pt_num``: padded with seeded uniform points in its box (random unit
      normal, intensity 0.5); more: a seeded subset.  ``real`` = how many of the rows are real returns;
    * ``extent``: ``scene_extent`` of the background (used where meta.json carries none).

    Random draws come from a CPU generator seeded by ``seed``: N ranks build the same scene."""
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    rf = seq.frames
    dev = next(iter(rf.depth.values())).device
    A = len(seq.boxes)
    bg, actors = [], [[] for _ in range(A)]
    for f in seq.train_frames:
        o, d = rf.rays[f]
        depth, mask = rf.get_depth(f).float(), rf.get_mask(f)
        normals, _ = estimate_normals(o, d, depth, mask, k)
        pts = o + d * depth.reshape(*d.shape[:2], 1)
        poses, sizes, present = frame_pose_table(seq.boxes, f, dev)
        label, lp, ln = assign_to_boxes(pts, normals, mask, poses, sizes, present)
        label, lp, ln, it = label.reshape(-1), lp.reshape(-1, 3), ln.reshape(-1, 3), rf.get_intensity(f).float().reshape(-1)
        sel = torch.nonzero(label == 0).squeeze(1)
        bg.append((lp.index_select(0, sel), it.index_select(0, sel), ln.index_select(0, sel)))
        for a in range(A):
            sel = torch.nonzero(label == a + 1).squeeze(1)
            actors[a].append((lp.index_select(0, sel), it.index_select(0, sel), ln.index_select(0, sel)))
    cat = lambda rows, i, tail: torch.cat([r[i] for r in rows]) if rows else torch.zeros((0,) + tail, device=dev)
    p, it, nr = cat(bg, 0, (3,)), cat(bg, 1, ()), cat(bg, 2, (3,))
    if use_voxel_init:
        p, it, nr, _ = voxel_downsample(p, it, nr, voxel_size)
    else:
        keep = min(p.shape[0], 5 * (p.shape[0] // max(1, len(seq.train_frames))))
        sel = torch.randperm(p.shape[0], generator=g)[:keep].to(dev)
        p, it, nr = p[sel], it[sel], nr[sel]
    out = {"background": {"points": p, "intensity": it, "normals": nr, "extent": scene_extent(p, extent_factor)}}
    for a, tb in enumerate(seq.boxes):
        p, it, nr = cat(actors[a], 0, (3,)), cat(actors[a], 1, ()), cat(actors[a], 2, (3,))
        real = int(min(p.shape[0], obj_pt_num))
        if p.shape[0] < obj_pt_num:
            extra = obj_pt_num - p.shape[0]
            u = torch.rand((extra, 3), generator=g).to(dev)
            v = torch.randn((extra, 3), generator=g)
            v = (v / v.norm(dim=1, keepdim=True).clamp_min(1e-12)).to(dev)
            lo, hi = tb.min_xyz.float().to(dev), tb.max_xyz.float().to(dev)
            p, it, nr = torch.cat([p, lo + u * (hi - lo)]), torch.cat([it, torch.full((extra,), 0.5, device=dev)]), torch.cat([nr, v])
        elif p.shape[0] > obj_pt_num:
            sel = torch.randperm(p.shape[0], generator=g)[:obj_pt_num].to(dev)
            p, it, nr = p[sel], it[sel], nr[sel]
        out[f"actor_{a:02d}"] = {"points": p, "intensity": it, "normals": nr, "real": real}
    return out
