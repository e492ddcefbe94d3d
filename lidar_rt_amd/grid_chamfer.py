"""The Chamfer term of the training loss on the range-image grid (``training.training_step`` with ``opt.grid_chamfer``).

Both clouds of the term are ``o + d * range`` on the same (H, W) ray grid: cloud A the pixels of ``mask_a`` at ``range_a`` (the prediction),
cloud B those of ``mask_b`` at ``range_b`` (the ground truth).  With dist_a the squared distance of each point of A to its nearest point of B
and dist_b the other way round,

    loss = weight * 0.5 * (mean dist_a + mean dist_b)          (means over the valid pixels; 0 if either cloud is empty)

    loss, mean_a, mean_b = grid_chamfer_torch(rays_o, rays_d, range_a, range_b, mask_a, mask_b=None, weight=1.0)
    loss, mean_a, mean_b = grid_chamfer(rays_o, rays_d, range_a, range_b, mask_a, mask_b=None, weight=1.0)

* ``grid_chamfer_torch``: brute force in plain PyTorch, any float dtype, any device, differentiable by autograd.  It is the yardstick of the
  HIP operator and what runs where that one cannot (CPU tensors).
* ``grid_chamfer``: the same numbers from ``csrc/liblrt_gridcd.so`` (``include/lrt_gridcd.h``): an exact tiled search over the image -- no sort,
  no tree -- returning the same (distance, index) bits as ``chamfer3D.chamfer_3DDist`` on the torch-formed points, and a backward without float
  atomics (bit-reproducible).  ``loss`` is differentiable w.r.t. ``range_a`` and, where they require it, ``rays_o`` / ``rays_d`` (both clouds
  counted); the means are returned detached.  HIP float32 tensors only -- a missing library is an error, there is no quiet fall-back.
* ``grid_chamfer_nearest``: the operator's per-pixel outputs ``(dist_a, dist_b, idx_a, idx_b)`` (invalid pixels: 0 and -1), no gradient.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LRT_GRIDCD_LIB") or os.path.join(HERE, "csrc", "liblrt_gridcd.so")
EXPORTS = ("lrt_gridcd_abi_version", "lrt_gridcd_last_error", "lrt_gridcd_work_bytes", "lrt_gridcd_forward", "lrt_gridcd_backward")   # include/lrt_gridcd.h
ABI_VERSION = 1

_lib = None


class GridChamferError(RuntimeError):
    pass


def load():
    """Load liblrt_gridcd.so (after torch, so that both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GridChamferError(f"{LIB_PATH} is missing: build it with `python -m lidar_rt_amd.build` (hipcc --offload-arch=gfx950). "
                               "grid_chamfer has no fall-back; grid_chamfer_torch is the PyTorch expression.")
    lib = C.CDLL(LIB_PATH)
    vp, ci = C.c_void_p, C.c_int
    lib.lrt_gridcd_abi_version.restype = ci
    lib.lrt_gridcd_last_error.restype = C.c_char_p
    lib.lrt_gridcd_work_bytes.restype = C.c_size_t; lib.lrt_gridcd_work_bytes.argtypes = [ci, ci]
    lib.lrt_gridcd_forward.restype = ci
    lib.lrt_gridcd_forward.argtypes = [ci, ci, ci, vp, vp, vp, vp, vp, vp, C.c_double, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    lib.lrt_gridcd_backward.restype = ci
    lib.lrt_gridcd_backward.argtypes = [ci, ci, ci, vp, vp, vp, vp, vp, vp, C.c_double, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    if lib.lrt_gridcd_abi_version() != ABI_VERSION:
        raise GridChamferError("liblrt_gridcd.so ABI version mismatch; rebuild with `python -m lidar_rt_amd.build --force`")
    _lib = lib
    return lib


def _check(rc: int, what: str):
    if rc != 0:
        raise GridChamferError(f"{what} failed ({rc}): {load().lrt_gridcd_last_error().decode()}")


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------------------

def _nearest_torch(q: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """Index of the nearest row of ``c`` for each row of ``q`` (squared distances summed x, y, z; the first of equal minima), in chunks of
    about 4 M pairs so that two clouds of a 66 x 1030 image fit in memory."""
    out = torch.empty(q.shape[0], dtype=torch.long, device=q.device)
    step = max(1, (1 << 22) // max(1, c.shape[0]))
    with torch.no_grad():
        for s in range(0, q.shape[0], step):
            d = c[None, :, :] - q[s:s + step, None, :]
            out[s:s + step] = (d * d).sum(-1).argmin(1)
    return out


def grid_chamfer_torch(rays_o, rays_d, range_a, range_b, mask_a, mask_b=None, weight: float = 1.0):
    """(loss, mean dist_a, mean dist_b) by brute force, in the dtype of ``range_a``; every tensor input may require a gradient."""
    mask_b = mask_a if mask_b is None else mask_b
    dt = range_a.dtype
    o, d = rays_o.to(dt), rays_d.to(dt)
    ia = torch.nonzero(mask_a.reshape(-1) != 0).squeeze(1)
    ib = torch.nonzero(mask_b.reshape(-1) != 0).squeeze(1)
    a = (o + d * range_a.reshape(*d.shape[:2], 1)).reshape(-1, 3).index_select(0, ia)
    b = (o + d * range_b.to(dt).reshape(*d.shape[:2], 1)).reshape(-1, 3).index_select(0, ib)
    if a.shape[0] == 0 or b.shape[0] == 0:
        z = (a.sum() + b.sum()) * 0.0                         # an exact 0 that still hangs on the inputs: their gradients are zeros, not None
        return z, z.detach(), z.detach()
    nn_a, nn_b = _nearest_torch(a.detach(), b.detach()), _nearest_torch(b.detach(), a.detach())
    mean_a = ((a - b.index_select(0, nn_a)) ** 2).sum(-1).mean()
    mean_b = ((b - a.index_select(0, nn_b)) ** 2).sum(-1).mean()
    return weight * 0.5 * (mean_a + mean_b), mean_a.detach(), mean_b.detach()


# ---- the HIP operator ---------------------------------------------------------------------------------------------------------------------------

_WORK = {}          # (H, W, device index) -> workspace (scratch only: nothing lives there between two calls)


def _workspace(H: int, W: int, dev: torch.device) -> torch.Tensor:
    key = (H, W, dev.index)
    w = _WORK.get(key)
    if w is None:
        nb = int(load().lrt_gridcd_work_bytes(H, W))
        if nb == 0:
            raise GridChamferError(f"grid_chamfer: unsupported image size {H} x {W}")
        if len(_WORK) > 16:
            _WORK.clear()
        w = _WORK[key] = torch.empty((nb + 7) // 8, dtype=torch.float64, device=dev)
    return w


def _mask8(mask: torch.Tensor) -> torch.Tensor:
    if mask.dtype == torch.bool:
        return mask.contiguous().view(torch.uint8)              # the same bytes: no launch
    if mask.dtype == torch.uint8:
        return mask.contiguous()
    return (mask != 0).view(torch.uint8)


def _prepare(rays_o, rays_d, range_a, range_b, mask_a, mask_b):
    if not (isinstance(range_a, torch.Tensor) and range_a.is_cuda and range_a.dtype == torch.float32 and range_a.dim() == 2):
        raise GridChamferError("grid_chamfer: range_a must be a float32 HIP tensor (H, W); grid_chamfer_torch takes everything else")
    H, W = range_a.shape
    dev = range_a.device
    for name, t in (("rays_o", rays_o), ("rays_d", rays_d)):
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.float32 or tuple(t.shape) != (H, W, 3):
            raise GridChamferError(f"grid_chamfer: {name} must be a float32 ({H}, {W}, 3) tensor on {dev}")
    mask_b = mask_a if mask_b is None else mask_b
    for name, t in (("range_b", range_b), ("mask_a", mask_a), ("mask_b", mask_b)):
        if not isinstance(t, torch.Tensor) or t.device != dev or tuple(t.shape) != (H, W):
            raise GridChamferError(f"grid_chamfer: {name} must be a ({H}, {W}) tensor on {dev}")
    m_a = _mask8(mask_a)
    m_b = m_a if mask_b is mask_a else _mask8(mask_b)
    return rays_o, rays_d, range_a, range_b.detach().to(torch.float32).contiguous(), m_a, m_b


def _launch_forward(o, d, ra, rb, ma, mb, weight):
    H, W = ra.shape
    dev = ra.device
    new = lambda dtype: torch.empty((H, W), dtype=dtype, device=dev)
    out = torch.empty(4, dtype=torch.float32, device=dev)
    dist_a, dist_b, idx_a, idx_b = new(torch.float32), new(torch.float32), new(torch.int32), new(torch.int32)
    work = _workspace(H, W, dev)
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _check(load().lrt_gridcd_forward(dev.index, H, W, o.data_ptr(), d.data_ptr(), ra.data_ptr(), ma.data_ptr(), rb.data_ptr(), mb.data_ptr(),
                                         float(weight), out.data_ptr(), dist_a.data_ptr(), dist_b.data_ptr(), idx_a.data_ptr(), idx_b.data_ptr(),
                                         work.data_ptr(), work.numel() * 8, stream), "lrt_gridcd_forward")
    return out, dist_a, dist_b, idx_a, idx_b


class _GridChamfer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rays_o, rays_d, range_a, range_b, mask_a8, mask_b8, weight):
        o, d, ra = rays_o.contiguous(), rays_d.contiguous(), range_a.contiguous()
        out, _, _, idx_a, idx_b = _launch_forward(o, d, ra, range_b, mask_a8, mask_b8, weight)
        ctx.weight = float(weight)
        ctx.save_for_backward(o, d, ra, range_b, mask_a8, mask_b8, idx_a, idx_b)
        ctx.mark_non_differentiable(out)
        return out[0], out

    @staticmethod
    def backward(ctx, d_loss, _d_out):
        o, d, ra, rb, ma, mb, idx_a, idx_b = ctx.saved_tensors
        H, W = ra.shape
        dev = ra.device
        rays = bool(ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        d_loss = d_loss.to(torch.float32).reshape(1).contiguous()
        d_ra = torch.empty_like(ra)                              # every element is written by the kernels: no clearing
        d_o = torch.empty_like(o) if rays else None
        d_d = torch.empty_like(d) if rays else None
        work = _workspace(H, W, dev)
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _check(load().lrt_gridcd_backward(dev.index, H, W, o.data_ptr(), d.data_ptr(), ra.data_ptr(), ma.data_ptr(), rb.data_ptr(), mb.data_ptr(),
                                              ctx.weight, idx_a.data_ptr(), idx_b.data_ptr(), d_loss.data_ptr(), d_ra.data_ptr(),
                                              d_o.data_ptr() if rays else None, d_d.data_ptr() if rays else None,
                                              work.data_ptr(), work.numel() * 8, stream), "lrt_gridcd_backward")
        return (d_o if ctx.needs_input_grad[0] else None, d_d if ctx.needs_input_grad[1] else None,
                d_ra if ctx.needs_input_grad[2] else None, None, None, None, None)


def grid_chamfer(rays_o, rays_d, range_a, range_b, mask_a, mask_b: Optional[torch.Tensor] = None, weight: float = 1.0):
    """(loss, mean dist_a, mean dist_b) from the HIP operator; ``loss`` carries the gradient w.r.t. ``range_a`` (and the rays where they require it)."""
    o, d, ra, rb, ma, mb = _prepare(rays_o, rays_d, range_a, range_b, mask_a, mask_b)
    loss, out = _GridChamfer.apply(o, d, ra, rb, ma, mb, float(weight))
    return loss, out[1], out[2]


@torch.no_grad()
def grid_chamfer_nearest(rays_o, rays_d, range_a, range_b, mask_a, mask_b: Optional[torch.Tensor] = None):
    """(dist_a, dist_b, idx_a, idx_b), each (H, W): squared distance to and linear pixel index of the nearest valid pixel of the other cloud."""
    o, d, ra, rb, ma, mb = _prepare(rays_o, rays_d, range_a, range_b, mask_a, mask_b)
    return _launch_forward(o.contiguous(), d.contiguous(), ra.detach().contiguous(), rb, ma, mb, 1.0)[1:]
