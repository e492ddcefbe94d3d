"""The per-pixel training loss of a range image (train.py:160-214 of the reference; ``training.training_step``): depth L1, intensity
L1 / L2 / DSSIM and ray-drop BCE of the tracer's raw ``(H, W, 9)`` image against a ground-truth frame.

    total, depth, intensity, raydrop, n = range_image_loss_torch(rendered, gt_depth, gt_intensity, mask, opt)
    total, depth, intensity, raydrop, n = range_image_loss(rendered, gt_depth, gt_intensity, mask, opt)

* ``range_image_loss_torch``: the expression of ``training_step`` as a function of the raw image, in plain PyTorch: any float dtype, any
  device.  It is the yardstick of the fused operator and what runs where that one cannot (CPU tensors).
* ``range_image_loss``: the same numbers from ``csrc/liblrt_loss.so`` (``include/lrt_loss.h``; two launches forward, one backward, no float
  atomics: bit-reproducible).  Only ``total`` is differentiable (w.r.t. ``rendered``); the terms and ``n`` are returned detached.
  HIP float32 tensors only -- a missing library is an error, there is no quiet fall-back.

``opt`` supplies ``lambda_depth_l1``, ``lambda_intensity_l1``, ``lambda_intensity_l2``, ``lambda_intensity_dssim``, ``lambda_raydrop_bce`` and
``use_rayhit`` (``training.default_options()``).  Channels of ``rendered``: 0 intensity, 1 ray-hit logit, 2 ray-drop logit, 3 depth.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Tuple

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LRT_LOSS_LIB") or os.path.join(HERE, "csrc", "liblrt_loss.so")
EXPORTS = ("lrt_loss_abi_version", "lrt_loss_last_error", "lrt_loss_work_bytes", "lrt_loss_forward", "lrt_loss_backward")   # include/lrt_loss.h
ABI_VERSION = 1

_lib = None


class LossError(RuntimeError):
    pass


def load():
    """Load liblrt_loss.so (after torch, so that both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LossError(f"{LIB_PATH} is missing: build it with `python -m lidar_rt_amd.build` (hipcc --offload-arch=gfx950). "
                        "range_image_loss has no fall-back; range_image_loss_torch is the PyTorch expression.")
    lib = C.CDLL(LIB_PATH)
    vp, ci = C.c_void_p, C.c_int
    lib.lrt_loss_abi_version.restype = ci
    lib.lrt_loss_last_error.restype = C.c_char_p
    lib.lrt_loss_work_bytes.restype = C.c_size_t; lib.lrt_loss_work_bytes.argtypes = [ci, ci]
    lib.lrt_loss_forward.restype = ci
    lib.lrt_loss_forward.argtypes = [ci, ci, ci, vp, vp, vp, vp, C.POINTER(C.c_double), ci, vp, vp, C.c_size_t, vp]
    lib.lrt_loss_backward.restype = ci
    lib.lrt_loss_backward.argtypes = [ci, ci, ci, vp, vp, vp, vp, C.POINTER(C.c_double), ci, vp, vp, vp, C.c_size_t, vp]
    if lib.lrt_loss_abi_version() != ABI_VERSION:
        raise LossError("liblrt_loss.so ABI version mismatch; rebuild with `python -m lidar_rt_amd.build --force`")
    _lib = lib
    return lib


def _check(rc: int, what: str):
    if rc != 0:
        raise LossError(f"{what} failed ({rc}): {load().lrt_loss_last_error().decode()}")


def _weights(opt) -> Tuple[float, float, float, float, float]:
    return (float(opt.lambda_depth_l1), float(opt.lambda_intensity_l1), float(opt.lambda_intensity_l2), float(opt.lambda_intensity_dssim),
            float(opt.lambda_raydrop_bce))


def range_image_loss_torch(rendered: torch.Tensor, gt_depth: torch.Tensor, gt_intensity: torch.Tensor, mask: torch.Tensor, opt):
    """(total, depth term, intensity term, ray-drop term, n) in PyTorch, term for term what ``training_step`` computes from
    ``renderer.raytracing``'s package: the channel slices and the ray-drop probability of the renderer, then the step's losses."""
    from .training import ssim
    intensities, rayhit_logits = rendered[:, :, 0:1], rendered[:, :, 1:2]
    raydrop_logits, depth = rendered[:, :, 2:3], rendered[:, :, 3:4]
    if getattr(opt, "use_rayhit", False):
        prob = F.softmax(torch.cat([rayhit_logits, raydrop_logits], dim=-1), dim=-1)
        raydrop = prob[..., 1:2]
    else:
        raydrop = torch.sigmoid(raydrop_logits)
    depth, intensity = depth.squeeze(-1), intensities.squeeze(-1)
    gt_int = gt_intensity
    mf = mask.to(depth.dtype)
    n_valid = mf.sum().clamp_min(1.0)
    mmean = lambda x: (x * mf).sum() / n_valid
    loss_depth = opt.lambda_depth_l1 * mmean(torch.abs(depth - gt_depth))
    loss_int = (opt.lambda_intensity_l1 * mmean(torch.abs(intensity - gt_int))
                + opt.lambda_intensity_l2 * mmean((intensity - gt_int) ** 2)
                + opt.lambda_intensity_dssim * (1 - ssim((intensity * mf).unsqueeze(0), (gt_int * mf).unsqueeze(0))))
    labels = (1.0 - mf).reshape(-1, 1)                                # 1 = dropped ray (train.py:188-193)
    loss_drop = opt.lambda_raydrop_bce * F.binary_cross_entropy(raydrop.reshape(-1, 1).clamp(1e-7, 1 - 1e-7), labels)
    return loss_depth + loss_int + loss_drop, loss_depth, loss_int, loss_drop, n_valid


_WORK = {}          # (H, W, device index) -> [workspace, serial of the forward whose maps it holds]
_SERIAL = 0


def _workspace(H: int, W: int, dev: torch.device):
    key = (H, W, dev.index)
    ent = _WORK.get(key)
    if ent is None:
        nb = int(load().lrt_loss_work_bytes(H, W))
        if nb == 0:
            raise LossError(f"range_image_loss: unsupported image size {H} x {W}")
        if len(_WORK) > 16:
            _WORK.clear()
        ent = _WORK[key] = [torch.empty((nb + 7) // 8, dtype=torch.float64, device=dev), -1]
    return ent


class _RangeImageLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rendered, gt_depth, gt_intensity, mask8, weights, use_rayhit):
        H, W = rendered.shape[0], rendered.shape[1]
        dev = rendered.device
        rendered = rendered.contiguous()
        out = torch.empty(5, dtype=torch.float32, device=dev)
        ctx.args = (H, W, dev.index, (C.c_double * 5)(*weights), int(bool(use_rayhit)))
        ctx.save_for_backward(rendered, gt_depth, gt_intensity, mask8)
        ctx.serial = _RangeImageLoss._launch_forward(ctx.args, rendered, gt_depth, gt_intensity, mask8, out)
        ctx.mark_non_differentiable(out)
        return out[0], out

    @staticmethod
    def _launch_forward(args, rendered, gt_depth, gt_intensity, mask8, out):
        global _SERIAL
        H, W, idx, w, rayhit = args
        ent = _workspace(H, W, rendered.device)
        work = ent[0]
        with torch.cuda.device(idx):
            stream = C.c_void_p(torch.cuda.current_stream(rendered.device).cuda_stream)
            _check(load().lrt_loss_forward(idx, H, W, rendered.data_ptr(), gt_depth.data_ptr(), gt_intensity.data_ptr(), mask8.data_ptr(), w, rayhit,
                                           out.data_ptr(), work.data_ptr(), work.numel() * 8, stream), "lrt_loss_forward")
        _SERIAL += 1
        ent[1] = _SERIAL
        return _SERIAL

    @staticmethod
    def backward(ctx, d_total, _d_out):
        rendered, gt_depth, gt_intensity, mask8 = ctx.saved_tensors
        H, W, idx, w, rayhit = ctx.args
        dev = rendered.device
        ent = _workspace(H, W, dev)
        if ent[1] != ctx.serial:
            # another forward of this image size ran in between (the workspace is shared): redo this one's, two launches
            ctx.serial = _RangeImageLoss._launch_forward(ctx.args, rendered, gt_depth, gt_intensity, mask8, torch.empty(5, dtype=torch.float32, device=dev))
        d_total = d_total.to(torch.float32).reshape(1).contiguous()
        d_rendered = torch.empty_like(rendered)              # every row is written whole by the kernel: no clearing
        work = ent[0]
        with torch.cuda.device(idx):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _check(load().lrt_loss_backward(idx, H, W, rendered.data_ptr(), gt_depth.data_ptr(), gt_intensity.data_ptr(), mask8.data_ptr(), w, rayhit,
                                            d_total.data_ptr(), d_rendered.data_ptr(), work.data_ptr(), work.numel() * 8, stream), "lrt_loss_backward")
        return d_rendered, None, None, None, None, None


def range_image_loss(rendered: torch.Tensor, gt_depth: torch.Tensor, gt_intensity: torch.Tensor, mask: torch.Tensor, opt):
    """(total, depth term, intensity term, ray-drop term, n) from the fused HIP operator; ``total`` carries the gradient w.r.t. ``rendered``."""
    if not (isinstance(rendered, torch.Tensor) and rendered.is_cuda and rendered.dtype == torch.float32 and rendered.dim() == 3 and rendered.shape[2] == 9):
        raise LossError("range_image_loss: rendered must be a float32 HIP tensor (H, W, 9); range_image_loss_torch takes everything else")
    H, W = rendered.shape[0], rendered.shape[1]
    dev = rendered.device
    for name, t in (("gt_depth", gt_depth), ("gt_intensity", gt_intensity), ("mask", mask)):
        if not isinstance(t, torch.Tensor) or t.device != dev or tuple(t.shape) != (H, W):
            raise LossError(f"range_image_loss: {name} must be a ({H}, {W}) tensor on {dev}")
    gt_depth = gt_depth.detach().to(torch.float32).contiguous()
    gt_intensity = gt_intensity.detach().to(torch.float32).contiguous()
    if mask.dtype == torch.bool:
        mask8 = mask.contiguous().view(torch.uint8)          # the same bytes: no launch
    elif mask.dtype == torch.uint8:
        mask8 = mask.contiguous()
    else:
        mask8 = (mask != 0).view(torch.uint8)
    total, out = _RangeImageLoss.apply(rendered, gt_depth, gt_intensity, mask8, _weights(opt), bool(getattr(opt, "use_rayhit", False)))
    return total, out[1], out[2], out[3], out[4]
