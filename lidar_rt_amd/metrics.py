"""Every figure ``evaluation.evaluate`` reports for a frame, in one operator (``evaluate(..., fused=True)``).

    row = frame_metrics(pred, gt_depth, gt_intensity, gt_mask, rays=None, *, raydrop_ratio=0.4, use_gt_mask=False, max_depth=80.0,
                        threshold=0.05, out=None)
    row = frame_metrics_reference(...)                      # the same arguments without ``out``

``pred`` is what ``evaluation.render_frames`` returns for a frame (``{"depth", "intensity", "raydrop"}``, each (H, W, 1) or (H, W)) or the three
images as a tuple; ``rays`` the frame's ``(rays_o, rays_d)``, each (H, W, 3) -- ``None`` skips the points metrics (NaN).  ``ROW`` names the row's
elements in order: depth and intensity ``rmse, mae, medae, ssim, psnr``, ray-drop ``rmse, acc, f1``, points ``chamfer_dist, fscore, n_pred, n_gt``
(the last two are extras: the sizes of the two clouds).  ``include/lrt_metrics.h`` states every figure line by line.

* ``frame_metrics_reference``: the float64 PyTorch twin, any device -- float32 clamps and ONE float32 subtraction as ``evaluate`` forms them, then
  float64 sums; the median from a sort, SSIM from ``avg_pool2d``, nearest neighbours by brute force.  Returns a float64 row.  It is the yardstick.
* ``frame_metrics``: the same row in float32 from ``csrc/liblrt_metrics.so`` (``include/lrt_metrics.h``): no sort (a three-level histogram
  selection returns the sort's bits), no boolean indexing, no host wait.  The nearest distances come from the grid Chamfer operator
  (``grid_chamfer``: ``lrt_gridcd_forward`` on cloud A = the ground truth under its mask, cloud B = the prediction under the chosen mask), this
  library adds them up.  HIP float32 tensors only -- a missing library is an error, there is no quiet fall-back.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LRT_METRICS_LIB") or os.path.join(HERE, "csrc", "liblrt_metrics.so")
EXPORTS = ("lrt_metrics_abi_version", "lrt_metrics_last_error", "lrt_metrics_work_bytes", "lrt_metrics_frame")   # include/lrt_metrics.h
ABI_VERSION = 1

ROW = (("depth", "rmse"), ("depth", "mae"), ("depth", "medae"), ("depth", "ssim"), ("depth", "psnr"),
       ("intensity", "rmse"), ("intensity", "mae"), ("intensity", "medae"), ("intensity", "ssim"), ("intensity", "psnr"),
       ("raydrop", "rmse"), ("raydrop", "acc"), ("raydrop", "f1"),
       ("points", "chamfer_dist"), ("points", "fscore"), ("points", "n_pred"), ("points", "n_gt"))
N = len(ROW)                                                        # LRT_METRICS_N
EXTRAS = (("points", "n_pred"), ("points", "n_gt"))                # in the row, not in evaluate's dictionary
WIN = 7

_lib = None


class MetricsError(RuntimeError):
    pass


def load():
    """Load liblrt_metrics.so (after torch, so that both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MetricsError(f"{LIB_PATH} is missing: build it with `python -m lidar_rt_amd.build` (hipcc --offload-arch=gfx950). "
                           "frame_metrics has no fall-back; frame_metrics_reference is the PyTorch expression.")
    lib = C.CDLL(LIB_PATH)
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    lib.lrt_metrics_abi_version.restype = ci
    lib.lrt_metrics_last_error.restype = C.c_char_p
    lib.lrt_metrics_work_bytes.restype = C.c_size_t; lib.lrt_metrics_work_bytes.argtypes = [ci, ci]
    lib.lrt_metrics_frame.restype = ci
    lib.lrt_metrics_frame.argtypes = [ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, cd, ci, cd, cd, vp, vp, C.c_size_t, vp]
    if lib.lrt_metrics_abi_version() != ABI_VERSION:
        raise MetricsError("liblrt_metrics.so ABI version mismatch; rebuild with `python -m lidar_rt_amd.build --force`")
    _lib = lib
    return lib


def _check(rc: int, what: str):
    if rc != 0:
        raise MetricsError(f"{what} failed ({rc}): {load().lrt_metrics_last_error().decode()}")


def _images(pred) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    if isinstance(pred, dict):
        return pred["depth"], pred["intensity"], pred["raydrop"]
    d, i, r = pred
    return d, i, r


def _hw(name: str, t, H: int, W: int) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or tuple(t.shape) not in ((H, W), (H, W, 1)):
        raise MetricsError(f"frame_metrics: {name} must be a ({H}, {W}) or ({H}, {W}, 1) tensor, not {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    return t.reshape(H, W)


def _ratio32(raydrop_ratio: float) -> float:
    """The threshold as the float32 comparison sees it (`raydrop < ratio` on a float32 tensor compares in float32)."""
    return float(torch.tensor(float(raydrop_ratio), dtype=torch.float32))


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------------------

def _nearest_d2_f32(q: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """Per row of ``q`` the smallest squared distance to a row of ``c`` with the operators' float32 arithmetic (lrt_gridcd.h): d = c - q in
    float32, then fma(dz, dz, fma(dy, dy, dx * dx)) -- each product exact in float64 and rounded to float32 once per step."""
    out = torch.empty(q.shape[0], dtype=torch.float32, device=q.device)
    step = max(1, (1 << 21) // max(1, c.shape[0]))
    for s in range(0, q.shape[0], step):
        d = (c[None, :, :] - q[s:s + step, None, :]).double()
        t = (d[..., 0] * d[..., 0]).float().double()
        t = (d[..., 1] * d[..., 1] + t).float().double()
        out[s:s + step] = (d[..., 2] * d[..., 2] + t).float().min(1).values
    return out


def _ssim64(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """skimage.metrics.structural_similarity(x, y, data_range = max y - min y) with its defaults, float64 (evaluation.ssim_uniform's expression
    without the final rounding); NaN for a constant ground truth (C1 = C2 = 0: the window term is 0 / 0 or rounding noise over rounding noise)."""
    import torch.nn.functional as F
    x = x.double()[None, None]; y = y.double()[None, None]
    pool = lambda a: F.avg_pool2d(a, WIN, stride=1)
    ux, uy = pool(x), pool(y)
    norm = WIN * WIN / (WIN * WIN - 1.0)
    vx = norm * (pool(x * x) - ux * ux); vy = norm * (pool(y * y) - uy * uy); vxy = norm * (pool(x * y) - ux * uy)
    R = y.max() - y.min()
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return torch.where(R == 0, torch.full_like(R, float("nan")), S.mean())


def _image_row(y: torch.Tensor, x: torch.Tensor, peak: float):
    """[rmse, mae, medae, ssim, psnr] of the clamped float32 pair (y the ground truth, x the prediction), float64."""
    e = y - x                                                           # ONE float32 subtraction
    a = e.abs()
    mse = (e.double() ** 2).mean()
    v = a.flatten().sort().values
    n = v.numel()
    medae = (0.5 * (v[(n - 1) // 2] + v[n // 2])).double()              # float32, as numpy's median of float32 values
    return [mse.sqrt(), a.double().mean(), medae, _ssim64(x, y), 10.0 * torch.log10(peak * peak / mse.clamp_min(1e-30))]


@torch.no_grad()
def frame_metrics_reference(pred, gt_depth, gt_intensity, gt_mask, rays=None, *, raydrop_ratio: float = 0.4, use_gt_mask: bool = False,
                            max_depth: float = 80.0, threshold: float = 0.05) -> torch.Tensor:
    """The row in float64, by the plainest means: sort, avg_pool2d, brute force."""
    H, W = gt_depth.shape[:2]
    if H < WIN or W < WIN:
        raise MetricsError(f"frame_metrics: a {WIN} x {WIN} SSIM window does not fit a {H} x {W} image")
    pd, pi, pr = (_hw(n_, t, H, W).float() for n_, t in zip(("pred depth", "pred intensity", "pred raydrop"), _images(pred)))
    gd, gi = _hw("gt_depth", gt_depth, H, W).float(), _hw("gt_intensity", gt_intensity, H, W).float()
    gt_hit = _hw("gt_mask", gt_mask, H, W) != 0
    pred_hit = pr < _ratio32(raydrop_ratio)
    mask = gt_hit if use_gt_mask else pred_hit
    mk = mask.float()
    row = _image_row(gd.clamp(1e-6, max_depth), (pd * mk).clamp(1e-6, max_depth), float(max_depth))
    row += _image_row(gi.clamp(0, 1).clamp(1e-6, 1.0), (pi.clamp(0, 1) * mk).clamp(1e-6, 1.0), 1.0)
    g, p = ~gt_hit, ~pred_hit                                           # the drop masks
    cnt = lambda m: m.sum().double()
    tp, fp, fn, eq, n = cnt(g & p), cnt(~g & p), cnt(g & ~p), cnt(g == p), float(H * W)
    precision, recall = tp / (tp + fp).clamp_min(1.0), tp / (tp + fn).clamp_min(1.0)
    row += [((n - eq) / n).sqrt(), eq / n, 2 * precision * recall / (precision + recall).clamp_min(1e-30)]
    n_pred, n_gt = cnt(mask), cnt(gt_hit)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=gd.device)
    if rays is None:
        row += [nan, nan]
    elif int(n_pred) == 0 or int(n_gt) == 0:
        row += [nan, torch.zeros_like(nan)]
    else:
        o, d = rays
        o, d = o.float(), d.float()
        a = (o + d * gd[..., None]).reshape(-1, 3)[gt_hit.reshape(-1)]
        b = (o + d * pd[..., None]).reshape(-1, 3)[mask.reshape(-1)]
        da, db = _nearest_d2_f32(a, b), _nearest_d2_f32(b, a)
        thr = float(torch.tensor(float(threshold), dtype=torch.float32))
        p1, p2 = (da < thr).double().mean(), (db < thr).double().mean()
        row += [da.double().mean() + db.double().mean(), torch.nan_to_num(2 * p1 * p2 / (p1 + p2), nan=0.0)]
    row += [n_pred, n_gt]
    return torch.stack([torch.as_tensor(v, dtype=torch.float64, device=gd.device).reshape(()) for v in row])


# ---- the HIP operator ---------------------------------------------------------------------------------------------------------------------------

_WORK = {}          # (H, W, device index) -> workspace (scratch only: nothing lives there between two calls)


def _workspace(H: int, W: int, dev: torch.device) -> torch.Tensor:
    key = (H, W, dev.index)
    w = _WORK.get(key)
    if w is None:
        nb = int(load().lrt_metrics_work_bytes(H, W))
        if nb == 0:
            raise MetricsError(f"frame_metrics: unsupported image size {H} x {W} (a {WIN} x {WIN} SSIM window must fit)")
        if len(_WORK) > 16:
            _WORK.clear()
        w = _WORK[key] = torch.empty((nb + 7) // 8, dtype=torch.float64, device=dev)
    return w


def _dev32(name: str, t, H: int, W: int, dev: torch.device) -> torch.Tensor:
    t = _hw(name, t, H, W)
    if t.device != dev or t.dtype != torch.float32:
        raise MetricsError(f"frame_metrics: {name} must be a float32 tensor on {dev} (it is {t.dtype} on {t.device})")
    return t.detach().contiguous()


@torch.no_grad()
def frame_metrics(pred, gt_depth, gt_intensity, gt_mask, rays=None, *, raydrop_ratio: float = 0.4, use_gt_mask: bool = False,
                  max_depth: float = 80.0, threshold: float = 0.05, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The row (``N`` float32 on the device) from the HIP operator, stream-ordered, without a host wait; ``out``: a row of a caller-owned table."""
    from . import grid_chamfer as gc
    if not (isinstance(gt_depth, torch.Tensor) and gt_depth.is_cuda and gt_depth.dtype == torch.float32 and gt_depth.dim() in (2, 3)):
        raise MetricsError("frame_metrics: gt_depth must be a float32 HIP tensor (H, W); frame_metrics_reference takes everything else")
    H, W = gt_depth.shape[:2]
    dev = gt_depth.device
    work = _workspace(H, W, dev)
    gd, gi = _dev32("gt_depth", gt_depth, H, W, dev), _dev32("gt_intensity", gt_intensity, H, W, dev)
    pd, pi, pr = (_dev32(n_, t, H, W, dev) for n_, t in zip(("pred depth", "pred intensity", "pred raydrop"), _images(pred)))
    gm = _hw("gt_mask", gt_mask, H, W)
    if gm.device != dev:
        raise MetricsError(f"frame_metrics: gt_mask must be on {dev}")
    gm8 = gc._mask8(gm)
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=dev)
    elif not (isinstance(out, torch.Tensor) and out.device == dev and out.dtype == torch.float32 and out.numel() == N and out.is_contiguous()):
        raise MetricsError(f"frame_metrics: out must be {N} contiguous float32 on {dev}")
    dist_a = dist_b = None
    if rays is not None:
        o, d = rays
        for name, t in (("rays_o", o), ("rays_d", d)):
            if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.float32 or tuple(t.shape) != (H, W, 3):
                raise MetricsError(f"frame_metrics: {name} must be a float32 ({H}, {W}, 3) tensor on {dev}")
        mb8 = gm8 if use_gt_mask else (pr < _ratio32(raydrop_ratio)).view(torch.uint8)
        _, dist_a, dist_b, _, _ = gc._launch_forward(o.detach().contiguous(), d.detach().contiguous(), gd, pd, gm8, mb8, 1.0)
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _check(load().lrt_metrics_frame(dev.index, H, W, pd.data_ptr(), pi.data_ptr(), pr.data_ptr(), gd.data_ptr(), gi.data_ptr(), gm8.data_ptr(),
                                        dist_a.data_ptr() if dist_a is not None else None, dist_b.data_ptr() if dist_b is not None else None,
                                        float(raydrop_ratio), int(bool(use_gt_mask)), float(max_depth), float(threshold), out.data_ptr(),
                                        work.data_ptr(), work.numel() * 8, stream), "lrt_metrics_frame")
    return out
