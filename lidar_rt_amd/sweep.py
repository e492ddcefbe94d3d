"""Sweep rays: the ray grid of a spinning LiDAR that moves while it turns, with gradients for its pose and its motion, through
``csrc/liblrt_sweep.so``.

    o, d = sweep_rays(pose, twist, H, W, inclination, data_type="KITTI", sensor2ego=None, tau=None, t_ref=0.5)
    o, d = sweep_rays_reference(...)                     # the float64 torch twin, autograd-able, runs anywhere
    tau = column_times(W, t_ref=0.5, direction="cw")     # (w + 0.5) / W - t_ref
    xi = twist_between(T0, T1)                           # Log(T0^-1 T1), host float64; se3_log is the inverse of poses.se3_exp

Column ``w`` of a range image is fired at its own instant ``tau[w]`` (in sweeps, 0 = the instant the frame's pose holds), so it has its own
pose ``T(tau[w]) = pose @ Exp(tau[w] * twist)``: ``twist = (rho, phi)`` is the sensor's motion over one whole sweep in the sensor frame, the
convention of ``poses.se3_exp`` and of ``sensor2world @ Exp(xi)``.  The local directions are ``RangeFrames.range_rays``'s.
``include/lrt_sweep.h`` states the rule; ``csrc/lrt_sweep_math.h`` is its text for the device and the host, all of it float64.

* ``pose``: ``(3, 4)`` / ``(4, 4)`` or batched ``(F, 3, 4)`` / ``(F, 4, 4)``; ``twist``: ``(6,)`` / ``(F, 6)`` or ``None`` (a static sensor: the
  grid of ``range_rays`` in float64).  Without a batch axis the results ``(H, W, 3)`` have none either.
* ``inclination``: two bounds, a per-beam table of ``H`` angles (row ``h`` has ``inclination[H - 1 - h]``), or one number ``x`` for ``[-x, x]``;
  it is read as float32, as the library reads it.  ``tau``: ``(W,)``, read as float32; ``None`` means ``column_times(W, t_ref)``.  Both may be
  float32 tensors that already live on the pose's device (they are used as they are, without an upload).
* ``sweep_rays``: HIP float32 tensors go through the library -- two launches forward, two backward, no host wait (give ``sensor2ego`` as host
  data).  It is differentiable in ``pose`` and ``twist``.  A missing library is an error, and so is any other tensor on a HIP device: there is
  no quiet fall-back.  CPU tensors go to the twin.
* ``sweep_rays_reference(..., per_ray=True, g_o=..., g_d=...)`` also returns ``(F, H, W, 18)``: every ray's contribution to the 12 entries of
  ``d_pose`` and the 6 of ``d_twist`` for those upstream gradients (their sum over the rays is the gradient).
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LRT_SWEEP_LIB") or os.path.join(HERE, "csrc", "liblrt_sweep.so")
EXPORTS = ("lrt_sweep_abi_version", "lrt_sweep_last_error", "lrt_sweep_work_bytes", "lrt_sweep_rays", "lrt_sweep_backward")     # include/lrt_sweep.h
ABI_VERSION = 1
BLOCK = 256                                                                  # LRT_SWEEP_BLOCK
COLS = 64                                                                    # LRT_SWEEP_COLS
MAX_RAYS = (2 ** 31 - 1) // 3                                                # LRT_SWEEP_MAX_RAYS
SERIES_TH2 = 0.25                                                            # SW_SERIES_TH2
SERIES_TERMS = 10                                                            # SW_SERIES_TERMS
TWO_PI = 6.28318530717958647692
PI = 3.14159265358979323846

_lib = None


class SweepError(RuntimeError):
    pass


def load():
    """Load liblrt_sweep.so (after torch, so that both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SweepError(f"{LIB_PATH} is missing: build it with `python -m lidar_rt_amd.build` (hipcc --offload-arch=gfx950). "
                         "sweep_rays has no fall-back on a HIP device.")
    lib = C.CDLL(LIB_PATH)
    lib.lrt_sweep_abi_version.restype = C.c_int
    lib.lrt_sweep_last_error.restype = C.c_char_p
    lib.lrt_sweep_work_bytes.restype = C.c_longlong
    lib.lrt_sweep_work_bytes.argtypes = [C.c_longlong, C.c_int, C.c_int]
    common = [C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p]
    lib.lrt_sweep_rays.restype = C.c_int
    lib.lrt_sweep_rays.argtypes = common + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
    lib.lrt_sweep_backward.restype = C.c_int
    lib.lrt_sweep_backward.argtypes = common + [C.c_void_p] * 5 + [C.c_longlong, C.c_void_p]
    if lib.lrt_sweep_abi_version() != ABI_VERSION:
        raise SweepError("liblrt_sweep.so ABI version mismatch; rebuild with `python -m lidar_rt_amd.build --force`")
    _lib = lib
    return lib


# ---- column times, Log ------------------------------------------------------------------------------------------------------------------------------------

def column_times(W: int, t_ref: float = 0.5, direction: str = "cw") -> torch.Tensor:
    """(W,) float64: the instant of column w in sweeps, (w + 0.5) / W - t_ref.  "cw": time rises with the column index, the order in which a
    clockwise-spinning sensor fills this grid (its azimuth falls with w); "ccw" negates it."""
    if direction not in ("cw", "ccw"):
        raise SweepError(f"column_times: direction {direction!r} (cw or ccw)")
    if not (isinstance(W, (int, np.integer)) and W >= 1):
        raise SweepError(f"column_times: {W!r} columns")
    t = (torch.arange(int(W), dtype=torch.float64) + 0.5) / float(W) - float(t_ref)
    return t if direction == "cw" else -t


def _nested_np(u, j):
    v = 1.0
    for k in range(SERIES_TERMS - 1, -1, -1):
        v = 1.0 - u * v / float((2 * k + 2 + j) * (2 * k + 3 + j))
    return v


def _coef_np(u):
    """(A, B, C) of lrt_sweep_math.h at u = theta^2."""
    if u < SERIES_TH2:
        return _nested_np(u, 0), _nested_np(u, 1) / 2.0, _nested_np(u, 2) / 6.0
    t = math.sqrt(u)
    return math.sin(t) / t, (1.0 - math.cos(t)) / u, (t - math.sin(t)) / (u * t)


def _hat_np(p):
    return np.array([[0.0, -p[2], p[1]], [p[2], 0.0, -p[0]], [-p[1], p[0], 0.0]])


def _host_matrix(name, T):
    if torch.is_tensor(T):
        T = T.detach().cpu().numpy()
    T = np.asarray(T, np.float64)
    if T.shape not in ((3, 4), (4, 4)):
        raise SweepError(f"{name}: a (3, 4) or (4, 4) pose (it is {T.shape})")
    return T[:3]


def se3_log(T) -> np.ndarray:
    """(6,) float64 xi = (rho, phi) with poses.se3_exp(xi) = T; host arithmetic.  |phi| <= pi; exact at zero rotation and stable next to pi, where
    the axis comes from the symmetric part of R."""
    T = _host_matrix("se3_log", T)
    R, t = T[:, :3], T[:, 3]
    w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])          # sin(theta) axis
    c = 0.5 * (np.trace(R) - 1.0)
    sn = float(np.linalg.norm(w))
    theta = math.atan2(sn, c)
    if c > -0.5:
        phi = w * (1.0 + sn * sn / 6.0 + 3.0 * sn ** 4 / 40.0 if sn < 1e-4 else theta / sn)     # asin(x) / x = 1 + x^2 / 6 + 3 x^4 / 40
    else:
        S = (0.5 * (R + R.T) - c * np.eye(3)) / (1.0 - c)                                  # axis axis^T
        k = int(np.argmax(np.diag(S)))
        a = S[:, k] / math.sqrt(S[k, k])
        if np.dot(a, w) < 0.0:
            a = -a
        phi = theta * a / np.linalg.norm(a)
    _, B, Cc = _coef_np(float(phi @ phi))
    K = _hat_np(phi)
    V = np.eye(3) + B * K + Cc * (K @ K)
    return np.concatenate([np.linalg.solve(V, t), phi])


def twist_between(T0, T1) -> np.ndarray:
    """Log(T0^-1 T1): the motion, in T0's frame, that carries pose T0 to pose T1."""
    A, B = _host_matrix("twist_between", T0), _host_matrix("twist_between", T1)
    Ri = A[:, :3].T
    rel = np.concatenate([Ri @ B[:, :3], (Ri @ (B[:, 3] - A[:, 3]))[:, None]], 1)
    return se3_log(rel)


def twists_from_poses(poses: dict, sweep_fraction: float = 1.0) -> dict:
    """{id: (6,) float64}: the sensor's motion over one sweep from a trajectory {id: (4, 4) pose}: xi_k = Log(T_k^-1 T_next) * sweep_fraction /
    (id gap) over the ids in ascending order (``sweep_fraction``: the part of the time between two consecutive ids that one sweep takes); the
    last frame takes the previous interval's.  A single pose has no neighbour and is refused."""
    ids = sorted(int(i) for i in poses)
    if len(ids) < 2:
        raise SweepError(f"twists_from_poses: twists from poses need at least two frames (there {'is' if len(ids) == 1 else 'are'} {len(ids)})")
    if not (float(sweep_fraction) > 0.0 and math.isfinite(float(sweep_fraction))):
        raise SweepError(f"twists_from_poses: sweep_fraction {sweep_fraction!r} (positive)")
    out = {}
    for a, b in zip(ids[:-1], ids[1:]):
        out[a] = twist_between(poses[a], poses[b]) * (float(sweep_fraction) / float(b - a))
    out[ids[-1]] = out[ids[-2]].copy()
    return out


# ---- the arguments ------------------------------------------------------------------------------------------------------------------------------------------

def convention(data_type: str = "KITTI", sensor2ego=None):
    """(off, yaw) of a data type as ``RangeFrames.range_rays`` derives them (yaw: atan2 of the sensor-to-ego rotation in float32)."""
    if data_type not in ("KITTI", "Waymo"):
        raise SweepError(f"sweep_rays: data_type {data_type!r} (KITTI or Waymo)")
    if data_type != "Waymo":
        return 0.0, 0.0
    if sensor2ego is None:
        return 0.5, 0.0
    s = torch.as_tensor(sensor2ego).detach().to("cpu", torch.float32)
    if s.dim() != 2 or s.shape[0] < 2 or s.shape[1] < 1:
        raise SweepError(f"sweep_rays: sensor2ego must be a (4, 4) matrix (it is {tuple(s.shape)})")
    return 0.5, float(torch.atan2(s[1, 0], s[0, 0]))


def _small(name, x, n_ok, dev=None):
    """A small argument as a float32 tensor: host data becomes a CPU tensor; a float32 tensor on ``dev`` is kept."""
    if torch.is_tensor(x) and x.device.type != "cpu":
        if dev is None or x.device != dev or x.dtype != torch.float32:
            raise SweepError(f"sweep_rays: {name} on {x.device} must be a float32 tensor on the pose's device (or host data)")
        t = x.detach().reshape(-1).contiguous()
    else:
        try:
            t = torch.as_tensor(np.asarray(x.detach().numpy() if torch.is_tensor(x) else x, dtype=np.float64)).reshape(-1).to(torch.float32)
        except (TypeError, ValueError) as e:
            raise SweepError(f"sweep_rays: {name} is not numeric: {e}") from None
        if not bool(torch.isfinite(t).all()):
            raise SweepError(f"sweep_rays: a non-finite {name}")
    if t.numel() not in n_ok:
        raise SweepError(f"sweep_rays: {name} holds {t.numel()} numbers ({' or '.join(str(n) for n in sorted(set(n_ok)))})")
    return t


def _arguments(pose, twist, H, W, inclination, data_type, sensor2ego, tau, t_ref, dev=None):
    """(pose (F, 3, 4), twist (F, 6) or None, batched, H, W, inc float32, tau float32, off, yaw); pose and twist keep their graph."""
    if not (isinstance(H, (int, np.integer)) and isinstance(W, (int, np.integer)) and H >= 1 and W >= 1):
        raise SweepError(f"sweep_rays: a grid of {H!r} x {W!r} rays")
    H, W = int(H), int(W)
    if not torch.is_tensor(pose) or pose.dim() not in (2, 3) or tuple(pose.shape[-2:]) not in ((3, 4), (4, 4)):
        raise SweepError(f"sweep_rays: pose must be a (3, 4) / (4, 4) tensor or a batch of them (it is {tuple(pose.shape) if torch.is_tensor(pose) else type(pose).__name__})")
    batched = pose.dim() == 3
    P = (pose if batched else pose[None])[:, :3, :]
    F = P.shape[0]
    if F < 1 or F * H * W > MAX_RAYS:
        raise SweepError(f"sweep_rays: {F} frames of {H} x {W} rays (each at least 1, F H W at most {MAX_RAYS})")
    xi = None
    if twist is not None:
        if not torch.is_tensor(twist) or tuple(twist.shape) != ((F, 6) if batched else (6,)):
            raise SweepError(f"sweep_rays: twist must be {(F, 6) if batched else (6,)} (it is {tuple(twist.shape) if torch.is_tensor(twist) else type(twist).__name__})")
        if twist.device != pose.device or twist.dtype != pose.dtype:
            raise SweepError(f"sweep_rays: twist ({twist.dtype}, {twist.device}) and pose ({pose.dtype}, {pose.device}) differ")
        xi = twist if batched else twist[None]
    if isinstance(inclination, (int, float)):
        inclination = [-float(inclination), float(inclination)]
    inc = _small("inclination", inclination, (2, H), dev)
    if tau is None:
        tau = column_times(W, t_ref)
    tau = _small("tau", tau, (W,), dev)
    off, yaw = convention(data_type, sensor2ego)
    return P, xi, batched, H, W, inc, tau, off, yaw


# ---- the twin -----------------------------------------------------------------------------------------------------------------------------------------------

def _nested(u, j):
    v = torch.ones_like(u)
    for k in range(SERIES_TERMS - 1, -1, -1):
        v = 1.0 - u * v / float((2 * k + 2 + j) * (2 * k + 3 + j))
    return v


def _exp64(x):
    """Exp of x (..., 6) float64 = (rho, phi): (Re (..., 3, 3), te (..., 3)); the series below SERIES_TH2, as lrt_sweep_math.h."""
    rho, phi = x[..., :3], x[..., 3:]
    u = (phi * phi).sum(-1)
    small = u < SERIES_TH2
    us = torch.where(small, torch.ones_like(u), u)                           # keeps the unused branch finite (and its gradient)
    t = torch.sqrt(us)
    A = torch.where(small, _nested(u, 0), torch.sin(t) / t)
    B = torch.where(small, _nested(u, 1) / 2.0, (1.0 - torch.cos(t)) / us)
    Cc = torch.where(small, _nested(u, 2) / 6.0, (t - torch.sin(t)) / (us * t))
    z = torch.zeros_like(u)
    K = torch.stack([torch.stack([z, -phi[..., 2], phi[..., 1]], -1), torch.stack([phi[..., 2], z, -phi[..., 0]], -1),
                     torch.stack([-phi[..., 1], phi[..., 0], z], -1)], -2)
    K2 = K @ K
    I = torch.eye(3, dtype=x.dtype, device=x.device)
    A, B, Cc = A[..., None, None], B[..., None, None], Cc[..., None, None]
    Re = I + A * K + B * K2
    te = ((I + B * K + Cc * K2) @ rho[..., None])[..., 0]
    return Re, te


def column_poses_reference(pose, twist, tau):
    """T(tau[w]) of every column in float64: (R (F, W, 3, 3), t (F, W, 3)).  pose (F, 3, 4); twist (F, 6) or None; tau (W,)."""
    P = pose.to(torch.float64)
    W = tau.numel()
    Rp, tp = P[:, None, :, :3], P[:, None, :, 3]
    if twist is None:
        return Rp.expand(-1, W, 3, 3), tp.expand(-1, W, 3)
    x = tau.to(device=P.device, dtype=torch.float64)[None, :, None] * twist.to(torch.float64)[:, None, :]
    Re, te = _exp64(x)
    return Rp @ Re, (Rp @ te[..., None])[..., 0] + tp


def _local(H, W, inc, off, yaw, dev):
    """cos / sin of the inclination (H,) and of the azimuth (W,), float64."""
    w = torch.arange(W, dtype=torch.float64, device=dev)
    az = ((float(W) - w) - off) / float(W) * TWO_PI - PI - yaw
    inc = inc.to(device=dev, dtype=torch.float64)
    if inc.numel() == 2:
        h = torch.arange(H, dtype=torch.float64, device=dev)
        el = ((float(H) - h) - off) / float(H) * (inc[1] - inc[0]) + inc[0]
    else:
        el = inc.flip(0)
    return torch.cos(el), torch.sin(el), torch.cos(az), torch.sin(az)


def _rays64(P, xi, s, ci, si, ca, sa):
    """The rule on broadcastable float64 batches: P (..., 3, 4), xi (..., 6) or None, s and the four trigonometric factors (...)."""
    Rp, tp = P[..., :3], P[..., 3]
    if xi is None:
        R, t = Rp, tp
    else:
        Re, te = _exp64(s[..., None] * xi)
        R = Rp @ Re
        t = (Rp @ te[..., None])[..., 0] + tp
    l = torch.stack([ci * ca, ci * sa, si.expand_as(ci * ca)], -1)
    v = (R @ l[..., None])[..., 0]
    d = v / torch.sqrt((v * v).sum(-1, keepdim=True))
    return t, d


def sweep_rays_reference(pose, twist, H, W, inclination, data_type="KITTI", sensor2ego=None, tau=None, t_ref=0.5, per_ray=False, g_o=None, g_d=None):
    """The float64 torch twin (see the module text): (ray_o, ray_d) float64 on the pose's device, differentiable in pose and twist.  With
    ``per_ray=True`` (and upstream gradients ``g_o``, ``g_d``) a third result (F, H, W, 18): each ray's contribution to d_pose (12) and d_twist (6)."""
    P, xi, batched, H, W, inc, tau, off, yaw = _arguments(pose, twist, H, W, inclination, data_type, sensor2ego, tau, t_ref, pose.device if torch.is_tensor(pose) else None)
    dev = P.device
    F = P.shape[0]
    ci, si, ca, sa = _local(H, W, inc, off, yaw, dev)
    ci, si, ca, sa = ci[None, :, None], si[None, :, None], ca[None, None, :], sa[None, None, :]
    s = tau.to(device=dev, dtype=torch.float64)[None, None, :]
    P64 = P.to(torch.float64)
    x64 = None if xi is None else xi.to(torch.float64)
    t, d = _rays64(P64[:, None, None], None if x64 is None else x64[:, None, None], s, ci, si, ca, sa)
    o = t.expand(F, H, W, 3)
    d = d.expand(F, H, W, 3)
    sq = (lambda a: a) if batched else (lambda a: a[0])
    if not per_ray:
        return sq(o), sq(d)
    if g_o is None or g_d is None:
        raise SweepError("sweep_rays_reference: per_ray=True needs the upstream gradients g_o and g_d")
    with torch.enable_grad():
        Pe = P64.detach()[:, None, None].expand(F, H, W, 3, 4).clone().requires_grad_(True)
        xe = None if x64 is None else x64.detach()[:, None, None].expand(F, H, W, 6).clone().requires_grad_(True)
        te, de = _rays64(Pe, xe, s.expand(F, H, W), ci, si, ca, sa)
        go = g_o.detach().to(device=dev, dtype=torch.float64).reshape(F, H, W, 3)
        gd = g_d.detach().to(device=dev, dtype=torch.float64).reshape(F, H, W, 3)
        ((te.expand(F, H, W, 3) * go).sum() + (de * gd).sum()).backward()
    gx = torch.zeros((F, H, W, 6), dtype=torch.float64, device=dev) if xe is None else xe.grad
    contrib = torch.cat([Pe.grad.reshape(F, H, W, 12), gx], -1)
    return sq(o.detach()), sq(d.detach()), sq(contrib)


# ---- the operator ---------------------------------------------------------------------------------------------------------------------------------------------

def work_bytes(F: int, H: int, W: int) -> int:
    """Bytes of the workspace of one call: the column and row tables and the workgroups' partial sums."""
    n = int(load().lrt_sweep_work_bytes(int(F), int(H), int(W)))
    if n < 0:
        raise SweepError(f"sweep_rays: {F} frames of {H} x {W} rays (each at least 1, F H W at most {MAX_RAYS})")
    return n


def _upload(t: torch.Tensor, dev) -> torch.Tensor:
    """A small host tensor on the device without a host wait: through pinned memory, which the allocator keeps until the copy has run."""
    return t if t.device == dev else t.contiguous().pin_memory().to(dev, non_blocking=True)


def _workspace(workspace, nbytes, dev):
    if workspace is None:
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)              # the caching allocator's blocks are 512-byte aligned
    if not (torch.is_tensor(workspace) and workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.device == dev
            and workspace.numel() >= nbytes and workspace.data_ptr() % 256 == 0):
        raise SweepError(f"lrt_sweep: the workspace must be a contiguous uint8 tensor of at least {nbytes} bytes on {dev}, 256-byte aligned")
    return workspace


class _SweepRays(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pose, twist, inc, tau, H, W, off, yaw, workspace):
        lib = load()
        dev = pose.device
        F = pose.shape[0]
        P = pose.detach().contiguous()
        xi = None if twist is None else twist.detach().contiguous()
        ws = _workspace(workspace, work_bytes(F, H, W), dev)
        ray_o = torch.empty((F, H, W, 3), dtype=torch.float32, device=dev)
        ray_d = torch.empty((F, H, W, 3), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = lib.lrt_sweep_rays(dev.index, F, H, W, P.data_ptr(), None if xi is None else xi.data_ptr(), inc.data_ptr(), inc.numel(), off, yaw,
                                    tau.data_ptr(), ray_o.data_ptr(), ray_d.data_ptr(), ws.data_ptr(), ws.numel(),
                                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc != 0:
            raise SweepError(f"lrt_sweep_rays failed ({rc}): {lib.lrt_sweep_last_error().decode()}")
        ctx.save_for_backward(P, xi, inc, tau)
        ctx.args = (H, W, off, yaw, workspace)
        return ray_o, ray_d

    @staticmethod
    def backward(ctx, g_o, g_d):
        lib = load()
        P, xi, inc, tau = ctx.saved_tensors
        H, W, off, yaw, workspace = ctx.args
        dev = P.device
        F = P.shape[0]
        g_o, g_d = g_o.to(torch.float32).contiguous(), g_d.to(torch.float32).contiguous()
        ws = _workspace(workspace, work_bytes(F, H, W), dev)
        d_pose = torch.empty((F, 3, 4), dtype=torch.float32, device=dev)
        d_twist = None if xi is None else torch.empty((F, 6), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = lib.lrt_sweep_backward(dev.index, F, H, W, P.data_ptr(), None if xi is None else xi.data_ptr(), inc.data_ptr(), inc.numel(), off, yaw,
                                        tau.data_ptr(), g_o.data_ptr(), g_d.data_ptr(), d_pose.data_ptr(), None if d_twist is None else d_twist.data_ptr(),
                                        ws.data_ptr(), ws.numel(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc != 0:
            raise SweepError(f"lrt_sweep_backward failed ({rc}): {lib.lrt_sweep_last_error().decode()}")
        return d_pose, d_twist, None, None, None, None, None, None, None


def sweep_rays(pose, twist, H, W, inclination, data_type="KITTI", sensor2ego=None, tau=None, t_ref=0.5, workspace=None):
    """The sweep rays of F frames (see the module text): (ray_o, ray_d), each (F, H, W, 3) float32, or (H, W, 3) for an unbatched pose.
    ``workspace``: a uint8 tensor on the pose's device of at least ``work_bytes(F, H, W)`` bytes to use instead of a fresh one, forward and
    backward; its contents do not matter."""
    dev = pose.device if torch.is_tensor(pose) else None
    P, xi, batched, H, W, inc, tau, off, yaw = _arguments(pose, twist, H, W, inclination, data_type, sensor2ego, tau, t_ref, dev)
    if dev.type != "cuda":
        if workspace is not None:
            raise SweepError(f"sweep_rays: a workspace with a pose on {dev}")
        o, d = sweep_rays_reference(pose, twist, H, W, inc, data_type, sensor2ego, tau)
        return o.to(torch.float32).contiguous(), d.to(torch.float32).contiguous()
    load()
    if P.dtype != torch.float32:
        raise SweepError(f"lrt_sweep: pose and twist must be float32 tensors (they are {P.dtype}); there is no fall-back to PyTorch on a HIP device")
    o, d = _SweepRays.apply(P.contiguous(), None if xi is None else xi.contiguous(), _upload(inc, dev), _upload(tau, dev), H, W, off, yaw, workspace)
    return (o, d) if batched else (o[0], d[0])
