"""Beam rays: the sweep rays of a sensor whose lasers are not where the nominal grid puts them, with gradients for its pose, its motion and
its beam table, through ``csrc/liblrt_beams.so``.

    o, d = beam_rays(pose, twist, H, W, inclination, beams, data_type="KITTI", sensor2ego=None, tau=None, t_ref=0.5)
    o, d = beam_rays_reference(...)                      # the float64 torch twin, autograd-able, runs anywhere
    cal = BeamCalibration(H, lr=1e-4)                    # the table as a parameter with its Adam; cal.table is the (H, 2) tensor
    table = load_table("beams300.pth" or "table.txt")    # (H, 2) float32

``beams`` is an ``(H, 2)`` tensor on the pose's device and of its dtype: row ``h`` holds ``(eps_h, delta_h)``, the elevation offset and the
azimuth offset of IMAGE ROW ``h`` in radians.  It is indexed by the image row; it is not flipped the way a per-beam inclination table is.  Row
``h``, column ``w`` looks along ``l = (cos e cos a, cos e sin a, sin e)`` with ``e`` = the nominal inclination of the row + ``eps_h`` and ``a`` =
the nominal azimuth of the column + ``delta_h``; everything else -- the column's pose ``pose @ Exp(tau[w] * twist)``, the origins, the
arguments and how they are checked -- is ``sweep.sweep_rays``'s.  The offsets say how a laser is mounted, not when it fires: a column's instant
stays ``tau[w]``.  ``include/lrt_beams.h`` states the rule; ``csrc/lrt_beams_math.h`` is its text for the device and the host.

* ``beam_rays``: HIP float32 tensors go through the library -- two launches forward, two backward, no host wait, no float atomics.  It is
  differentiable in ``pose``, ``twist`` and ``beams``; an output nobody asked for costs no reduction.  ``beams=None`` is ``sweep_rays``.  A row
  whose two offsets are exactly zero carries the bits of ``sweep_rays``.  A missing library is an error; CPU tensors go to the twin.
* ``beam_rays_reference(..., per_ray=True, g_o=..., g_d=...)`` also returns ``(F, H, W, 20)``: every ray's contribution to the 12 entries of
  ``d_pose``, the 6 of ``d_twist`` and the 2 of its row's ``d_beams``.
* The gauge: the same azimuth offset on every row is exactly a yaw of the sensor, so a table learnt beside the poses is determined only up to
  it.  ``BeamCalibration(zero_mean_azimuth=True)`` removes the mean of the azimuth column after every step.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import sweep as sw

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LRT_BEAMS_LIB") or os.path.join(HERE, "csrc", "liblrt_beams.so")
EXPORTS = ("lrt_beams_abi_version", "lrt_beams_last_error", "lrt_beams_work_bytes", "lrt_beams_rays", "lrt_beams_backward")     # include/lrt_beams.h
ABI_VERSION = 1

_lib = None


class BeamError(sw.SweepError):
    pass


def load():
    """Load liblrt_beams.so (after torch, so that both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BeamError(f"{LIB_PATH} is missing: build it with `python -m lidar_rt_amd.build` (hipcc --offload-arch=gfx950). "
                        "beam_rays has no fall-back on a HIP device.")
    lib = C.CDLL(LIB_PATH)
    lib.lrt_beams_abi_version.restype = C.c_int
    lib.lrt_beams_last_error.restype = C.c_char_p
    lib.lrt_beams_work_bytes.restype = C.c_longlong
    lib.lrt_beams_work_bytes.argtypes = [C.c_longlong, C.c_int, C.c_int]
    common = [C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    lib.lrt_beams_rays.restype = C.c_int
    lib.lrt_beams_rays.argtypes = common + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
    lib.lrt_beams_backward.restype = C.c_int
    lib.lrt_beams_backward.argtypes = common + [C.c_void_p] * 6 + [C.c_longlong, C.c_void_p]
    if lib.lrt_beams_abi_version() != ABI_VERSION:
        raise BeamError("liblrt_beams.so ABI version mismatch; rebuild with `python -m lidar_rt_amd.build --force`")
    _lib = lib
    return lib


def _check_table(beams, H, pose):
    """The table's shape, dtype and device, before anything runs."""
    if not torch.is_tensor(beams) or tuple(beams.shape) != (int(H), 2):
        raise BeamError(f"beam_rays: beams must be an ({int(H)}, 2) tensor, (elevation offset, azimuth offset) per image row "
                        f"(it is {tuple(beams.shape) if torch.is_tensor(beams) else type(beams).__name__})")
    if torch.is_tensor(pose) and (beams.device != pose.device or beams.dtype != pose.dtype):
        raise BeamError(f"beam_rays: beams ({beams.dtype}, {beams.device}) and pose ({pose.dtype}, {pose.device}) differ")
    return beams


# ---- the twin -----------------------------------------------------------------------------------------------------------------------------------------------

def _angles(H, W, inc, off, yaw, dev):
    """The nominal inclination (H,) and azimuth (W,), float64: the expressions of sweep._local."""
    w = torch.arange(W, dtype=torch.float64, device=dev)
    az = ((float(W) - w) - off) / float(W) * sw.TWO_PI - sw.PI - yaw
    inc = inc.to(device=dev, dtype=torch.float64)
    if inc.numel() == 2:
        h = torch.arange(H, dtype=torch.float64, device=dev)
        el = ((float(H) - h) - off) / float(H) * (inc[1] - inc[0]) + inc[0]
    else:
        el = inc.flip(0)
    return el, az


def beam_rays_reference(pose, twist, H, W, inclination, beams, data_type="KITTI", sensor2ego=None, tau=None, t_ref=0.5, per_ray=False, g_o=None, g_d=None):
    """The float64 torch twin (see the module text): (ray_o, ray_d) float64 on the pose's device, differentiable in pose, twist and beams; the
    angle sums are taken as they are written.  With ``per_ray=True`` (and upstream gradients ``g_o``, ``g_d``) a third result (F, H, W, 20):
    each ray's contribution to d_pose (12), d_twist (6) and the d_beams (2) of its row."""
    if beams is None:
        return sw.sweep_rays_reference(pose, twist, H, W, inclination, data_type, sensor2ego, tau, t_ref, per_ray, g_o, g_d)
    P, xi, batched, H, W, inc, tau, off, yaw = sw._arguments(pose, twist, H, W, inclination, data_type, sensor2ego, tau, t_ref, pose.device if torch.is_tensor(pose) else None)
    _check_table(beams, H, pose)
    dev = P.device
    F = P.shape[0]
    el, az = _angles(H, W, inc, off, yaw, dev)
    s = tau.to(device=dev, dtype=torch.float64)[None, None, :]
    P64 = P.to(torch.float64)
    x64 = None if xi is None else xi.to(torch.float64)

    def rays(Pb, xb, b64):                                                  # b64 (H, 2) or (F, H, W, 2)
        e = el[:, None] + b64[..., 0:1] if b64.dim() == 2 else el[None, :, None] + b64[..., 0]
        a = az[None, :] + b64[..., 1:2] if b64.dim() == 2 else az[None, None, :] + b64[..., 1]
        if b64.dim() == 2:
            e, a = e[None], a[None]                                         # (1, H, 1), (1, H, W)
        return sw._rays64(Pb, xb, s if b64.dim() == 2 else s.expand(F, H, W), torch.cos(e), torch.sin(e), torch.cos(a), torch.sin(a))

    t, d = rays(P64[:, None, None], None if x64 is None else x64[:, None, None], beams.to(torch.float64))
    o = t.expand(F, H, W, 3)
    d = d.expand(F, H, W, 3)
    sq = (lambda a: a) if batched else (lambda a: a[0])
    if not per_ray:
        return sq(o), sq(d)
    if g_o is None or g_d is None:
        raise BeamError("beam_rays_reference: per_ray=True needs the upstream gradients g_o and g_d")
    with torch.enable_grad():
        Pe = P64.detach()[:, None, None].expand(F, H, W, 3, 4).clone().requires_grad_(True)
        xe = None if x64 is None else x64.detach()[:, None, None].expand(F, H, W, 6).clone().requires_grad_(True)
        be = beams.detach().to(torch.float64)[None, :, None, :].expand(F, H, W, 2).clone().requires_grad_(True)
        te, de = rays(Pe, xe, be)
        go = g_o.detach().to(device=dev, dtype=torch.float64).reshape(F, H, W, 3)
        gd = g_d.detach().to(device=dev, dtype=torch.float64).reshape(F, H, W, 3)
        ((te.expand(F, H, W, 3) * go).sum() + (de * gd).sum()).backward()
    gx = torch.zeros((F, H, W, 6), dtype=torch.float64, device=dev) if xe is None else xe.grad
    contrib = torch.cat([Pe.grad.reshape(F, H, W, 12), gx, be.grad], -1)
    return sq(o.detach()), sq(d.detach()), sq(contrib)


# ---- the operator ---------------------------------------------------------------------------------------------------------------------------------------------

def work_bytes(F: int, H: int, W: int) -> int:
    """Bytes of the workspace of one call: the column and row tables, the workgroups' partial sums and the rows' partial sums."""
    n = int(load().lrt_beams_work_bytes(int(F), int(H), int(W)))
    if n < 0:
        raise BeamError(f"beam_rays: {F} frames of {H} x {W} rays (each at least 1, F H W at most {sw.MAX_RAYS})")
    return n


def _workspace(workspace, nbytes, dev):
    if workspace is None:
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)              # the caching allocator's blocks are 512-byte aligned
    if not (torch.is_tensor(workspace) and workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.device == dev
            and workspace.numel() >= nbytes and workspace.data_ptr() % 256 == 0):
        raise BeamError(f"lrt_beams: the workspace must be a contiguous uint8 tensor of at least {nbytes} bytes on {dev}, 256-byte aligned")
    return workspace


class _BeamRays(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pose, twist, beams, inc, tau, H, W, off, yaw, workspace):
        lib = load()
        dev = pose.device
        F = pose.shape[0]
        P = pose.detach().contiguous()
        xi = None if twist is None else twist.detach().contiguous()
        tab = beams.detach().contiguous()
        ws = _workspace(workspace, work_bytes(F, H, W), dev)
        ray_o = torch.empty((F, H, W, 3), dtype=torch.float32, device=dev)
        ray_d = torch.empty((F, H, W, 3), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = lib.lrt_beams_rays(dev.index, F, H, W, P.data_ptr(), None if xi is None else xi.data_ptr(), inc.data_ptr(), inc.numel(), off, yaw,
                                    tau.data_ptr(), tab.data_ptr(), ray_o.data_ptr(), ray_d.data_ptr(), ws.data_ptr(), ws.numel(),
                                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc != 0:
            raise BeamError(f"lrt_beams_rays failed ({rc}): {lib.lrt_beams_last_error().decode()}")
        ctx.save_for_backward(P, xi, tab, inc, tau)
        ctx.args = (H, W, off, yaw, workspace)
        return ray_o, ray_d

    @staticmethod
    def backward(ctx, g_o, g_d):
        lib = load()
        P, xi, tab, inc, tau = ctx.saved_tensors
        H, W, off, yaw, workspace = ctx.args
        dev = P.device
        F = P.shape[0]
        want_pose = ctx.needs_input_grad[0] or (xi is not None and ctx.needs_input_grad[1])
        want_beams = ctx.needs_input_grad[2]
        g_o, g_d = g_o.to(torch.float32).contiguous(), g_d.to(torch.float32).contiguous()
        ws = _workspace(workspace, work_bytes(F, H, W), dev)
        d_pose = torch.empty((F, 3, 4), dtype=torch.float32, device=dev) if want_pose else None
        d_twist = torch.empty((F, 6), dtype=torch.float32, device=dev) if want_pose and xi is not None else None
        d_beams = torch.empty((H, 2), dtype=torch.float32, device=dev) if want_beams else None
        ptr = lambda t: None if t is None else t.data_ptr()
        with torch.cuda.device(dev):
            rc = lib.lrt_beams_backward(dev.index, F, H, W, P.data_ptr(), ptr(xi), inc.data_ptr(), inc.numel(), off, yaw, tau.data_ptr(), tab.data_ptr(),
                                        g_o.data_ptr(), g_d.data_ptr(), ptr(d_pose), ptr(d_twist), ptr(d_beams), ws.data_ptr(), ws.numel(),
                                        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc != 0:
            raise BeamError(f"lrt_beams_backward failed ({rc}): {lib.lrt_beams_last_error().decode()}")
        return (d_pose if ctx.needs_input_grad[0] else None, d_twist if ctx.needs_input_grad[1] else None, d_beams) + (None,) * 7


def beam_rays(pose, twist, H, W, inclination, beams, data_type="KITTI", sensor2ego=None, tau=None, t_ref=0.5, workspace=None):
    """The beam rays of F frames (see the module text): (ray_o, ray_d), each (F, H, W, 3) float32, or (H, W, 3) for an unbatched pose.
    ``beams``: (H, 2) on the pose's device and of its dtype, or ``None`` for the sweep rays.  ``workspace``: a uint8 tensor on the pose's device
    of at least ``work_bytes(F, H, W)`` bytes to use instead of a fresh one, forward and backward; its contents do not matter."""
    if beams is None:
        return sw.sweep_rays(pose, twist, H, W, inclination, data_type, sensor2ego, tau, t_ref, workspace)
    dev = pose.device if torch.is_tensor(pose) else None
    P, xi, batched, H, W, inc, tau, off, yaw = sw._arguments(pose, twist, H, W, inclination, data_type, sensor2ego, tau, t_ref, dev)
    _check_table(beams, H, pose)
    if dev.type != "cuda":
        if workspace is not None:
            raise BeamError(f"beam_rays: a workspace with a pose on {dev}")
        o, d = beam_rays_reference(pose, twist, H, W, inc, beams, data_type, sensor2ego, tau)
        return o.to(torch.float32).contiguous(), d.to(torch.float32).contiguous()
    load()
    if P.dtype != torch.float32:
        raise BeamError(f"lrt_beams: pose, twist and beams must be float32 tensors (they are {P.dtype}); there is no fall-back to PyTorch on a HIP device")
    o, d = _BeamRays.apply(P.contiguous(), None if xi is None else xi.contiguous(), beams, sw._upload(inc, dev), sw._upload(tau, dev), H, W, off, yaw, workspace)
    return (o, d) if batched else (o[0], d[0])


# ---- the table as a parameter -----------------------------------------------------------------------------------------------------------------------------------

def load_table(path, H=None, device="cpu") -> torch.Tensor:
    """(H, 2) float32 from a file BeamCalibration.save wrote, or from a text table with one ``eps delta`` pair per line (radians)."""
    try:
        sd = torch.load(path, map_location="cpu", weights_only=False)
        t = sd["beams"] if isinstance(sd, dict) else sd
    except Exception:
        try:
            t = torch.as_tensor(np.loadtxt(path, dtype=np.float64, ndmin=2))
        except (OSError, ValueError) as e:
            raise BeamError(f"load_table: {path} is neither a beams<it>.pth nor a text table of `eps delta` rows: {e}") from None
    t = torch.as_tensor(t).detach().to(torch.float32)
    if t.dim() != 2 or t.shape[1] != 2 or (H is not None and t.shape[0] != int(H)):
        raise BeamError(f"load_table: {path} holds a table of shape {tuple(t.shape)}" + (f", the images have {int(H)} rows" if H is not None else " (it must be (H, 2))"))
    return t.contiguous().to(device)


@torch.no_grad()
def apply_table(frames, table, frame_ids=None):
    """Put a fixed table into a ``RangeFrames``: the stored rays of every listed frame (default: all) are replaced by its beam rays -- the frame's
    pose, its twist and column times if it has them, the table.  For the renders of evaluate and simulate and for synthetic ground truth; every
    frame must have been added with ``add_range_image``."""
    from .poses import SensorPoses
    ids = [f for f in (frames.rays if frame_ids is None else frame_ids)]
    sensor = SensorPoses(frames, ids, beams=table, fixed_poses=True)
    for f in ids:
        o, d = sensor.get_range_rays(f)
        frames.rays[f] = (o.detach().contiguous(), d.detach().contiguous())
    return frames


class BeamCalibration:
    """One (H, 2) parameter -- zero, or ``init`` -- with Adam (betas (0.9, 0.999), eps 1e-15, learning rate ``lr`` in radians).
    ``zero_mean_azimuth``: ``step()`` subtracts the mean of the azimuth column afterwards (the gauge a learnt yaw leaves open)."""

    def __init__(self, H, init=None, lr: float = 1e-4, zero_mean_azimuth: bool = False, device="cpu"):
        if not (isinstance(H, (int, np.integer)) and H >= 1):
            raise BeamError(f"BeamCalibration: {H!r} rows")
        if init is None:
            t = torch.zeros((int(H), 2), dtype=torch.float32, device=device)
        else:
            t = torch.as_tensor(init).detach()
            if tuple(t.shape) != (int(H), 2):
                raise BeamError(f"BeamCalibration: init must be ({int(H)}, 2) (it is {tuple(t.shape)})")
            t = t.to(device=device, dtype=torch.float32).clone()
        self.H = int(H)
        self.table = torch.nn.Parameter(t.contiguous())
        self.lr = float(lr)
        self.zero_mean_azimuth = bool(zero_mean_azimuth)
        self.optimizer = torch.optim.Adam([{"params": [self.table], "lr": self.lr, "name": "beams"}], betas=(0.9, 0.999), eps=1e-15)

    def zero_grad(self):
        self.optimizer.zero_grad(set_to_none=True)

    @torch.no_grad()
    def step(self):
        self.optimizer.step()
        if self.zero_mean_azimuth:
            col = self.table[:, 1].to(torch.float64)
            self.table[:, 1] = (col - col.mean()).to(torch.float32)

    def state_dict(self):
        return {"beams": self.table.detach().cpu().clone(), "optimizer": self.optimizer.state_dict(), "lr": self.lr, "zero_mean_azimuth": self.zero_mean_azimuth}

    def load_state_dict(self, sd):
        t = torch.as_tensor(sd["beams"])
        if tuple(t.shape) != (self.H, 2):
            raise BeamError(f"BeamCalibration: the state dict's table is {tuple(t.shape)}, this one ({self.H}, 2)")
        with torch.no_grad():
            self.table.copy_(t.to(device=self.table.device, dtype=torch.float32))
        import copy
        self.optimizer.load_state_dict(copy.deepcopy(sd["optimizer"]))     # a live state dict shares its moment tensors with the optimizer it came from
        self.lr = float(sd.get("lr", self.lr))
        for g in self.optimizer.param_groups:
            g["lr"] = self.lr

    def save(self, path):
        """The table and the optimizer state, nothing else."""
        torch.save(self.state_dict(), path)

    def load(self, path):
        self.load_state_dict(torch.load(path, map_location=self.table.device, weights_only=False))
