"""Actors that move within a sweep: every Gaussian of a moving actor at the instant the sweep passes over it, through ``csrc/liblrt_actorsweep.so``.

    xyz_s, rot_s, info = actor_sweep(xyz, rot_raw, seg_start, poses, actor_twist, sensor_pose, sensor_twist, tau, W, data_type="KITTI", sensor2ego=None)
    twin = actor_sweep_reference(...)                    # the float64 torch twin: xyz_s, rot_s (un-rounded), column, counts, evals, margin, ...
    eta = actor_twists_from_boxes(boxes, frame_ids)      # per actor {frame: (6,) float64}: Log(A_f^-1 A_f') * sweep_fraction / (f' - f)

Over one sweep an actor moves as ``A(s) = A Exp(s eta)``: ``A`` the tracking-box pose at the frame's reference instant (the ``poses`` row of
``preprocess.pack_poses``), ``eta = (rho, phi)`` its twist over one whole sweep in its OWN frame (the convention of ``sweep.py`` and
``poses.se3_exp``), ``s`` in sweeps.  A Gaussian is placed where it is when the sweep passes over its centre: ``s* = tau[w*]``, ``w*`` the column
that, at its own instant, has the centre inside its azimuth bin.  ``include/lrt_actorsweep.h`` states the rule; ``csrc/lrt_actorsweep_math.h``
is its text for the device and the host, all of it float64.  The operator is a stage IN FRONT of ``preprocess.fused_activations``: it maps
actor-local parameters to actor-local parameters, ``xyz_s = R_E x + t_E`` and ``rot_s = q_E (x) normalize(rot_raw)`` with ``E = Exp(s* eta)``.

* ``xyz (P, 3)``, ``rot_raw (P, 4)``, ``seg_start (A + 1,) int32``, ``poses (A, 8)``: what ``fused_activations`` takes.  ``actor_twist (A, 6)``.
* ``sensor_pose`` ``(3, 4)`` / ``(4, 4)`` and ``sensor_twist`` ``(6,)`` or ``None`` (a static sensor), ``poses``: read detached, they only steer
  the search.  ``tau (W,)``: the column times (``sweep.column_times``), read as float64.  Host data or tensors on the Gaussians' device.
* Pass-through is bit for bit (``rot_raw`` NOT normalised): every Gaussian of an unposed asset or of an asset whose twist row is all zeros
  (column -1), and every Gaussian whose ``tau[w*] * eta`` is zero (it records its column).  With all twists zero nothing changes.
* ``info.column (P,) int32`` and ``info.counts (4,) int64`` = moved, passed, unconverged, invalid (``COUNT_NAMES``) stay on the device: no wait.
* ``w*`` is an integer and ``tau`` a table: the instants are piecewise constant, so the backward treats them as constants, exactly.
* ``actor_sweep``: HIP float32 tensors go through the library -- two launches forward, two backward, no host wait, equal bits for equal inputs.
  It is differentiable in ``xyz``, ``rot_raw`` and ``actor_twist``.  A missing library is an ``ActorSweepError``: there is no quiet fall-back.
  CPU tensors go to the twin.
* ``actor_sweep_reference(..., column=...)`` freezes the columns (no search); ``g_xyz=..., g_rot=...`` adds ``contrib (P, 6)``: every
  Gaussian's term of ``d_actor_twist`` for those upstream gradients.  ``margin``: the smallest distance of ANY evaluated column coordinate ``u``
  from a rounding boundary, as ``sweep_project``'s twin reports it.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import sweep

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LRT_ACTORSWEEP_LIB") or os.path.join(HERE, "csrc", "liblrt_actorsweep.so")
EXPORTS = ("lrt_actorsweep_abi_version", "lrt_actorsweep_last_error", "lrt_actorsweep_work_bytes", "lrt_actorsweep_forward",
           "lrt_actorsweep_backward")                                        # include/lrt_actorsweep.h
ABI_VERSION = 1
N_COUNTS = 4                                                                 # LRT_ACTORSWEEP_N_COUNTS
MAX_EVAL = 8                                                                 # LRT_ACTORSWEEP_MAX_EVAL
TABLE = 12                                                                   # LRT_ACTORSWEEP_TABLE
BLOCK = 256                                                                  # LRT_ACTORSWEEP_BLOCK
MAX_POINTS = 2 ** 30                                                         # LRT_ACTORSWEEP_MAX_POINTS
MAX_ASSETS = 2 ** 20                                                         # LRT_ACTORSWEEP_MAX_ASSETS
MAX_COLUMNS = 2 ** 20                                                        # LRT_ACTORSWEEP_MAX_COLUMNS
NORM_EPS = 1e-12                                                             # AS_NORM_EPS
COUNT_NAMES = ("moved", "passed", "unconverged", "invalid")
CONVERGED, UNCONVERGED, INVALID, NOT_SEARCHED = 0, 1, 2, 3                   # AS_CONVERGED .. AS_INVALID; 3: an unposed or zero-twist asset

_lib = None


class ActorSweepError(RuntimeError):
    pass


def load():
    """Load liblrt_actorsweep.so (after torch, so that both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ActorSweepError(f"{LIB_PATH} is missing: build it with `python -m lidar_rt_amd.build` (hipcc --offload-arch=gfx950). "
                              "actor_sweep has no fall-back on a HIP device.")
    lib = C.CDLL(LIB_PATH)
    lib.lrt_actorsweep_abi_version.restype = C.c_int
    lib.lrt_actorsweep_last_error.restype = C.c_char_p
    lib.lrt_actorsweep_work_bytes.restype = C.c_longlong
    lib.lrt_actorsweep_work_bytes.argtypes = [C.c_longlong, C.c_int, C.c_int]
    lib.lrt_actorsweep_forward.restype = C.c_int
    lib.lrt_actorsweep_forward.argtypes = [C.c_int, C.c_longlong, C.c_int] + [C.c_void_p] * 8 + [C.c_int, C.c_double, C.c_double] + [C.c_void_p] * 5 \
        + [C.c_longlong, C.c_void_p]
    lib.lrt_actorsweep_backward.restype = C.c_int
    lib.lrt_actorsweep_backward.argtypes = [C.c_int, C.c_longlong, C.c_int] + [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 7 + [C.c_longlong, C.c_void_p]
    if lib.lrt_actorsweep_abi_version() != ABI_VERSION:
        raise ActorSweepError("liblrt_actorsweep.so ABI version mismatch; rebuild with `python -m lidar_rt_amd.build --force`")
    _lib = lib
    return lib


# ---- the arguments ------------------------------------------------------------------------------------------------------------------------------------------

def _side(name, x, shape_ok, dev, dtype=torch.float64):
    """A small steering argument as a detached tensor of ``dtype`` on ``dev``: host data is uploaded without a wait, a tensor on ``dev`` is converted there."""
    if torch.is_tensor(x):
        t = x.detach()
        if t.device.type != "cpu" and t.device != dev:
            raise ActorSweepError(f"actor_sweep: {name} on {t.device} (host data or a tensor on {dev})")
    else:
        try:
            t = torch.as_tensor(np.asarray(x, dtype=np.float64))
        except (TypeError, ValueError) as e:
            raise ActorSweepError(f"actor_sweep: {name} is not numeric: {e}") from None
    if tuple(t.shape) not in shape_ok:
        raise ActorSweepError(f"actor_sweep: {name} must be {' or '.join(str(s) for s in shape_ok)} (it is {tuple(t.shape)})")
    t = t.to(dtype)
    return t if t.device == dev else sweep._upload(t, dev)


def world2sensor(pose: torch.Tensor) -> torch.Tensor:
    """(3, 4): the inverse of a rigid pose [R | t], [R^T | -(R^T t)], every entry by elementwise operations summed left to right (so that the host
    and the device give the same bits)."""
    R, t = pose[:3, :3], pose[:3, 3]
    rows = []
    for i in range(3):
        rows.append(torch.stack([R[0, i], R[1, i], R[2, i], -(R[0, i] * t[0] + R[1, i] * t[1] + R[2, i] * t[2])]))
    return torch.stack(rows)


def _arguments(xyz, rot_raw, seg_start, poses, actor_twist, sensor_pose, sensor_twist, tau, W, data_type, sensor2ego):
    for name, t, last in (("xyz", xyz, 3), ("rot_raw", rot_raw, 4), ("poses", poses, 8), ("actor_twist", actor_twist, 6)):
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != last:
            raise ActorSweepError(f"actor_sweep: {name} must be a (N, {last}) tensor (it is {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__})")
    dev = xyz.device
    P, A = xyz.shape[0], poses.shape[0]
    if rot_raw.shape[0] != P:
        raise ActorSweepError(f"actor_sweep: {P} centres and {rot_raw.shape[0]} rotations")
    if A < 1 or A > MAX_ASSETS or actor_twist.shape[0] != A:
        raise ActorSweepError(f"actor_sweep: {A} pose rows (1 .. {MAX_ASSETS}) and {actor_twist.shape[0]} twist rows")
    if P > MAX_POINTS:
        raise ActorSweepError(f"actor_sweep: {P} Gaussians (0 .. {MAX_POINTS})")
    if not (isinstance(W, (int, np.integer)) and 1 <= W <= MAX_COLUMNS):
        raise ActorSweepError(f"actor_sweep: {W!r} columns (1 .. {MAX_COLUMNS})")
    W = int(W)
    if not torch.is_tensor(seg_start) or seg_start.dtype != torch.int32 or tuple(seg_start.shape) != (A + 1,):
        raise ActorSweepError(f"actor_sweep: seg_start must be a ({A + 1},) int32 tensor (preprocess.pack_poses)")
    for name, t in (("rot_raw", rot_raw), ("seg_start", seg_start), ("poses", poses), ("actor_twist", actor_twist)):
        if t.device != dev:
            raise ActorSweepError(f"actor_sweep: {name} is on {t.device}, xyz on {dev}")
    try:
        off, yaw = sweep.convention(data_type, sensor2ego)
    except sweep.SweepError as e:
        raise ActorSweepError(f"actor_sweep: {e}") from None
    P64 = _side("sensor_pose", sensor_pose, ((3, 4), (4, 4)), dev)
    xi = None if sensor_twist is None else _side("sensor_twist", sensor_twist, ((6,),), dev)
    tau = _side("tau", tau, ((W,),), dev)
    return dev, P, A, W, off, yaw, world2sensor(P64).contiguous(), xi, tau.contiguous()


# ---- the twin -----------------------------------------------------------------------------------------------------------------------------------------------

def _rigid(R, t, x):
    """R x + t on batches, each row summed left to right (as_rigid)."""
    return torch.stack([R[..., i, 0] * x[..., 0] + R[..., i, 1] * x[..., 1] + R[..., i, 2] * x[..., 2] + t[..., i] for i in range(3)], -1)


def _pose_table(poses, dtype):
    """as_pose: (Ra (A, 3, 3), ta (A, 3), posed (A,)) of the pose rows, the quaternion normalised as build_rotation does."""
    p = poses.detach().to(dtype)
    q0, q1, q2, q3 = p[:, 3], p[:, 4], p[:, 5], p[:, 6]
    n = torch.sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3)
    r, x, y, z = q0 / n, q1 / n, q2 / n, q3 / n
    R = torch.stack([1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - r * z), 2.0 * (x * z + r * y),
                     2.0 * (x * y + r * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - r * x),
                     2.0 * (x * z - r * y), 2.0 * (y * z + r * x), 1.0 - 2.0 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    return R, p[:, :3], poses.detach()[:, 7] != 0


def column_table(w2s, xi, tau):
    """(W, 3, 4): world -> the sensor frame of every column, as_table_entry; an E_w that is exactly the identity keeps ``w2s``.  Any float dtype."""
    W = tau.numel()
    if xi is None:
        return w2s[None].expand(W, 3, 4)
    Re, te = sweep._exp64(tau[:, None] * xi[None, :])
    Ri = Re.transpose(-1, -2)
    ti = torch.stack([-(Re[:, 0, i] * te[:, 0] + Re[:, 1, i] * te[:, 1] + Re[:, 2, i] * te[:, 2]) for i in range(3)], -1)
    ident = (Ri == torch.eye(3, dtype=w2s.dtype, device=w2s.device)).all(-1).all(-1) & (ti == 0).all(-1)
    rows = []
    for i in range(3):
        row = [Ri[:, i, 0] * w2s[0, j] + Ri[:, i, 1] * w2s[1, j] + Ri[:, i, 2] * w2s[2, j] for j in range(3)]
        row.append(Ri[:, i, 0] * w2s[0, 3] + Ri[:, i, 1] * w2s[1, 3] + Ri[:, i, 2] * w2s[2, 3] + ti[:, i])
        rows.append(torch.stack(row, -1))
    T = torch.stack(rows, -2)
    return torch.where(ident[:, None, None], w2s[None].expand(W, 3, 4), T)


def _u_of(q, W, off, yaw):
    return (sweep.PI - (torch.atan2(q[:, 1], q[:, 0]) + yaw)) * float(W) / sweep.TWO_PI - off


def _column_of(c, W):
    """sp_column_of with the wrap: a rounded u as a column of [0, W)."""
    Wf = float(W)
    c = c - torch.floor(c / Wf) * Wf
    return torch.where((c >= 0.0) & (c < Wf), c, torch.zeros_like(c)).to(torch.int64)


def asset_of(seg_start, P, A):
    """(P,) int64: the asset of every Gaussian, the last a of [0, A) with seg_start[a] <= g."""
    g = torch.arange(P, dtype=torch.int64, device=seg_start.device)
    return (torch.searchsorted(seg_start.to(torch.int64)[:A].contiguous(), g, right=True) - 1).clamp_(0, A - 1)


@torch.no_grad()
def search(x, asset, Ra, ta, posed, eta, w2s, table, tau, W, off, yaw, with_margin=True):
    """as_search, vectorised over the Gaussians in the dtype of ``x``: MAX_EVAL rounds over those still searching.
    -> (column (P,) int64, -1 where there is none; state (P,); evals (P,); margin)."""
    P = x.shape[0]
    dev = x.device
    column = torch.full((P,), -1, dtype=torch.int64, device=dev)
    state = torch.full((P,), NOT_SEARCHED, dtype=torch.int64, device=dev)
    evals = torch.zeros(P, dtype=torch.int64, device=dev)
    live = (posed & (eta != 0).any(-1))[asset]
    idx = torch.nonzero(live)[:, 0]
    margins = [float("inf")]
    usable = lambda q: torch.isfinite(q).all(-1) & ~((q[:, 0] == 0) & (q[:, 1] == 0))

    def coordinate(q):
        u = _u_of(q, W, off, yaw)
        if with_margin and u.numel():
            margins.append(float(((u - torch.round(u)).abs() - 0.5).abs().min()))
        return _column_of(torch.round(u), W)
    a = asset[idx]
    q = _rigid(w2s[None, :, :3], w2s[None, :, 3], _rigid(Ra[a], ta[a], x[idx]))
    ok = usable(q)
    state[idx[~ok]] = INVALID
    idx, q = idx[ok], q[ok]
    col = coordinate(q)
    state[idx] = UNCONVERGED
    for k in range(MAX_EVAL):
        if idx.numel() == 0:
            break
        a = asset[idx]
        xs = tau[col][:, None] * eta[a]
        Re, te = sweep._exp64(xs)
        e = torch.where((xs != 0).any(-1)[:, None], _rigid(Re, te, x[idx]), x[idx])
        T = table[col]
        q = _rigid(T[:, :, :3], T[:, :, 3], _rigid(Ra[a], ta[a], e))
        evals[idx] += 1
        ok = usable(q)
        state[idx[~ok]] = INVALID
        idx, q, col = idx[ok], q[ok], col[ok]
        nxt = coordinate(q)
        same = nxt == col
        state[idx[same]] = CONVERGED
        column[idx[same]] = col[same]
        if k + 1 == MAX_EVAL:
            column[idx[~same]] = col[~same]                                   # the LAST evaluated column
        idx, col = idx[~same], nxt[~same]
    return column, state, evals, min(margins)


def _half_coef(u):
    """(cos t, sin t / t) at u = t^2: the series below SERIES_TH2 (as_half_coef)."""
    small = u < sweep.SERIES_TH2
    us = torch.where(small, torch.ones_like(u), u)
    t = torch.sqrt(us)
    return torch.where(small, sweep._nested(u, -1), torch.cos(t)), torch.where(small, sweep._nested(u, 0), torch.sin(t) / t)


def place(x, r, eta_g, s, searched):
    """as_place on batches, autograd-able: (xyz_s, rot_s, moved, parts).  x (P, 3), r (P, 4), eta_g (P, 6), s (P,); ``searched``: the rows that
    have a column.  Rows that do not move return x and r themselves."""
    xs = s[:, None] * eta_g
    moved = searched & (xs.detach() != 0).any(-1)
    Re, te = sweep._exp64(xs)
    e = _rigid(Re, te, x)
    phi = xs[:, 3:]
    c, a = _half_coef(0.25 * (phi[:, 0] * phi[:, 0] + phi[:, 1] * phi[:, 1] + phi[:, 2] * phi[:, 2]))
    qe = torch.cat([c[:, None], 0.5 * a[:, None] * phi], 1)
    n = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    b = r / n.clamp(min=NORM_EPS)[:, None]
    aw, ax, ay, az = qe.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    out = torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                       aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)
    parts = SimpleNamespace(Re=Re.detach(), te=te.detach(), qe=qe.detach(), b=b.detach(), n=n.detach())
    return torch.where(moved[:, None], e, x), torch.where(moved[:, None], out, r), moved, parts


def actor_sweep_reference(xyz, rot_raw, seg_start, poses, actor_twist, sensor_pose, sensor_twist, tau, W, data_type="KITTI", sensor2ego=None, column=None,
                          g_xyz=None, g_rot=None, dtype=torch.float64, with_margin=True):
    """The float64 torch twin (see the module text), on the device of ``xyz``.  ``xyz_s`` and ``rot_s`` are NOT rounded to float32 and carry the
    graph of ``xyz``, ``rot_raw`` and ``actor_twist``; the columns are detached.  ``dtype``: the arithmetic's (float32 for the benchmark tool)."""
    dev, P, A, W, off, yaw, w2s, xi, tau = _arguments(xyz, rot_raw, seg_start, poses, actor_twist, sensor_pose, sensor_twist, tau, W, data_type, sensor2ego)
    w2s, tau = w2s.to(dtype), tau.to(dtype)
    xi = None if xi is None else xi.to(dtype)
    x, r, eta = xyz.to(dtype), rot_raw.to(dtype), actor_twist.to(dtype)
    asset = asset_of(seg_start, P, A)
    Ra, ta, posed = _pose_table(poses, dtype)
    if column is None:
        column, state, evals, margin = search(x.detach(), asset, Ra, ta, posed, eta.detach(), w2s, column_table(w2s, xi, tau), tau, W, off, yaw, with_margin)
    else:
        column = column.to(device=dev, dtype=torch.int64)
        state = evals = None
        margin = float("inf")
    searched = (column >= 0) & (column < W)
    s = tau[column.clamp(0, W - 1)]
    xyz_s, rot_s, moved, parts = place(x, r, eta[asset], s, searched)
    out = SimpleNamespace(xyz_s=xyz_s, rot_s=rot_s, column=column.to(torch.int32), moved=moved, state=state, evals=evals, margin=margin, asset=asset, s=s, parts=parts)
    if state is not None:
        out.counts = torch.stack([moved.sum(), (~moved).sum(), (state == UNCONVERGED).sum(), (state == INVALID).sum()]).to(torch.int64)
    if g_xyz is not None or g_rot is not None:
        with torch.enable_grad():
            leaf = eta.detach()[asset].clone().requires_grad_(True)
            xs_, rs_, _, _ = place(x.detach(), r.detach(), leaf, s, searched)
            (xs_ * g_xyz.detach().to(device=dev, dtype=dtype)).sum().add((rs_ * g_rot.detach().to(device=dev, dtype=dtype)).sum()).backward()
        out.contrib = leaf.grad
    return out


# ---- the operator ---------------------------------------------------------------------------------------------------------------------------------------------

def work_bytes(P: int, A: int, W: int) -> int:
    """Bytes of the workspace of one call: the column table and the backward's partial sums."""
    n = int(load().lrt_actorsweep_work_bytes(int(P), int(A), int(W)))
    if n < 0:
        raise ActorSweepError(f"actor_sweep: {P} Gaussians in {A} assets under {W} columns (at most {MAX_POINTS}, 1 .. {MAX_ASSETS}, 1 .. {MAX_COLUMNS})")
    return n


def _workspace(workspace, nbytes, dev):
    if workspace is None:
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)              # the caching allocator's blocks are 512-byte aligned
    if not (torch.is_tensor(workspace) and workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.device == dev
            and workspace.numel() >= nbytes and workspace.data_ptr() % 256 == 0):
        raise ActorSweepError(f"lrt_actorsweep: the workspace must be a contiguous uint8 tensor of at least {nbytes} bytes on {dev}, 256-byte aligned")
    return workspace


class _ActorSweep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, rot_raw, actor_twist, seg, poses, w2s, xi, tau, W, off, yaw, workspace):
        lib = load()
        dev = xyz.device
        P, A = xyz.shape[0], poses.shape[0]
        x, r, eta, pz = xyz.detach().contiguous(), rot_raw.detach().contiguous(), actor_twist.detach().contiguous(), poses.detach().contiguous()
        ws = _workspace(workspace, work_bytes(P, A, W), dev)
        xyz_s, rot_s = torch.empty_like(x), torch.empty_like(r)
        column = torch.empty((P,), dtype=torch.int32, device=dev)
        counts = torch.empty((N_COUNTS,), dtype=torch.int64, device=dev)
        ptr = lambda t: t.data_ptr() if t.numel() else None
        with torch.cuda.device(dev):
            rc = lib.lrt_actorsweep_forward(dev.index, P, A, ptr(x), ptr(r), seg.data_ptr(), pz.data_ptr(), eta.data_ptr(), w2s.data_ptr(),
                                            None if xi is None else xi.data_ptr(), tau.data_ptr(), W, off, yaw, ptr(xyz_s), ptr(rot_s), ptr(column),
                                            counts.data_ptr(), ws.data_ptr(), ws.numel(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc != 0:
            raise ActorSweepError(f"lrt_actorsweep_forward failed ({rc}): {lib.lrt_actorsweep_last_error().decode()}")
        ctx.save_for_backward(x, r, eta, seg, pz, tau, column)
        ctx.args = (W, workspace)
        ctx.mark_non_differentiable(column, counts)
        return xyz_s, rot_s, column, counts

    @staticmethod
    def backward(ctx, g_xyz, g_rot, _g_column, _g_counts):
        lib = load()
        x, r, eta, seg, pz, tau, column = ctx.saved_tensors
        W, workspace = ctx.args
        dev = x.device
        P, A = x.shape[0], pz.shape[0]
        g_xyz, g_rot = g_xyz.to(torch.float32).contiguous(), g_rot.to(torch.float32).contiguous()
        ws = _workspace(workspace, work_bytes(P, A, W), dev)
        d_xyz, d_rot = torch.empty_like(x), torch.empty_like(r)
        d_twist = torch.empty_like(eta)
        ptr = lambda t: t.data_ptr() if t.numel() else None
        with torch.cuda.device(dev):
            rc = lib.lrt_actorsweep_backward(dev.index, P, A, ptr(x), ptr(r), seg.data_ptr(), pz.data_ptr(), eta.data_ptr(), tau.data_ptr(), W, ptr(column),
                                             ptr(g_xyz), ptr(g_rot), ptr(d_xyz), ptr(d_rot), d_twist.data_ptr(), ws.data_ptr(), ws.numel(),
                                             C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc != 0:
            raise ActorSweepError(f"lrt_actorsweep_backward failed ({rc}): {lib.lrt_actorsweep_last_error().decode()}")
        return d_xyz, d_rot, d_twist, None, None, None, None, None, None, None, None, None


def actor_sweep(xyz, rot_raw, seg_start, poses, actor_twist, sensor_pose, sensor_twist, tau, W, data_type="KITTI", sensor2ego=None, workspace=None):
    """(xyz_s (P, 3), rot_s (P, 4), info) (see the module text).  ``workspace``: a uint8 tensor on the Gaussians' device of at least
    ``work_bytes(P, A, W)`` bytes to use instead of a fresh one, forward and backward; its contents do not matter."""
    dev, P, A, W, off, yaw, w2s, xi, tau64 = _arguments(xyz, rot_raw, seg_start, poses, actor_twist, sensor_pose, sensor_twist, tau, W, data_type, sensor2ego)
    if dev.type != "cuda":
        if workspace is not None:
            raise ActorSweepError(f"actor_sweep: a workspace with Gaussians on {dev}")
        t = actor_sweep_reference(xyz, rot_raw, seg_start, poses, actor_twist, sensor_pose, sensor_twist, tau, W, data_type, sensor2ego)
        # the rows that pass keep their bits: float32 -> float64 -> float32 is exact
        return t.xyz_s.to(xyz.dtype), t.rot_s.to(rot_raw.dtype), SimpleNamespace(column=t.column, counts=t.counts)
    load()
    for name, t in (("xyz", xyz), ("rot_raw", rot_raw), ("poses", poses), ("actor_twist", actor_twist)):
        if t.dtype != torch.float32:
            raise ActorSweepError(f"lrt_actorsweep: {name} must be a float32 tensor (it is {t.dtype}); there is no fall-back to PyTorch on a HIP device")
    xyz_s, rot_s, column, counts = _ActorSweep.apply(xyz, rot_raw, actor_twist, seg_start.contiguous(), poses, w2s, xi, tau64, W, off, yaw, workspace)
    return xyz_s, rot_s, SimpleNamespace(column=column, counts=counts)


# ---- twists from tracking boxes ---------------------------------------------------------------------------------------------------------------------------------

def box_pose(entry) -> np.ndarray:
    """(4, 4) float64 actor -> world of a TrackingBox frame entry (translation (3,), quaternion (1, 4) or (4,), ...), the quaternion normalised."""
    npy = lambda a: (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(np.float64).reshape(-1)
    t, q = npy(entry[0]), npy(entry[1])
    r, x, y, z = q / math.sqrt(float(q @ q))
    T = np.eye(4)
    T[:3, :3] = [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - r * z), 2.0 * (x * z + r * y)],
                 [2.0 * (x * y + r * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - r * x)],
                 [2.0 * (x * z - r * y), 2.0 * (y * z + r * x), 1.0 - 2.0 * (x * x + y * y)]]
    T[:3, 3] = t
    return T


def actor_twists_from_boxes(boxes, frame_ids, sweep_fraction: float = 1.0):
    """Per actor ``{frame: (6,) float64}``: the actor's motion over one sweep in its own frame from its tracking boxes,
    ``eta[f] = Log(A_f^-1 A_f') * sweep_fraction / (f' - f)`` with ``f'`` the next of ``frame_ids`` in which the actor has a pose; the last such frame
    takes the previous interval's twist, an actor seen once gets zeros.  It mirrors ``sweep.twists_from_poses``.  ``boxes``: a dict or a sequence of
    ``sequence.TrackingBox``-like objects (``.frame[f] = (translation, quaternion, ...)``); the result has the same keys (or is a list)."""
    if not (float(sweep_fraction) > 0.0 and math.isfinite(float(sweep_fraction))):
        raise ActorSweepError(f"actor_twists_from_boxes: sweep_fraction {sweep_fraction!r} (positive)")
    wanted = sorted(int(f) for f in frame_ids)

    def one(box):
        ids = [f for f in wanted if f in box.frame]
        out = {}
        for a, b in zip(ids[:-1], ids[1:]):
            out[a] = sweep.twist_between(box_pose(box.frame[a]), box_pose(box.frame[b])) * (float(sweep_fraction) / float(b - a))
        if ids:
            out[ids[-1]] = out[ids[-2]].copy() if len(ids) > 1 else np.zeros(6)
        return out
    if isinstance(boxes, dict):
        return {k: one(b) for k, b in boxes.items()}
    return [one(b) for b in boxes]


# ---- refinement of the twists ---------------------------------------------------------------------------------------------------------------------------------------

class ActorTwists:
    """``train --refine-actor-twist``: one ``nn.Parameter (6,)`` per (actor, training frame) that has a pose and a twist, initialised from the boxes'
    twists and put in their place (``box.twist[frame]``), where ``renderer.actor_sweep`` reads them; Adam, with separate learning rates for the
    translation and the rotation part as ``poses.SensorPoses`` has for the sensor's twists.  The gradient is ``actor_sweep``'s ``d_actor_twist``:
    identical on every rank, as the operator is."""

    def __init__(self, boxes, frame_ids, lr_trans: float = 1e-3, lr_rot: float = 1e-4):
        self.boxes, self.frame_ids = list(boxes), [int(f) for f in frame_ids]
        self.eta = {}
        for a, bb in enumerate(self.boxes):
            for f in self.frame_ids:
                tw = getattr(bb, "twist", {}).get(f)
                if tw is not None and f in bb.frame:
                    self.eta[(a, f)] = bb.twist[f] = torch.nn.Parameter(tw.detach().to(torch.float32).clone())
        if not self.eta:
            raise ValueError("ActorTwists: no actor has a twist in a training frame (load the sequence with actor_sweep='stored' or 'boxes')")
        self.optimizer = torch.optim.Adam([{"params": list(self.eta.values()), "lr": 1.0, "name": "eta"}], betas=(0.9, 0.999), eps=1e-15)
        self.lr_trans, self.lr_rot = float(lr_trans), float(lr_rot)

    def zero_grad(self):
        self.optimizer.zero_grad(set_to_none=True)

    @torch.no_grad()
    def step(self):
        """One Adam step at unit rate, scaled per component: exactly two learning rates, since Adam's update is elementwise."""
        before = {k: p.detach().clone() for k, p in self.eta.items()}
        self.optimizer.step()
        p0 = next(iter(self.eta.values()))
        scale = torch.tensor([self.lr_trans] * 3 + [self.lr_rot] * 3, device=p0.device)
        for k, p in self.eta.items():
            p.copy_(before[k] + (p - before[k]) * scale)

    def state_dict(self):
        return {"eta": {k: p.detach().cpu() for k, p in self.eta.items()}, "optimizer": self.optimizer.state_dict(), "lr_trans": self.lr_trans, "lr_rot": self.lr_rot}

    def load_state_dict(self, sd):
        if set(sd["eta"]) != set(self.eta):
            raise ValueError("ActorTwists: the saved twists belong to other (actor, frame) pairs")
        with torch.no_grad():
            for k, p in self.eta.items():
                p.copy_(sd["eta"][k].to(p.device))
        self.optimizer.load_state_dict(sd["optimizer"])
