"""Scan registration: projective point-to-plane ICP between two range images of the same sensor model, through ``csrc/liblrt_reg.so`` -- the
step in front of every path that needs sensor poses (``ingest --poses``, ``sweep.twists_from_poses``, ``train --refine-poses``).

    pts, nrm, mask = frame_geometry(depth, mask, inclination, H, W, data_type="KITTI", sensor2ego=None)
    sums, assoc    = linearize(src, tgt, X, rh, rw, max_dist, huber=0.1, inclination=...)
    reg            = align(src, tgt, init=None, schedule=DEFAULT_SCHEDULE, huber=0.1, lam=1e-6, min_pairs=50, tol_t=1e-5, tol_r=1e-6,
                           data_type="KITTI", inclination=..., sensor2ego=None)          # Registration: X (F, 3, 4) float64, log, hessian, status
    poses, report  = odometry(frames, first_pose=None, ...)                             # {id: (4, 4) float64 sensor2world}

A geometry is ``(points (H, W, 3), normals (H, W, 3), mask (H, W))`` in the SENSOR frame, float32, or batched with a leading pair axis ``F``;
``src`` may leave its normals ``None`` (only the target's are read).  ``X`` is the source sensor's pose in the target sensor's frame,
``X = T_tgt^-1 T_src`` -- what ``sweep.twist_between`` takes the log of -- as float64 ``(3, 4)`` / ``(4, 4)`` or ``(F, 3, 4)`` / ``(F, 4, 4)``.
``include/lrt_reg.h`` states the rule (the pixel of ``X p`` by the projection's rule, the nearest valid target pixel of a window around it, the
point-to-plane residual with a Huber weight, a right perturbation ``X <- X Exp(delta)``, 30 float64 sums per pair in a fixed order, a Cholesky
solve); ``csrc/lrt_reg_math.h`` is its text for the device and the host.  The ``(0, 0, 1)`` fall-back normal is not special: a zero normal is
the one way to exclude a target pixel, and ``frame_geometry`` stores one where fewer than three neighbours were listed.

* HIP tensors go through the library: ``linearize`` is two launches, ``align`` is ``2 K`` launches for a schedule of ``K`` iterations and all
  ``F`` pairs, with no host wait and no atomics (two calls return the same bits; a pair's result does not depend on the other pairs of the
  call).  A missing library is an error, not a quiet fall-back.  CPU tensors go to the float64 numpy twins ``linearize_reference`` and
  ``align_reference``, which run anywhere and are the yardstick of the tests.
* ``schedule``: ``K <= 32`` rows ``(rh, rw, max_dist)`` -- the window's half height (``<= 4``) and half width (``<= 16``) in pixels and the
  largest partner distance in metres -- coarse to fine.  ``status`` per pair: 0 ok, 1 fewer than ``min_pairs`` partners, 2 a pivot that is not
  positive, 3 converged (``|rho| < tol_t`` and ``|phi| < tol_r``).  From the first non-zero status on ``X`` keeps its bits.  ``log`` is
  ``(F, K, 8)``: partners, ``sum w e^2``, ``sum w``, ``|rho|``, ``|phi|``, status, 0, 0; ``hessian`` ``(F, 6, 6)`` is ``sum w J J^T`` of the last iteration.
* ``odometry`` runs the consecutive pairs of ``frames`` ({id: geometry}) in id order.  The ``init`` of pair k is the result of pair k - 1 (the
  constant-velocity guess), handed over as a device tensor; the host reads once, at the end.  A pair that ends with status 1 or 2 keeps that
  guess and is named in the report.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import range_image, sweep as sw

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LRT_REG_LIB") or os.path.join(HERE, "csrc", "liblrt_reg.so")
EXPORTS = ("lrt_reg_abi_version", "lrt_reg_last_error", "lrt_reg_work_bytes", "lrt_reg_linearize", "lrt_reg_align")     # include/lrt_reg.h
ABI_VERSION = 1
BLOCK = 256                                                                  # LRT_REG_BLOCK
NSUM = 30                                                                    # LRT_REG_NSUM
NLOG = 8                                                                     # LRT_REG_NLOG
MAX_ITER, MAX_RH, MAX_RW, MAX_PAIRS = 32, 4, 16, 65535
MAX_PIXELS = (2 ** 31 - 1) // 3                                              # LRT_REG_MAX_PIXELS
EPS = 1e-12                                                                  # LRT_REG_EPS
OK, FEW, PIVOT, CONVERGED = 0, 1, 2, 3
FLT_MAX = float(np.finfo(np.float32).max)
# Three wide steps that catch an offset of a metre and a few degrees, one that tightens, ten that settle.  The wide levels are short on purpose:
# a pair that converges (status 3) keeps its X from then on, and one that converges against the wide level's partners -- many of them across a
# crease, at up to 2 m -- never sees the fine level.  On the room of tests/registration_cases.py four wide steps of the same windows already end
# there, 1.5 to 2.7 times further from the truth.
DEFAULT_SCHEDULE = ((2, 8, 2.0),) * 3 + ((1, 4, 0.5),) + ((1, 2, 0.25),) * 10

_lib = None


class RegistrationError(RuntimeError):
    pass


class Registration(SimpleNamespace):
    """X (F, 3, 4) float64, log (F, K, 8) float64, hessian (F, 6, 6) float64, status (F) int32; without a pair axis in the inputs, without one here."""

    def __iter__(self):
        return iter((self.X, self.log, self.hessian, self.status))


def load():
    """Load liblrt_reg.so (after torch, so that both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RegistrationError(f"{LIB_PATH} is missing: build it with `python -m lidar_rt_amd.build` (hipcc --offload-arch=gfx950). "
                                "registration has no fall-back on a HIP device.")
    lib = C.CDLL(LIB_PATH)
    vp, ci, ll, d = C.c_void_p, C.c_int, C.c_longlong, C.c_double
    lib.lrt_reg_abi_version.restype = ci
    lib.lrt_reg_last_error.restype = C.c_char_p
    lib.lrt_reg_work_bytes.restype = ll
    lib.lrt_reg_work_bytes.argtypes = [ll, ci, ci]
    common = [ci, ll, ci, ci, vp, ci, d, d, d, d, vp, vp, vp, vp, vp]
    lib.lrt_reg_linearize.restype = ci
    lib.lrt_reg_linearize.argtypes = common + [vp, ci, ci, d, d, vp, vp, vp, ll, vp]
    lib.lrt_reg_align.restype = ci
    lib.lrt_reg_align.argtypes = common + [vp, vp, ci, d, d, ll, d, d, vp, vp, vp, vp, vp, ll, vp]
    if lib.lrt_reg_abi_version() != ABI_VERSION:
        raise RegistrationError("liblrt_reg.so ABI version mismatch; rebuild with `python -m lidar_rt_amd.build --force`")
    _lib = lib
    return lib


# ---- the arguments ------------------------------------------------------------------------------------------------------------------------------------------

def _mask8(m):
    if m.dtype == torch.bool:
        return m.contiguous().view(torch.uint8)
    return m.contiguous() if m.dtype == torch.uint8 else (m != 0).view(torch.uint8)


def _geometry(name, g, want_normals):
    """(points (F, H, W, 3) float32, normals or None, mask (F, H, W) uint8, batched)."""
    if not isinstance(g, (tuple, list)) or len(g) not in (2, 3):
        raise RegistrationError(f"registration: {name} must be (points, normals, mask)" + ("" if want_normals else " or (points, mask)"))
    pts, nrm, mask = (g[0], None, g[1]) if len(g) == 2 else g
    if not torch.is_tensor(pts) or pts.dim() not in (3, 4) or pts.shape[-1] != 3 or pts.dtype != torch.float32:
        raise RegistrationError(f"registration: {name}'s points must be a float32 (H, W, 3) or (F, H, W, 3) tensor")
    batched = pts.dim() == 4
    shape = tuple(pts.shape[:-1])
    if not torch.is_tensor(mask) or tuple(mask.shape) != shape or mask.device != pts.device:
        raise RegistrationError(f"registration: {name}'s mask must be a {shape} tensor on {pts.device}")
    if want_normals:
        if not torch.is_tensor(nrm) or nrm.shape != pts.shape or nrm.dtype != torch.float32 or nrm.device != pts.device:
            raise RegistrationError(f"registration: {name}'s normals must be a float32 {tuple(pts.shape)} tensor on {pts.device}")
        nrm = nrm.detach().contiguous()
        nrm = nrm if batched else nrm[None]
    pts, mask = pts.detach().contiguous(), _mask8(mask.detach())
    return (pts if batched else pts[None]), (nrm if want_normals else None), (mask if batched else mask[None]), batched


def _model(H, W, inclination, data_type, sensor2ego, min_depth, max_depth):
    """(inc float64 numpy, off, yaw, min_depth, max_depth): the projection's checks of the same arguments."""
    if inclination is None:
        raise RegistrationError("registration: inclination is required (two bounds or a per-beam table)")
    try:
        _, _, _, _, inc, _, off, yaw, lo, hi, _ = range_image._arguments((0, 3), H, W, inclination, None, data_type, sensor2ego, None, max_depth, min_depth, True)
    except range_image.ProjectionError as e:
        raise RegistrationError(str(e).replace("project_points", "registration")) from None
    return inc, off, yaw, lo, hi


def _pair_arguments(src, tgt, inclination, data_type, sensor2ego, min_depth, max_depth):
    sp, _, sm, b0 = _geometry("src", src, False)
    tp, tn, tm, b1 = _geometry("tgt", tgt, True)
    if sp.shape != tp.shape or sp.device != tp.device or b0 != b1:
        raise RegistrationError(f"registration: src {tuple(sp.shape)} on {sp.device} and tgt {tuple(tp.shape)} on {tp.device} differ")
    F, H, W = (int(x) for x in sp.shape[:3])
    if F < 1 or F > MAX_PAIRS or H < 1 or W < 1 or F * H * W > MAX_PIXELS:
        raise RegistrationError(f"registration: {F} pairs of {H} x {W} pixels (each at least 1, at most {MAX_PAIRS} pairs, F H W at most {MAX_PIXELS})")
    inc, off, yaw, lo, hi = _model(H, W, inclination, data_type, sensor2ego, min_depth, max_depth)
    return sp, sm, tp, tn, tm, b0, F, H, W, inc, off, yaw, lo, hi


def _poses(name, X, F, batched, dev):
    """(F, 3, 4) float64 contiguous on dev; None is the identity."""
    if X is None:
        return torch.eye(4, dtype=torch.float64, device=dev)[:3].expand(F, 3, 4).contiguous()
    if isinstance(X, np.ndarray):
        X = torch.from_numpy(np.ascontiguousarray(X, np.float64))
    want = ((F, 3, 4), (F, 4, 4)) if batched else ((3, 4), (4, 4))
    if not torch.is_tensor(X) or tuple(X.shape) not in want or X.dtype != torch.float64 or X.device != dev:
        raise RegistrationError(f"registration: {name} must be a float64 tensor of shape {want[0]} or {want[1]} on {dev}"
                                + (f" (it is {tuple(X.shape)}, {X.dtype}, {X.device})" if torch.is_tensor(X) else ""))
    X = X.detach() if batched else X.detach()[None]
    return X[:, :3, :].contiguous()


def _window(rh, rw, max_dist):
    if not (float(rh).is_integer() and float(rw).is_integer() and 0 <= rh <= MAX_RH and 0 <= rw <= MAX_RW):
        raise RegistrationError(f"registration: a window of {rh} rows and {rw} columns either side (whole numbers, at most {MAX_RH} and {MAX_RW})")
    if not (float(max_dist) > 0.0 and math.isfinite(float(max_dist))):
        raise RegistrationError(f"registration: max_dist {max_dist} (positive)")
    return int(rh), int(rw), float(max_dist)


def _schedule(schedule):
    try:
        s = np.ascontiguousarray(np.asarray(schedule, np.float64))
    except (TypeError, ValueError) as e:
        raise RegistrationError(f"registration: the schedule is not numeric: {e}") from None
    if s.ndim != 2 or s.shape[1] != 3 or not 1 <= s.shape[0] <= MAX_ITER:
        raise RegistrationError(f"registration: the schedule must be (K, 3) rows of rh, rw, max_dist with 1 <= K <= {MAX_ITER} (it is {s.shape})")
    for row in s:
        _window(*row)
    return s


def _solver(huber, lam, min_pairs, tol_t, tol_r):
    huber, lam, tol_t, tol_r = float(huber), float(lam), float(tol_t), float(tol_r)
    if not (huber > 0.0 and math.isfinite(huber)):
        raise RegistrationError(f"registration: huber {huber} (positive)")
    if not (lam >= 0.0 and math.isfinite(lam)):
        raise RegistrationError(f"registration: lam {lam} (not negative)")
    if int(min_pairs) < 1:
        raise RegistrationError(f"registration: min_pairs {min_pairs} (at least 1)")
    if not (tol_t >= 0.0 and tol_r >= 0.0):
        raise RegistrationError(f"registration: tolerances {tol_t}, {tol_r} (not negative)")
    return huber, lam, int(min_pairs), tol_t, tol_r


# ---- the twin -----------------------------------------------------------------------------------------------------------------------------------------------

def _classify(q, H, W, inc, off, yaw, min_depth, max_depth):
    """pj_classify on (N, 3) float64 points with wrap = 1: (keep, h0, w0)."""
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    with np.errstate(all="ignore"):
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        r = np.sqrt(x * x + y * y + z * z)
        rd = r.astype(np.float32).astype(np.float64)
        keep = finite & (r != 0.0) & (rd > min_depth) & (rd <= max_depth)
        az = np.arctan2(y, x)
        el = np.arctan2(z, np.hypot(x, y))
        u = (np.pi - (az + yaw)) * float(W) / range_image.TWO_PI - off
        w = np.rint(u)
        w = w - np.floor(w / float(W)) * float(W)
        keep &= (w >= 0.0) & (w < float(W))
        if inc.size == 2:
            t = (el - inc[0]) / (inc[1] - inc[0]) * float(H)
            h = np.rint(float(H) - off - t)
            keep &= (h >= 0.0) & (h < float(H))
        else:
            h, _ = range_image._table_rows(np.where(np.isfinite(el), el, 0.0), inc, H)
            keep &= h >= 0
    return keep, np.where(keep, h, 0).astype(np.int64), np.where(keep, w, 0).astype(np.int64)


def _d2(t, q):
    """rg_d2 on float32 (N, 3) arrays: float32 differences, fma(dz, dz, fma(dy, dy, dx * dx)) with the products exact in float64."""
    d = t - q
    xx = d[:, 0] * d[:, 0]
    yy = (d[:, 1].astype(np.float64) * d[:, 1].astype(np.float64) + xx.astype(np.float64)).astype(np.float32)
    return (d[:, 2].astype(np.float64) * d[:, 2].astype(np.float64) + yy.astype(np.float64)).astype(np.float32)


def residuals_reference(p, X, qt, n):
    """(e (N,), J (N, 6)) of points p (N, 3) at X (3, 4) against partners qt with normals n, float64: steps 4 and 5 of the rule."""
    q = np.stack([X[k, 0] * p[:, 0] + X[k, 1] * p[:, 1] + X[k, 2] * p[:, 2] + X[k, 3] for k in range(3)], 1)
    e = n[:, 0] * (q[:, 0] - qt[:, 0]) + n[:, 1] * (q[:, 1] - qt[:, 1]) + n[:, 2] * (q[:, 2] - qt[:, 2])
    m = [X[0, j] * n[:, 0] + X[1, j] * n[:, 1] + X[2, j] * n[:, 2] for j in range(3)]
    J = np.stack(m + [p[:, 1] * m[2] - p[:, 2] * m[1], p[:, 2] * m[0] - p[:, 0] * m[2], p[:, 0] * m[1] - p[:, 1] * m[0]], 1)
    return e, J


def _linearize_pair(sp, sm, tp, tn, tm, X, H, W, inc, off, yaw, min_depth, max_depth, rh, rw, max_dist, huber):
    """One pair, numpy: (sums (30,), assoc (H W,) int32, abs_sums (30,): the sums of the terms' magnitudes)."""
    HW = H * W
    sp, tp, tn = sp.reshape(HW, 3), tp.reshape(HW, 3), tn.reshape(HW, 3)
    tm = tm.reshape(HW) != 0
    idx = np.nonzero(sm.reshape(HW))[0]
    assoc = np.full(HW, -1, np.int32)
    p = sp[idx].astype(np.float64)
    q = np.stack([X[k, 0] * p[:, 0] + X[k, 1] * p[:, 1] + X[k, 2] * p[:, 2] + X[k, 3] for k in range(3)], 1) if idx.size else np.zeros((0, 3))
    keep, h0, w0 = _classify(q, H, W, inc, off, yaw, min_depth, max_depth)
    with np.errstate(all="ignore"):
        q32 = q.astype(np.float32)
        best = np.full(idx.size, -1, np.int64)
        best_d2 = np.zeros(idx.size, np.float32)
        for dh in range(-rh, rh + 1):
            h = h0 + dh
            row_ok = keep & (h >= 0) & (h < H)
            for dw in range(-rw, rw + 1):
                j = np.clip(h, 0, H - 1) * W + (w0 + dw) % W
                d2 = _d2(tp[j], q32)
                cand = row_ok & tm[j] & ~np.isnan(d2)
                better = cand & ((best < 0) | (d2 < best_d2) | ((d2 == best_d2) & (j < best)))
                best = np.where(better, j, best)
                best_d2 = np.where(better, d2, best_d2)
        has = (best >= 0) & (best_d2.astype(np.float64) <= max_dist * max_dist)
        has &= (tn[np.maximum(best, 0)] != 0).any(1)
    sel = np.nonzero(has)[0]
    assoc[idx[sel]] = best[sel].astype(np.int32)
    e, J = residuals_reference(p[sel], X, tp[best[sel]].astype(np.float64), tn[best[sel]].astype(np.float64))
    ae = np.abs(e)
    with np.errstate(all="ignore"):
        wt = np.where(ae <= huber, 1.0, huber / ae)
    terms = np.empty((sel.size, NSUM))
    k = 0
    for i in range(6):
        wj = wt * J[:, i]
        for j in range(i, 6):
            terms[:, k] = wj * J[:, j]
            k += 1
    for i in range(6):
        terms[:, 21 + i] = (wt * J[:, i]) * e
    terms[:, 27] = (wt * e) * e
    terms[:, 28] = wt
    terms[:, 29] = 1.0
    return terms.sum(0), assoc, np.abs(terms).sum(0)


def exp_reference(delta):
    """sw_exp in numpy: (Re (3, 3), te (3,)) of delta = (rho, phi), the series below SERIES_TH2."""
    delta = np.asarray(delta, np.float64)
    rho, phi = delta[:3], delta[3:]
    A, B, Cc = sw._coef_np(float(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]))
    K = sw._hat_np(phi)
    K2 = K @ K
    return np.eye(3) + A * K + B * K2, (np.eye(3) + B * K + Cc * K2) @ rho


def _hessian(s):
    A = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = s[k]
            k += 1
    return A


def solve_reference(s, lam, min_pairs, tol_t, tol_r, X):
    """rg_solve in numpy: (status, X or its successor, |rho|, |phi|)."""
    if not s[29] >= min_pairs:
        return FEW, X, 0.0, 0.0
    M = _hessian(s)
    for i in range(6):
        M[i, i] = M[i, i] + lam * M[i, i] + EPS
    L = np.zeros((6, 6))
    for j in range(6):
        v = M[j, j]
        for c in range(j):
            v = v - L[j, c] * L[j, c]
        if not v > 0.0:
            return PIVOT, X, 0.0, 0.0
        L[j, j] = math.sqrt(v)
        for i in range(j + 1, 6):
            u = M[i, j]
            for c in range(j):
                u = u - L[i, c] * L[j, c]
            L[i, j] = u / L[j, j]
    y, d = np.zeros(6), np.zeros(6)
    for i in range(6):
        v = -s[21 + i]
        for c in range(i):
            v = v - L[i, c] * y[c]
        y[i] = v / L[i, i]
    for i in range(5, -1, -1):
        v = y[i]
        for c in range(i + 1, 6):
            v = v - L[c, i] * d[c]
        d[i] = v / L[i, i]
    nr, nf = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), math.sqrt(d[3] * d[3] + d[4] * d[4] + d[5] * d[5])
    if not (math.isfinite(nr) and math.isfinite(nf)):
        return PIVOT, X, 0.0, 0.0
    if nr < tol_t and nf < tol_r:
        return CONVERGED, X, nr, nf
    Re, te = exp_reference(d)
    return OK, np.concatenate([X[:, :3] @ Re, (X[:, :3] @ te + X[:, 3])[:, None]], 1), nr, nf


def _np(t):
    return t.detach().cpu().numpy()


def _sq(batched, *ts):
    return ts if batched else tuple(t[0] for t in ts)


@torch.no_grad()
def linearize_reference(src, tgt, X, rh, rw, max_dist, huber=0.1, inclination=None, data_type="KITTI", sensor2ego=None, min_depth=0.0, max_depth=FLT_MAX,
                        return_abs=False):
    """The float64 numpy twin of ``linearize``: (sums (F, 30) float64, assoc (F, H, W) int32) as CPU tensors; ``return_abs=True`` adds the sums of the
    terms' magnitudes (F, 30), the scale of the summation bound."""
    sp, sm, tp, tn, tm, batched, F, H, W, inc, off, yaw, lo, hi = _pair_arguments(src, tgt, inclination, data_type, sensor2ego, min_depth, max_depth)
    rh, rw, max_dist = _window(rh, rw, max_dist)
    huber = _solver(huber, 0.0, 1, 0.0, 0.0)[0]
    Xn = _np(_poses("X", X, F, batched, X.device if torch.is_tensor(X) else torch.device("cpu")))
    sp, sm, tp, tn, tm = (_np(t) for t in (sp, sm, tp, tn, tm))
    out = [_linearize_pair(sp[f], sm[f], tp[f], tn[f], tm[f], Xn[f], H, W, inc, off, yaw, lo, hi, rh, rw, max_dist, huber) for f in range(F)]
    sums, assoc, ab = (torch.from_numpy(np.stack([o[k] for o in out])) for k in range(3))
    res = _sq(batched, sums, assoc.reshape(F, H, W), ab)
    return res if return_abs else res[:2]


@torch.no_grad()
def align_reference(src, tgt, init=None, schedule=DEFAULT_SCHEDULE, huber=0.1, lam=1e-6, min_pairs=50, tol_t=1e-5, tol_r=1e-6, data_type="KITTI",
                    inclination=None, sensor2ego=None, min_depth=0.0, max_depth=FLT_MAX) -> Registration:
    """The float64 numpy twin of ``align`` (see the module text); the results are CPU tensors."""
    sp, sm, tp, tn, tm, batched, F, H, W, inc, off, yaw, lo, hi = _pair_arguments(src, tgt, inclination, data_type, sensor2ego, min_depth, max_depth)
    sched = _schedule(schedule)
    huber, lam, min_pairs, tol_t, tol_r = _solver(huber, lam, min_pairs, tol_t, tol_r)
    K = sched.shape[0]
    X = _np(_poses("init", init, F, batched, init.device if torch.is_tensor(init) else torch.device("cpu"))).copy()
    sp, sm, tp, tn, tm = (_np(t) for t in (sp, sm, tp, tn, tm))
    log, hess, status = np.zeros((F, K, NLOG)), np.zeros((F, 6, 6)), np.zeros(F, np.int32)
    for f in range(F):
        st = OK
        for it in range(K):
            s, _, _ = _linearize_pair(sp[f], sm[f], tp[f], tn[f], tm[f], X[f], H, W, inc, off, yaw, lo, hi, int(sched[it, 0]), int(sched[it, 1]),
                                      float(sched[it, 2]), huber)
            nr = nf = 0.0
            if st == OK:
                st, X[f], nr, nf = solve_reference(s, lam, float(min_pairs), tol_t, tol_r, X[f])
            log[f, it] = (s[29], s[27], s[28], nr, nf, float(st), 0.0, 0.0)
        hess[f], status[f] = _hessian(s), st
    X, log, hess, status = _sq(batched, *(torch.from_numpy(a) for a in (X, log, hess, status)))
    return Registration(X=X, log=log, hessian=hess, status=status)


# ---- the operators ------------------------------------------------------------------------------------------------------------------------------------------

def work_bytes(F: int, H: int, W: int) -> int:
    """Bytes of the workspace of one call: the workgroups' partial rows and the running status."""
    n = int(load().lrt_reg_work_bytes(int(F), int(H), int(W)))
    if n < 0:
        raise RegistrationError(f"registration: {F} pairs of {H} x {W} pixels (each at least 1, at most {MAX_PAIRS} pairs, F H W at most {MAX_PIXELS})")
    return n


def _workspace(workspace, nbytes, dev):
    if workspace is None:
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)              # the caching allocator's blocks are 512-byte aligned
    if not (torch.is_tensor(workspace) and workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.device == dev
            and workspace.numel() >= nbytes and workspace.data_ptr() % 256 == 0):
        raise RegistrationError(f"lrt_reg: the workspace must be a contiguous uint8 tensor of at least {nbytes} bytes on {dev}, 256-byte aligned")
    return workspace


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


@torch.no_grad()
def linearize(src, tgt, X, rh, rw, max_dist, huber=0.1, inclination=None, data_type="KITTI", sensor2ego=None, min_depth=0.0, max_depth=FLT_MAX,
              want_assoc=True, workspace=None):
    """(sums (F, 30) float64, assoc (F, H, W) int32 or None) of F pairs at X (see the module text)."""
    sp, sm, tp, tn, tm, batched, F, H, W, inc, off, yaw, lo, hi = _pair_arguments(src, tgt, inclination, data_type, sensor2ego, min_depth, max_depth)
    dev = sp.device
    if dev.type != "cuda":
        if workspace is not None:
            raise RegistrationError(f"linearize: a workspace with tensors on {dev}")
        sums, assoc = linearize_reference(src, tgt, X, rh, rw, max_dist, huber, inclination, data_type, sensor2ego, min_depth, max_depth)
        return sums, (assoc if want_assoc else None)
    lib = load()
    rh, rw, max_dist = _window(rh, rw, max_dist)
    huber = _solver(huber, 0.0, 1, 0.0, 0.0)[0]
    Xd = _poses("X", X, F, batched, dev)
    ws = _workspace(workspace, work_bytes(F, H, W), dev)
    d_inc = range_image._upload(inc, dev)
    sums = torch.empty((F, NSUM), dtype=torch.float64, device=dev)
    assoc = torch.empty((F, H, W), dtype=torch.int32, device=dev) if want_assoc else None
    with torch.cuda.device(dev):
        rc = lib.lrt_reg_linearize(dev.index, F, H, W, d_inc.data_ptr(), int(inc.size), off, yaw, lo, hi, sp.data_ptr(), sm.data_ptr(), tp.data_ptr(),
                                   tn.data_ptr(), tm.data_ptr(), Xd.data_ptr(), rh, rw, max_dist, huber, sums.data_ptr(),
                                   None if assoc is None else assoc.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev))
    if rc != 0:
        raise RegistrationError(f"lrt_reg_linearize failed ({rc}): {lib.lrt_reg_last_error().decode()}")
    if not batched:
        sums, assoc = sums[0], (None if assoc is None else assoc[0])
    return sums, assoc


@torch.no_grad()
def align(src, tgt, init=None, schedule=DEFAULT_SCHEDULE, huber=0.1, lam=1e-6, min_pairs=50, tol_t=1e-5, tol_r=1e-6, data_type="KITTI", inclination=None,
          sensor2ego=None, min_depth=0.0, max_depth=FLT_MAX, workspace=None) -> Registration:
    """Align F source frames to their target frames (see the module text).  ``init``: X to start from, float64 on the geometry's device (the ``X`` of
    an earlier call is used as it is, without a host read); ``None`` is the identity."""
    sp, sm, tp, tn, tm, batched, F, H, W, inc, off, yaw, lo, hi = _pair_arguments(src, tgt, inclination, data_type, sensor2ego, min_depth, max_depth)
    dev = sp.device
    if dev.type != "cuda":
        if workspace is not None:
            raise RegistrationError(f"align: a workspace with tensors on {dev}")
        return align_reference(src, tgt, init, schedule, huber, lam, min_pairs, tol_t, tol_r, data_type, inclination, sensor2ego, min_depth, max_depth)
    lib = load()
    sched = _schedule(schedule)
    huber, lam, min_pairs, tol_t, tol_r = _solver(huber, lam, min_pairs, tol_t, tol_r)
    K = int(sched.shape[0])
    X0 = _poses("init", init, F, batched, dev)
    ws = _workspace(workspace, work_bytes(F, H, W), dev)
    d_inc = range_image._upload(inc, dev)
    X = torch.empty((F, 3, 4), dtype=torch.float64, device=dev)
    log = torch.empty((F, K, NLOG), dtype=torch.float64, device=dev)
    hess = torch.empty((F, 6, 6), dtype=torch.float64, device=dev)
    status = torch.empty((F,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.lrt_reg_align(dev.index, F, H, W, d_inc.data_ptr(), int(inc.size), off, yaw, lo, hi, sp.data_ptr(), sm.data_ptr(), tp.data_ptr(),
                               tn.data_ptr(), tm.data_ptr(), X0.data_ptr(), sched.ctypes.data, K, huber, lam, min_pairs, tol_t, tol_r, X.data_ptr(),
                               log.data_ptr(), hess.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev))
    if rc != 0:
        raise RegistrationError(f"lrt_reg_align failed ({rc}): {lib.lrt_reg_last_error().decode()}")
    X, log, hess, status = _sq(batched, X, log, hess, status)
    return Registration(X=X, log=log, hessian=hess, status=status)


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------------------------

@torch.no_grad()
def frame_geometry(depth, mask, inclination, H=None, W=None, data_type="KITTI", sensor2ego=None, k: int = 6):
    """(points (H, W, 3) float32, normals (H, W, 3) float32, mask (H, W) bool) of one range image in its SENSOR frame (origins zero): the local
    directions of the ray grid times the range, and ``scene_init.estimate_normals`` on them.  A pixel with fewer than three listed neighbours gets
    the zero normal (it is no partner), not the estimator's (0, 0, 1) fall-back.  HIP tensors stay on the device; there is no host wait."""
    from . import scene_init
    if not torch.is_tensor(depth) or depth.dim() != 2:
        raise RegistrationError("frame_geometry: depth must be an (H, W) tensor")
    if (H is not None and int(H) != depth.shape[0]) or (W is not None and int(W) != depth.shape[1]):
        raise RegistrationError(f"frame_geometry: depth is {tuple(depth.shape)}, not ({H}, {W})")
    H, W = int(depth.shape[0]), int(depth.shape[1])
    dev = depth.device
    depth = depth.detach().to(torch.float32).contiguous()
    mask = (mask.detach() != 0).to(dev)
    P = torch.eye(4, dtype=torch.float32, device=dev)[:3].contiguous()
    o, d = sw.sweep_rays(P, None, H, W, inclination, data_type, sensor2ego)
    o, d = o.contiguous(), d.contiguous()
    normals, nbr = scene_init.estimate_normals(o, d, depth, mask, k)
    normals = torch.where(((nbr >= 0).sum(-1) >= 3)[..., None] & mask[..., None], normals, torch.zeros_like(normals))
    points = torch.where(mask[..., None], d * depth[..., None], torch.zeros_like(d))
    return points.contiguous(), normals.contiguous(), mask


@torch.no_grad()
def odometry(frames, first_pose=None, schedule=DEFAULT_SCHEDULE, huber=0.1, lam=1e-6, min_pairs=50, tol_t=1e-5, tol_r=1e-6, data_type="KITTI",
             inclination=None, sensor2ego=None, min_depth=0.0, max_depth=FLT_MAX, return_steps=False):
    """({id: (4, 4) float64 sensor2world}, report) from ``frames`` = {id: (points, normals, mask)} (``frame_geometry``), see the module text.
    ``first_pose``: the (4, 4) pose of the lowest id (the identity otherwise).  The report: the schedule and, per pair, ``source``, ``target``,
    ``status`` and the final number of ``partners``; ``failed`` names the source ids whose pair kept the constant-velocity guess.  ``return_steps=True`` adds
    ``report["steps"]``: per pair ``source``, ``target``, ``X`` (3, 4), ``hessian`` (6, 6) and ``status`` as numpy float64, from the same one host read
    -- the odometry edges of ``pose_graph``."""
    ids = sorted(int(i) for i in frames)
    if len(ids) < 1:
        raise RegistrationError("odometry: no frames")
    T0 = np.eye(4) if first_pose is None else np.asarray(first_pose.detach().cpu() if torch.is_tensor(first_pose) else first_pose, np.float64).reshape(-1)
    if T0.size == 12:
        T0 = np.concatenate([T0, [0.0, 0.0, 0.0, 1.0]])
    if T0.size != 16:
        raise RegistrationError("odometry: first_pose must be a (4, 4) or (3, 4) matrix")
    T0 = T0.reshape(4, 4)
    sched = _schedule(schedule)
    steps, prev = [], None
    for a, b in zip(ids[:-1], ids[1:]):                                      # b onto a: X = T_a^-1 T_b
        tgt, src = frames[a], frames[b]                                    # in this order: a mapping that makes its values on access keeps two
        reg = align(src, tgt, prev, sched, huber, lam, min_pairs, tol_t, tol_r, data_type, inclination, sensor2ego, min_depth, max_depth)
        steps.append(reg)
        prev = reg.X
    poses, pairs = {ids[0]: T0.copy()}, []
    if steps:                                                               # the one host read
        X = torch.stack([r.X for r in steps]).cpu().numpy()
        status = torch.stack([r.status for r in steps]).cpu().numpy()
        partners = torch.stack([r.log[-1, 0] for r in steps]).cpu().numpy()
        hessian = torch.stack([r.hessian for r in steps]).cpu().numpy() if return_steps else None
        for k, (a, b) in enumerate(zip(ids[:-1], ids[1:])):
            step = np.eye(4)
            step[:3] = X[k]
            poses[b] = poses[a] @ step
            pairs.append({"source": b, "target": a, "status": int(status[k]), "partners": int(partners[k])})
    report = {"schedule": sched.tolist(), "huber": float(huber), "pairs": pairs, "failed": [p["source"] for p in pairs if p["status"] in (FEW, PIVOT)]}
    if return_steps:
        report["steps"] = [{"source": p["source"], "target": p["target"], "X": X[k].copy(), "hessian": hessian[k].copy(), "status": p["status"]}
                           for k, p in enumerate(pairs)]
    return poses, report
