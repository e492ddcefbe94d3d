"""Loop closure and the pose graph over the odometry of ``registration.odometry``: a chain of pairwise registrations drifts, and nothing in it ever
compares frame 400 with frame 3 when the vehicle returns to the same street.

    poses, rep     = registration.odometry(frames, ..., return_steps=True)        # rep["steps"]: per pair X, hessian, status
    loops, lrep    = close_loops(frames, poses, rep["steps"], sensor_height=1.8, inclination=...)
    edges          = odometry_edges(rep["steps"]) + loops
    poses, grep    = optimize(poses, edges)

* An EDGE is ``{"a": j, "b": i, "Z": (3, 4), "info": (6, 6)}``: ``Z`` measures ``T_a^-1 T_b`` -- the ``X`` of ``registration.align``, source ``b``
  onto target ``a`` -- and ``info`` is its information matrix, ``align``'s ``hessian`` (``sum w J J^T`` for ``X <- X Exp(delta)``).  The odometry
  edges are the ``steps``.  A pair that ended with status 1 or 2 kept its constant-velocity guess and enters with ``info = weak_info I``;
  ``weak_info`` defaults to 1e-3 times the smallest diagonal entry among the converged pairs' hessians -- a stated choice: it only has to keep the
  system positive definite while letting other edges move that node.
* ``close_loops`` describes and matches all frames in one call each (``place.describe``, ``place.match``), takes ``place.candidates`` and drops a
  candidate ``(i, j)`` whose sensors the chain puts further apart than ``max_drift`` times the path length between them plus the matcher's reach
  (one ring of the descriptor) -- a sanity condition on the chain, not a tuned number.  The others are aligned, source ``i`` onto target ``j``,
  from ``place.shift_to_init`` with a wide-to-fine schedule, ``batch`` pairs per ``align`` call.  A pair is accepted iff its status is converged or
  it ended with at least ``min_overlap`` of the source's valid pixels as partners, AND the weighted rms residual of its last log row,
  ``sqrt(sum w e^2 / sum w)``, is at most ``max_rms``.
* ``optimize``: residual ``r = Log(Z^-1 T_a^-1 T_b)`` (``sweep.se3_log``, twists in ``(rho, phi)`` order), cost ``sum r^T info r``, right
  perturbations ``T <- T Exp(delta)`` (the convention of ``poses.se3_exp`` and of ``align``'s hessian), so ``J_b = Jr^-1(r)`` and
  ``J_a = -Jr^-1(r) Ad(T_b^-1 T_a)``.  The lowest id is fixed.  Levenberg-Marquardt in float64 numpy with a dense normal matrix and a Cholesky
  solve: ``6 (F - 1) <= 4096`` is supported, a larger graph raises a ``PoseGraphError`` that names the limit (a block-sparse factorisation is the
  next step).  There is no outlier rejection inside the solve beyond the gates of ``close_loops``.

Everything here is host float64, like everything after the integer tables in ``actors.discover``; the device work is ``place`` and ``align``.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import place, registration as rg, sweep as sw

MAX_UNKNOWNS = 4096
DEFAULT_MAX_DRIFT = 0.1
DEFAULT_WEAK_SCALE = 1e-3
# Wide steps that catch what a sector of yaw and a ring of offset leave, then the tightening and settling levels of registration.DEFAULT_SCHEDULE.
LOOP_SCHEDULE = ((4, 16, 3.0),) * 4 + ((2, 8, 1.0),) * 4 + ((1, 4, 0.5),) * 2 + ((1, 2, 0.25),) * 10
# Halfway between the worst alignment that settled and the best one that did not, as the twin saw them on the room tour of tests/place_cases.py
# (the table is in profiles/place.md; scenes of tools/make_sequence.py and real scans were not measured).
DEFAULT_MIN_OVERLAP = 0.63
DEFAULT_MAX_RMS = 0.028
DEFAULT_TOL = 1e-10
DEFAULT_MAX_ITER = 50


class PoseGraphError(RuntimeError):
    pass


# ---- SE(3) on the host, twists as (rho, phi) -----------------------------------------------------------------------------------------------------------------

def _pose34(name, T):
    if torch.is_tensor(T):
        T = T.detach().cpu().numpy()
    T = np.asarray(T, np.float64)
    if T.shape not in ((3, 4), (4, 4)):
        raise PoseGraphError(f"{name}: a (3, 4) or (4, 4) pose (it is {T.shape})")
    return T[:3].copy()


def relative(Ta, Tb):
    """(3, 4) ``T_a^-1 T_b``."""
    Ri = Ta[:, :3].T
    return np.concatenate([Ri @ Tb[:, :3], (Ri @ (Tb[:, 3] - Ta[:, 3]))[:, None]], 1)


def _compose(T, Re, te):
    return np.concatenate([T[:, :3] @ Re, (T[:, :3] @ te + T[:, 3])[:, None]], 1)


def adjoint(T):
    """(6, 6) Ad(T) for twists (rho, phi): [[R, t^ R], [0, R]]."""
    R, t = T[:, :3], T[:, 3]
    A = np.zeros((6, 6))
    A[:3, :3] = R
    A[:3, 3:] = sw._hat_np(t) @ R
    A[3:, 3:] = R
    return A


def _left_jacobian_inverse(xi):
    """Jl^-1 of SE(3) at xi = (rho, phi): [[J^-1, -J^-1 Q J^-1], [0, J^-1]] (Barfoot, State Estimation for Robotics, 7.95), the series in ad below
    a rotation of 1e-2 rad."""
    rho, phi = xi[:3], xi[3:]
    th2 = float(phi @ phi)
    P, Rh = sw._hat_np(phi), sw._hat_np(rho)
    if th2 < 1e-4:
        ad = np.zeros((6, 6))
        ad[:3, :3], ad[:3, 3:], ad[3:, 3:] = P, Rh, P
        ad2 = ad @ ad
        return np.eye(6) - 0.5 * ad + ad2 / 12.0 - (ad2 @ ad2) / 720.0           # B_n / n!: 1, -1/2, 1/12, 0, -1/720 (the next term is th^6 / 30240)
    th = math.sqrt(th2)
    s, c = math.sin(th), math.cos(th)
    P2 = P @ P
    Ji = np.eye(3) - 0.5 * P + (1.0 / th2 - (1.0 + c) / (2.0 * th * s)) * P2
    PR, RP = P @ Rh, Rh @ P
    PRP = PR @ P
    Q = (0.5 * Rh + (th - s) / (th2 * th) * (PR + RP + PRP)
         + (th2 + 2.0 * c - 2.0) / (2.0 * th2 * th2) * (P @ PR + RP @ P - 3.0 * PRP)
         + (2.0 * th - 3.0 * s + th * c) / (2.0 * th2 * th2 * th) * (PRP @ P + P @ PRP))
    out = np.zeros((6, 6))
    out[:3, :3] = Ji
    out[3:, 3:] = Ji
    out[:3, 3:] = -Ji @ Q @ Ji
    return out


def right_jacobian_inverse(xi):
    """(6, 6) Jr^-1(xi): Log(Exp(xi) Exp(d)) = xi + Jr^-1(xi) d + O(d^2)."""
    return _left_jacobian_inverse(-np.asarray(xi, np.float64))


def residual(Z, Ta, Tb):
    """(6,) r = Log(Z^-1 T_a^-1 T_b).  A measurement that IS the relative pose, bit for bit, has the residual zero, bit for bit."""
    M = relative(Ta, Tb)
    if np.array_equal(M, Z):
        return np.zeros(6)
    return sw.se3_log(relative(Z, M))


def jacobians(Z, Ta, Tb):
    """(r, J_a, J_b) of an edge for right perturbations of both poses."""
    r = residual(Z, Ta, Tb)
    Jb = right_jacobian_inverse(r)
    return r, -Jb @ adjoint(relative(Tb, Ta)), Jb


# ---- the edges -------------------------------------------------------------------------------------------------------------------------------------------------

def _edge(e):
    info = np.asarray(e["info"], np.float64)
    if info.shape != (6, 6):
        raise PoseGraphError(f"an edge's info must be (6, 6) (it is {info.shape})")
    return int(e["a"]), int(e["b"]), _pose34("an edge's Z", e["Z"]), 0.5 * (info + info.T)


def odometry_edges(steps, weak_info=None):
    """The odometry edges of ``registration.odometry(..., return_steps=True)``'s ``steps``; a pair of status 1 or 2 enters with its
    constant-velocity guess and ``weak_info I`` (see the module text)."""
    steps = list(steps)
    good = [np.diag(np.asarray(s["hessian"], np.float64)).min() for s in steps if int(s["status"]) not in (rg.FEW, rg.PIVOT)]
    if weak_info is None:
        weak_info = DEFAULT_WEAK_SCALE * min(good) if good and min(good) > 0.0 else 1.0
    weak_info = float(weak_info)
    if not (weak_info > 0.0 and math.isfinite(weak_info)):
        raise PoseGraphError(f"odometry_edges: weak_info {weak_info} (positive)")
    out = []
    for s in steps:
        failed = int(s["status"]) in (rg.FEW, rg.PIVOT)
        out.append({"a": int(s["target"]), "b": int(s["source"]), "Z": _pose34("a step's X", s["X"]),
                    "info": weak_info * np.eye(6) if failed else np.asarray(s["hessian"], np.float64).copy(), "kind": "weak" if failed else "odometry"})
    return out


def path_lengths(poses):
    """({id: index}, cumulative path length per index) along the ids in ascending order."""
    ids = sorted(int(i) for i in poses)
    t = np.stack([_pose34("a pose", poses[i])[:, 3] for i in ids])
    return {i: k for k, i in enumerate(ids)}, np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(t, axis=0), axis=1))])


@torch.no_grad()
def close_loops(frames, poses, steps=None, sensor_height=None, z_lo=None, gap=place.DEFAULT_GAP, top=place.DEFAULT_TOP, max_score=place.DEFAULT_MAX_SCORE,
                rings=place.DEFAULT_RINGS, sectors=place.DEFAULT_SECTORS, r_min=place.DEFAULT_R_MIN, r_max=place.DEFAULT_R_MAX, z_step=place.DEFAULT_Z_STEP,
                up=(0.0, 0.0, 1.0), max_drift=DEFAULT_MAX_DRIFT, schedule=LOOP_SCHEDULE, min_overlap=DEFAULT_MIN_OVERLAP, max_rms=DEFAULT_MAX_RMS, batch=16,
                huber=0.1, lam=1e-6, min_pairs=50, tol_t=1e-5, tol_r=1e-6, data_type="KITTI", inclination=None, sensor2ego=None, min_depth=0.0,
                max_depth=rg.FLT_MAX):
    """(loop edges, report) for ``frames`` = {id: (points, normals, mask)} and the chain's ``poses`` = {id: (4, 4)} (see the module text).  ``steps``
    is accepted for symmetry with ``odometry_edges`` and not read: the gate needs the chain's poses only.  ``z_lo`` defaults to ``-sensor_height``;
    one of the two is required.  The report: ``candidates`` (every pair the matcher proposed), ``accepted`` and ``rejected`` with the reason."""
    ids = sorted(int(i) for i in frames)
    if sorted(int(i) for i in poses) != ids:
        raise PoseGraphError("close_loops: frames and poses must carry the same ids")
    if z_lo is None:
        if sensor_height is None:
            raise PoseGraphError("close_loops: sensor_height is required (the height of the sensor above the ground, metres): nothing is guessed from the data")
        z_lo = -float(sensor_height)
    if not (float(max_drift) >= 0.0 and 0.0 <= float(min_overlap) <= 1.0 and float(max_rms) >= 0.0 and int(batch) >= 1):
        raise PoseGraphError(f"close_loops: max_drift {max_drift}, min_overlap {min_overlap}, max_rms {max_rms}, batch {batch}")
    geo = [frames[i] for i in ids]
    pts, msk = torch.stack([g[0] for g in geo]), torch.stack([g[2] for g in geo])
    desc, sums = place.describe(pts, msk, z_lo, rings, sectors, r_min, r_max, z_step, up)
    best_d, best_s = place.match(desc, gap)
    cand = place.candidates(best_d, best_s, sums, top, max_score)           # the one host read of the matcher's tables
    _, length = path_lengths(poses)
    P = [_pose34("a pose", poses[i]) for i in ids]
    reach = (float(r_max) - float(r_min)) / int(rings)
    report = {"gap": int(gap), "top": int(top), "max_score": float(max_score), "rings": int(rings), "sectors": int(sectors), "max_drift": float(max_drift),
              "reach": reach, "min_overlap": float(min_overlap), "max_rms": float(max_rms), "candidates": len(cand), "accepted": [], "rejected": []}
    todo = []
    for i, j, sc, s in cand:
        row = {"source": ids[i], "target": ids[j], "score": sc, "shift": s}
        dist, path = float(np.linalg.norm(P[i][:, 3] - P[j][:, 3])), float(length[i] - length[j])
        if dist > float(max_drift) * path + reach:
            report["rejected"].append(dict(row, reason=f"the chain puts the sensors {dist:.3f} m apart: more than max_drift {float(max_drift)} x the path of "
                                                       f"{path:.3f} m plus the reach of {reach:.3f} m"))
        else:
            todo.append((i, j, row))
    edges = []
    n_valid = msk.reshape(len(ids), -1).ne(0).sum(1).cpu().numpy()
    for k0 in range(0, len(todo), int(batch)):
        part = todo[k0:k0 + int(batch)]
        si, tj = [i for i, _, _ in part], [j for _, j, _ in part]
        src = tuple(torch.stack([geo[i][k] for i in si]) for k in range(3))
        tgt = tuple(torch.stack([geo[j][k] for j in tj]) for k in range(3))
        init = torch.from_numpy(np.stack([place.shift_to_init(row["shift"], sectors, up) for _, _, row in part])).to(pts.device)
        reg = rg.align(src, tgt, init, schedule, huber, lam, min_pairs, tol_t, tol_r, data_type, inclination, sensor2ego, min_depth, max_depth)
        X, hess, status, last = (t.cpu().numpy() for t in (reg.X, reg.hessian, reg.status, reg.log[:, -1]))
        for k, (i, j, row) in enumerate(part):
            partners, swe, sw_ = float(last[k, 0]), float(last[k, 1]), float(last[k, 2])
            rms = math.sqrt(swe / sw_) if sw_ > 0.0 else math.inf
            overlap = partners / max(int(n_valid[i]), 1)
            row = dict(row, status=int(status[k]), partners=int(partners), overlap=overlap, rms=rms)
            if int(status[k]) in (rg.FEW, rg.PIVOT):
                report["rejected"].append(dict(row, reason=f"the alignment ended with status {int(status[k])}"))
            elif not (int(status[k]) == rg.CONVERGED or overlap >= float(min_overlap)):
                report["rejected"].append(dict(row, reason=f"not converged and {overlap:.3f} of the source's valid pixels as partners: fewer than min_overlap {float(min_overlap)}"))
            elif not rms <= float(max_rms):
                report["rejected"].append(dict(row, reason=f"a weighted rms residual of {rms:.4f} m: more than max_rms {float(max_rms)}"))
            else:
                report["accepted"].append(row)
                edges.append(dict(row, a=ids[j], b=ids[i], Z=X[k].copy(), info=hess[k].copy(), kind="loop"))
    return edges, report


# ---- the solve -------------------------------------------------------------------------------------------------------------------------------------------------

def _cost(P, E):
    return sum(float(r @ info @ r) for r, info in ((residual(Z, P[a], P[b]), info) for a, b, Z, info in E))


def _normal(P, E, col, n):
    """(H, g) = (sum J^T info J, sum J^T info r) over the edges, the fixed pose (col < 0) left out."""
    H, g = np.zeros((n, n)), np.zeros(n)
    for a, b, Z, info in E:
        r, Ja, Jb = jacobians(Z, P[a], P[b])
        for (u, Ju) in ((a, Ja), (b, Jb)):
            if col[u] < 0:
                continue
            g[col[u]:col[u] + 6] += Ju.T @ (info @ r)
            for (v, Jv) in ((a, Ja), (b, Jb)):
                if col[v] >= 0:
                    H[col[u]:col[u] + 6, col[v]:col[v] + 6] += Ju.T @ info @ Jv
    return H, g


def normal_matrix(poses, edges):
    """The (6 (F - 1), 6 (F - 1)) normal matrix of ``optimize`` at ``poses``: its condition number bounds how far the minimiser moves with the edges."""
    ids = sorted(int(i) for i in poses)
    col = {i: 6 * (k - 1) for k, i in enumerate(ids)}
    return _normal({i: _pose34("a pose", poses[i]) for i in ids}, [_edge(e) for e in edges], col, 6 * (len(ids) - 1))[0]


def optimize(poses, edges, max_iter=DEFAULT_MAX_ITER, tol=DEFAULT_TOL, lam=1e-6):
    """({id: (4, 4) float64}, report): the poses that minimise ``sum r^T info r`` over ``edges`` (see the module text), the lowest id fixed.  The
    iteration ends when the cost or its gradient is zero, when a step is smaller than ``tol`` in every coordinate (that step is not taken), or
    after ``max_iter`` accepted steps.  The report: ``cost`` per iteration (the first entry is the chain's), ``iterations``, ``converged`` and, per
    edge that is not an odometry edge, its residual (|rho|, |phi|) before and after next to what ``close_loops`` recorded."""
    ids = sorted(int(i) for i in poses)
    n = 6 * (len(ids) - 1)
    if n > MAX_UNKNOWNS:
        raise PoseGraphError(f"optimize: {len(ids)} poses are {n} unknowns; the dense solve supports 6 (F - 1) <= {MAX_UNKNOWNS}")
    if len(ids) < 1:
        raise PoseGraphError("optimize: no poses")
    col = {i: 6 * (k - 1) for k, i in enumerate(ids)}                        # the lowest id sits at -6: fixed
    P = {i: _pose34("a pose", poses[i]) for i in ids}
    E = [_edge(e) for e in edges]
    for a, b, _, _ in E:
        if a not in P or b not in P or a == b:
            raise PoseGraphError(f"optimize: an edge between {a} and {b} (two different ids of the poses)")
    norms = lambda: [(float(np.linalg.norm(r[:3])), float(np.linalg.norm(r[3:]))) for r in (residual(Z, P[a], P[b]) for a, b, Z, _ in E)]
    before = norms()
    cost = _cost(P, E)
    costs, it, converged = [cost], 0, False
    while it < int(max_iter) and n > 0:
        if cost == 0.0:
            converged = True
            break
        H, g = _normal(P, E, col, n)
        if not g.any():
            converged = True
            break
        step = None
        while step is None:
            try:
                L = np.linalg.cholesky(H + lam * np.diag(np.diag(H)) + 1e-12 * np.eye(n))
            except np.linalg.LinAlgError:
                lam *= 10.0
                if lam > 1e12:
                    raise PoseGraphError("optimize: the normal matrix is not positive definite: a node without an edge to the rest?") from None
                continue
            d = -np.linalg.solve(L.T, np.linalg.solve(L, g))
            if float(np.abs(d).max()) < float(tol):
                converged = True
                break
            trial = dict(P)
            for i in ids[1:]:
                Re, te = rg.exp_reference(d[col[i]:col[i] + 6])
                trial[i] = _compose(P[i], Re, te)
            c = _cost(trial, E)
            if c < cost:
                step, P, cost = d, trial, c
                lam = max(lam / 3.0, 1e-12)
            else:
                lam *= 10.0
                if lam > 1e12:                                                 # no descent left at any damping: the minimum, to rounding
                    converged = True
                    break
        if converged:
            break
        it += 1
        costs.append(cost)
    after = norms()
    out = {}
    for i in ids:
        T = np.eye(4)
        T[:3] = P[i]
        out[i] = T
    if n == 0 or not E:
        converged = True
    loops = []
    for k, e in enumerate(edges):
        if e.get("kind", "loop") == "odometry":
            continue
        loops.append({"a": E[k][0], "b": E[k][1], "kind": e.get("kind", "loop"), "score": e.get("score"), "shift": e.get("shift"), "partners": e.get("partners"),
                      "rms": e.get("rms"), "before": list(before[k]), "after": list(after[k])})
    return out, {"cost": costs, "iterations": it, "converged": bool(converged), "unknowns": n, "edges": len(E), "loops": loops}


def closure_error(poses, a, b, Z):
    """(|rho|, |phi|) of Log(Z^-1 T_a^-1 T_b): how far the poses are from closing the loop that ``Z`` measures."""
    r = residual(_pose34("Z", Z), _pose34("a pose", poses[a]), _pose34("a pose", poses[b]))
    return float(np.linalg.norm(r[:3])), float(np.linalg.norm(r[3:]))
