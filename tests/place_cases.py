"""Seeded cases of the place matcher and the pose graph (lidar_rt_amd/place.py, lidar_rt_amd/pose_graph.py), shared by tests/test_place.py,
tests/test_pose_graph.py and tests/test_place_gpu.py.

The shapes are the smallest at which the kernels can still go wrong: frames of 5 x 37 (one frame, a multiple of nothing), 16 x 128 (five frames)
and 8 x 40 (nine frames: with the tile of 16 candidates a candidate count that is no multiple of it, and waves without a candidate); grids of
4 x 8, 20 x 60 (a ring count that is no multiple of 4 is 5 x 8 in the tests) and 32 x 128 (two passes of a wave over the shifts; a sector stride
of 8 dwords, the one the padding exists for).  The 32 x 128 grid needs ``sectors <= W``: it goes with the W = 128 frames only, the others assert
the refusal.  A batch has an all-invalid frame in its middle and two frames that are equal (the tie on ``j`` in ``candidates``).

THE ROOM TOUR.  Nine frames at 16 x 128 in the analytic room of tests/registration_cases.py (imported, not edited): the sensor walks a circle of
1 m radius and ends 0.3 m and 3 degrees from its start, so with ``gap = 8`` only the closing pair (8, 0) is eligible.  The descriptor's range is
the room's (``r_max = 20``).  This was the first seeded tour tried; the twin satisfies every condition of the tests on it.

THE THRESHOLDS ``place.DEFAULT_MAX_SCORE``, ``pose_graph.DEFAULT_MIN_OVERLAP`` and ``pose_graph.DEFAULT_MAX_RMS`` cannot be derived.  They were set
from what the twin sees on the tour with ``gap = 0``, every pair aligned from its shift with ``pose_graph.LOOP_SCHEDULE`` (all 36 pairs: the
table of profiles/place.md; TOUR_TABLE holds the rows that decide).  For the matcher the true revisit is the pair within 0.5 m and 5 degrees,
(8, 0), and every other pair is none.  For the verification every pair of this one room overlaps, so "true" is an alignment that settled
(overlap 0.767 to 0.870, rms 0.0154 to 0.0237 m, 24 pairs) and "false" one that did not (overlap 0.347 to 0.492, rms 0.0330 to 0.0721 m, 12 pairs,
all of them 1.36 m or more apart); there is nothing in between.

    max_score   = (0.208 + 0.354) / 2   = 0.28       the revisit (8, 0) against the best pair that is none, (4, 3), neighbours 0.73 m apart
    min_overlap = (0.767 + 0.492) / 2   = 0.63       (6, 3) against (7, 3)
    max_rms     = (0.0237 + 0.0330) / 2 = 0.028 m    (5, 1) against (7, 4)

Scenes of tools/make_sequence.py and real scans were not measured.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from lidar_rt_amd import place, pose_graph as pg, registration as rg
from tests import registration_cases as rc

SHAPES = ((1, 5, 37), (5, 16, 128), (9, 8, 40))
GRIDS = ((4, 8), (20, 60), (32, 128))
ODD_GRID = (5, 8)                                                            # rings that are no multiple of 4
RULE = dict(r_min=2.0, r_max=30.0, z_step=0.025, up=(0.0, 0.0, 1.0))
Z_LO = -1.75


@functools.lru_cache(maxsize=None)
def frames(F, H, W):
    """Seeded points (F, H, W, 3) float32 and mask (F, H, W) bool: ground ranges from inside r_min to beyond r_max, heights from below z_lo to
    above the 255 clamp, a few NaN coordinates under a set mask, the middle frame all invalid, the last frame equal to the first."""
    rng = np.random.default_rng(1000 * F + H * W)
    rho = rng.uniform(0.5, 36.0, size=(F, H, W))
    az = rng.uniform(-math.pi, math.pi, size=(F, H, W))
    h = rng.uniform(-2.5, 6.5, size=(F, H, W))
    p = np.stack([rho * np.cos(az), rho * np.sin(az), h], -1).astype(np.float32)
    p[rng.uniform(size=(F, H, W)) < 0.01] = np.nan
    mask = rng.uniform(size=(F, H, W)) < 0.8
    if F > 2:
        mask[F // 2] = False
        p[F - 1], mask[F - 1] = p[0], mask[0]
    return torch.from_numpy(p), torch.from_numpy(mask)


@functools.lru_cache(maxsize=None)
def described(F, H, W, NR, NS):
    """The twin's descriptors of frames(F, H, W), computed once and shared."""
    p, m = frames(F, H, W)
    return place.describe_reference(p, m, Z_LO, NR, NS, **RULE)


@functools.lru_cache(maxsize=None)
def matched(F, H, W, NR, NS, gap):
    return place.match_reference(described(F, H, W, NR, NS)[0], gap)


def margin(F, H, W, NR, NS):
    """The smallest distance of a float64 decision of describe from its threshold, relative to the threshold's scale."""
    p, m = frames(F, H, W)
    q = p.numpy().astype(np.float64)[m.numpy()]
    q = q[np.isfinite(q).all(-1)]
    rho, h = np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + 0.0), q[:, 2]
    a = (rho - RULE["r_min"]) * NR / (RULE["r_max"] - RULE["r_min"])
    b = (h - Z_LO) / RULE["z_step"]
    return float(min(np.abs(a - np.rint(a)).min(), np.abs(b - np.rint(b)).min()))


# ---- frames built per column: membership is exact ------------------------------------------------------------------------------------------------------------

COLUMN = dict(H=6, W=120, NR=20, NS=60)


def column_azimuth(W):
    """The azimuth of column w of the KITTI ray grid: (W - w) / W 2 pi - pi (RangeFrames.range_rays)."""
    return (W - np.arange(W)) / W * 2.0 * math.pi - math.pi


@functools.lru_cache(maxsize=None)
def column_frame():
    """(points (H, W, 3) float32, mask): every pixel sits at the azimuth of its own column, in the middle of a seeded ring and of a seeded height
    step, so that float32 rounding cannot move it to another cell."""
    H, W, NR = COLUMN["H"], COLUMN["W"], COLUMN["NR"]
    rng = np.random.default_rng(77)
    ring, step = rng.integers(0, NR, size=(H, W)), rng.integers(0, 200, size=(H, W))
    rho = RULE["r_min"] + (ring + 0.5) * (RULE["r_max"] - RULE["r_min"]) / NR
    h = Z_LO + (step + 0.5) * RULE["z_step"]
    az = column_azimuth(W)[None, :]
    p = np.stack([rho * np.cos(az), rho * np.sin(az), h], -1).astype(np.float32)
    return torch.from_numpy(p), torch.from_numpy(rng.uniform(size=(H, W)) < 0.9)


def yawed(points, mask, k):
    """What a sensor sees that stands where the sensor of (points, mask) stands, yawed by ``k`` sectors about ``up``: X = T_j^-1 T_i = Rz(alpha),
    alpha = 2 pi k / NS, every point p_i = X^-1 p_j, and the point lands in the column whose azimuth it now has -- ``k W / NS`` columns later,
    because the azimuth falls with the column.  Returns (points, mask, X (3, 4))."""
    W, NS = COLUMN["W"], COLUMN["NS"]
    alpha = 2.0 * math.pi * k / NS
    c, s = math.cos(alpha), math.sin(alpha)
    X = np.array([[c, -s, 0.0, 0.0], [s, c, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])
    q = points.numpy().astype(np.float64) @ X[:, :3]                         # rows p^T R = (R^T p)^T
    az = np.arctan2(q[..., 1], q[..., 0])
    col = np.rint((math.pi - az) / (2.0 * math.pi) * W).astype(np.int64) % W  # the inverse of column_azimuth
    assert np.array_equal(col, (np.arange(W)[None, :] + k * W // NS) % W * np.ones_like(col))
    out_p, out_m = np.zeros_like(q, dtype=np.float32), np.zeros(mask.shape, bool)
    rows = np.arange(q.shape[0])[:, None] * np.ones_like(col)
    out_p[rows, col], out_m[rows, col] = q.astype(np.float32), mask.numpy()
    return torch.from_numpy(out_p), torch.from_numpy(out_m), X


# ---- the room tour -------------------------------------------------------------------------------------------------------------------------------------------

TOUR = dict(n=9, H=16, W=128, gap=8, sensor_height=1.8, r_max=20.0)
TOUR_KW = dict(inclination=list(rc.BOUNDS), data_type="KITTI", sensor2ego=None)


def _pose(x, y, yaw, z):
    T = np.eye(4)
    c, s = math.cos(yaw), math.sin(yaw)
    T[:2, :2] = [[c, -s], [s, c]]
    T[:3, 3] = [x, y, z]
    return T


def tour_truth():
    n, R, miss, yaw_end = TOUR["n"], 1.0, 0.3, math.radians(3.0)
    out = {}
    for k in range(n):
        a = 2.0 * math.pi * k / (n - 1) * (1.0 - miss / (2.0 * math.pi * R))
        out[k] = _pose(R * math.sin(a) + 0.5, R * (1.0 - math.cos(a)) - 1.0, 0.15 * math.sin(a) + yaw_end * k / (n - 1), 0.03 * math.sin(2.0 * a))
    return out


@functools.lru_cache(maxsize=None)
def tour():
    """frames {id: geometry}, truth {id: (4, 4)}: the closed tour, CPU tensors."""
    truth = tour_truth()
    return {i: rc.geometry(TOUR["H"], TOUR["W"], TOUR_KW["inclination"], "KITTI", None, P) for i, P in truth.items()}, truth


def tour_on(dev):
    fr, truth = tour()
    return {i: tuple(t.to(dev) for t in g) for i, g in fr.items()}, truth


def run_tour(fr, truth):
    """The whole path on the frames' device: odometry with its steps, the loops, the solve."""
    chain, rep = rg.odometry(fr, first_pose=truth[0], return_steps=True, **TOUR_KW)
    loops, lrep = pg.close_loops(fr, chain, rep["steps"], sensor_height=TOUR["sensor_height"], gap=TOUR["gap"], r_max=TOUR["r_max"], **TOUR_KW)
    solved, srep = pg.optimize(chain, pg.odometry_edges(rep["steps"]) + loops)
    return SimpleNamespace(chain=chain, steps=rep["steps"], loops=loops, loop_report=lrep, solved=solved, solve_report=srep)


@functools.lru_cache(maxsize=None)
def tour_reference():
    """run_tour on the twins, computed once and shared."""
    return run_tour(*tour())


def closing_truth():
    truth = tour_truth()
    return pg.relative(truth[0][:3], truth[TOUR["n"] - 1][:3])


# what the twin gives on the tour.  align_alone: align_reference on the closing pair from the identity with pose_graph.LOOP_SCHEDULE, its error against
# the truth (|t - t_true| m, angle rad); closure_chain / closure_solved: Log(Z_true^-1 T_0^-1 T_8) of the chain's and of the corrected poses (|rho|, |phi|)
RECORDED_TOUR = {
    "align_alone": (6.086e-03, 1.897e-03),
    "closure_chain": (8.513e-03, 2.414e-03),
    "closure_solved": (4.575e-03, 1.433e-03),
}

# (i, j, distance m, score, overlap, rms m, status) of the deciding pairs, as the twin gives them with gap = 0, top = 9, max_score = 1 and the gates open
TOUR_TABLE = ((8, 0, 0.299, 0.208, 0.850, 0.0164, 3), (4, 3, 0.731, 0.354, 0.870, 0.0184, 3), (6, 3, 1.802, 0.694, 0.767, 0.0170, 3),
              (7, 3, 1.994, 0.591, 0.492, 0.0350, 3), (5, 1, 1.994, 0.683, 0.801, 0.0237, 3), (7, 4, 1.802, 0.616, 0.485, 0.0330, 3))


# ---- the seeded closed trajectory of the pose graph ------------------------------------------------------------------------------------------------------------

GRAPH = dict(n=40, info=400.0, bias=(2.0e-3, -1.0e-3, 5.0e-4, 2.0e-5, -3.0e-5, 4.0e-5))


def exp34(xi):
    Re, te = rg.exp_reference(np.asarray(xi, np.float64))
    return np.concatenate([Re, te[:, None]], 1)


@functools.lru_cache(maxsize=None)
def trajectory():
    """truth {id: (4, 4)} on a closed curve (a circle of 8 m radius with a seeded wobble; the last pose is the first again), the chain built from
    the true steps times Exp(bias) each, the odometry edges (Z = the biased step, info = c I) and the exact loop edge.  The sensor keeps its
    heading within 0.2 rad and the bias is mostly a translation, so the chain's error grows in proportion to the path and the even spread of the
    correction over equal edges helps every node.  A first trajectory whose sensor turned once around with a yaw bias of 6e-4 rad per step was
    dropped: there the error grows with the square of the path, the even spread overcorrects the first nodes, and nodes 2 to 6 ended up to 0.8 mm
    further from the truth than the chain had them -- a property of that drift, not of the solver."""
    n, rng = GRAPH["n"], np.random.default_rng(5)
    wob = rng.normal(size=(n, 3)) * 0.05
    truth = {}
    for k in range(n):
        a = 2.0 * math.pi * k / (n - 1)
        T = _pose(8.0 * math.sin(a), 8.0 * (1.0 - math.cos(a)), 0.2 * math.sin(a), 0.0)
        if 0 < k < n - 1:
            T[:3] = pg._compose(T[:3], *rg.exp_reference(np.concatenate([wob[k], 0.3 * wob[k][::-1]])))
        truth[k] = T
    bias = exp34(GRAPH["bias"])
    chain, edges = {0: truth[0].copy()}, []
    for k in range(1, n):
        Z = pg._compose(pg.relative(truth[k - 1][:3], truth[k][:3]), bias[:, :3], bias[:, 3])
        T = np.eye(4)
        T[:3] = pg._compose(chain[k - 1][:3], Z[:, :3], Z[:, 3])
        chain[k] = T
        edges.append({"a": k - 1, "b": k, "Z": Z, "info": GRAPH["info"] * np.eye(6), "kind": "odometry"})
    loop = {"a": n - 1, "b": 0, "Z": pg.relative(truth[n - 1][:3], truth[0][:3]), "info": GRAPH["info"] * np.eye(6), "kind": "loop"}
    return truth, chain, edges, loop


def position_errors(poses, truth):
    return np.array([np.linalg.norm(np.asarray(poses[i])[:3, 3] - truth[i][:3, 3]) for i in sorted(truth)])


# the last pose's position error [m]: of the chain, and after optimize with the one exact loop edge
RECORDED_GRAPH = {"last_chain": 9.864e-02, "last_solved": 6.522e-05}
