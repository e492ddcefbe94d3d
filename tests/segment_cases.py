"""Seeded cases of the range-image segmentation (lidar_rt_amd/segmentation.py) and of the actor discovery (lidar_rt_amd/actors.py), shared by
tests/test_segmentation.py, tests/test_segmentation_gpu.py and tests/test_actors.py.

LABELLING.  The pattern cases put the pixels on a cylinder of radius 0.1 W / 2 pi with rows 0.05 m apart: 4-neighbours are 0.1 m or 0.05 m apart
(joined under d_abs = 0.15, c = 0), pixels two apart are not, and the column seam w = W - 1 <-> 0 is a neighbourhood like any other.  The mask
draws the shape.  `threshold_abs` / `threshold_dir` use points that float32 represents exactly: one pair with d2 == the bound (joined), one with
d2 exactly one ulp above it (not joined), horizontally and vertically, and one pair with a NaN coordinate.

WORLD.  The room of tests/registration_cases.py (its floor is z = -1.8) with boxes of 4.6 x 2.1 x 1.5 m standing 0.25 m above the floor; ranges are
ray-plane and ray-slab intersections, so every pixel's primitive is known (0..7 the room's planes, 8 + b box b).  SCENARIO: eight frames of
32 x 2048; box A moves 0.6 m per frame along x, box B (-0.5, 0.3) m per frame, box C is parked; the sensor advances 0.4 m and 0.01 rad per frame,
1.7 m above the floor; the poses are the true ones.  Why 2048 columns and not 512: a face seen beyond the 76 degrees of incidence that the default
c_h allows falls apart into one segment per column, too small to be candidates, and their returns may then lie outside the track's box; in this
small room every box shows such a face in some frame.  At 2048 columns neighbouring returns on a face 2 to 6 m away stay within d_abs = 0.15 m up
to 84 degrees, and what remains beyond that lies inside the union of the other frames' views.  The room is 15 m x 18 m with two slanted walls:
with these sizes and speeds it cannot hold 2 m between every two things in every frame, so the layout keeps at least 1 m between a box and a
wall or another box (more where there is room) -- tighter than 2 m, and harder for the segmentation, never easier.

RECORDED holds what the committed twin gives on the scenario: per actor the largest centre error [m], yaw error [rad] and size excess over the
true box [m].  tests/test_actors.py asserts twice these and nothing looser.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from lidar_rt_amd import segmentation as sg
from tests import registration_cases as rc

# ---- labelling ------------------------------------------------------------------------------------------------------------------------------------------------

PATTERN_KW = dict(d_abs=0.15, c_h=0.0, c_v=0.0)


def cylinder(H, W):
    R = 0.1 * W / (2.0 * math.pi)
    w = np.arange(W) * (2.0 * math.pi / W)
    p = np.stack([np.broadcast_to(R * np.cos(w), (H, W)), np.broadcast_to(R * np.sin(w), (H, W)), np.broadcast_to(0.05 * np.arange(H)[:, None], (H, W))], -1)
    return p.astype(np.float32)


def _pattern(name, H, W):
    m = np.zeros((H, W), bool)
    if name == "seam":
        m[2, [W - 3, W - 2, W - 1, 0, 1, 2]] = True
    elif name == "serpent":
        m[0::2] = True
        m[0::2, W // 2] = False                                              # every long row is whole only through the seam
        for k, h in enumerate(range(1, H, 2)):
            m[h, W - 1 if k % 2 == 0 else 0] = True
    elif name == "u_shape":
        m[:H - 1, 10] = m[:H - 1, W - 14] = True
        m[H - 1, 10:W - 13] = True
    elif name == "checker":
        m[(np.add.outer(np.arange(H), np.arange(W)) % 2) == 0] = True
    elif name == "diagonal":
        m[np.arange(W) % H, np.arange(W)] = True
    elif name == "full":
        m[:] = True
    elif name != "empty":
        raise KeyError(name)
    return m


_SHAPES = {"seam": (6, 40), "serpent": (16, 130), "u_shape": (8, 64), "checker": (8, 64), "diagonal": (8, 64), "odd": (5, 37), "empty": (8, 64), "full": (8, 64),
           "random_3": (16, 128), "random_6": (16, 128), "random_9": (16, 128), "threshold_abs": (2, 12), "threshold_dir": (2, 12)}
LABEL_KEYS = tuple(_SHAPES)
RANDOM_KEYS = ("random_3", "random_6", "random_9")


def _threshold(kind):
    """(points (2, 12, 3), mask, kw, expected labels)."""
    e = 2.0 ** -12                                                            # e * e = 2^-24 = one ulp of 0.5625
    if kind == "abs":
        a, tie, above, kw = (1.0, 0.0, 0.0), (1.75, 0.0, 0.0), (1.75, e, 0.0), dict(d_abs=0.75, c_h=0.0, c_v=0.0)
    else:                                                                     # bound = 0.25 * min(r2) = 0.25 * 2.25
        a, tie, above, kw = (1.5, 0.0, 0.0), (1.5, 0.75, 0.0), (1.5, 0.75, e), dict(d_abs=0.0, c_h=0.5, c_v=0.5)
    p = np.zeros((2, 12, 3), np.float32)
    m = np.zeros((2, 12), bool)
    for (h, w), v in {(0, 0): a, (0, 1): tie, (0, 3): a, (0, 4): above, (0, 6): a, (1, 6): tie, (0, 8): a, (1, 8): above, (0, 10): a,
                      (0, 11): (float("nan"), 0.0, 0.0)}.items():
        p[h, w], m[h, w] = v, True
    want = np.full((2, 12), -1, np.int32)
    for (h, w), v in {(0, 0): 0, (0, 1): 0, (0, 3): 3, (0, 4): 4, (0, 6): 6, (1, 6): 6, (0, 8): 8, (1, 8): 20, (0, 10): 10, (0, 11): 11}.items():
        want[h, w] = v
    return p, m, kw, want


@functools.lru_cache(maxsize=None)
def label_case(key):
    """points (H, W, 3), mask (H, W), ev (two int8 images), kw of label; expected: the labels where the case knows them."""
    H, W = _SHAPES[key]
    expected = None
    if key.startswith("threshold"):
        p, m, kw, expected = _threshold(key.split("_")[1])
    elif key.startswith("random") or key == "odd":
        seed, density = {"random_3": (3, 0.3), "random_6": (6, 0.6), "random_9": (9, 0.9), "odd": (5, 0.6)}[key]
        rng = np.random.default_rng(seed)
        p = (cylinder(H, W) + rng.normal(0.0, 0.03, (H, W, 3))).astype(np.float32)
        m = rng.random((H, W)) < density
        kw = dict(d_abs=0.12, c_h=0.02, c_v=0.03)
    else:
        p, m, kw = cylinder(H, W), _pattern(key, H, W), dict(PATTERN_KW)
    rng = np.random.default_rng(100 + len(key))
    ev = tuple(torch.from_numpy(rng.integers(-1, 2, (H, W)).astype(np.int8)) for _ in range(2))
    return SimpleNamespace(key=key, H=H, W=W, points=torch.from_numpy(p), mask=torch.from_numpy(m), ev=ev, kw=kw,
                           expected=None if expected is None else torch.from_numpy(expected))


@functools.lru_cache(maxsize=None)
def label_reference(key):
    c = label_case(key)
    return sg.label_reference(c.points, c.mask, **c.kw)


@functools.lru_cache(maxsize=None)
def stats_reference(key, s_max=512):
    c = label_case(key)
    return sg.stats_reference(c.points, label_reference(key), c.ev, s_max)


# ---- the world ------------------------------------------------------------------------------------------------------------------------------------------------

BOX_SIZE = np.array([4.6, 2.1, 1.5])
BOX_Z = -1.8 + 0.25 + 0.75
SENSOR_HEIGHT = 1.7                                                           # the scenario's sensor: below the boxes' tops, which it therefore never sees


def world_depth(d_local, pose, boxes):
    """(depth (H, W) float32, primitive (H, W) int64) of a sensor at `pose` in the room with `boxes` = [(centre (3,), yaw)]."""
    d = d_local.numpy().astype(np.float64) @ pose[:3, :3].T
    o = pose[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (rc.PLANES[:, 3] - rc.PLANES[:, :3] @ o)[None, None, :] / (d @ rc.PLANES[:, :3].T)
        t = np.where(t > 0.0, t, np.inf)
        for c, yaw in boxes:
            cy, sy = math.cos(yaw), math.sin(yaw)
            R = np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]])
            ol, dl = R.T @ (o - np.asarray(c)), d @ R                         # the ray in the box's frame
            t0, t1 = (-0.5 * BOX_SIZE - ol) / dl, (0.5 * BOX_SIZE - ol) / dl
            near, far = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
            hit = (near <= far) & (near > 0.0)
            t = np.concatenate([t, np.where(hit, near, np.inf)[..., None]], -1)
    return torch.from_numpy(t.min(-1).astype(np.float32)), t.argmin(-1)


def world_frame(H, W, inc, data_type, s2e, pose, boxes):
    """(points, depth, mask, primitive) of one frame."""
    d_local = rc.local_directions(H, W, inc, data_type, s2e)
    depth, prim = world_depth(d_local, pose, boxes)
    mask = torch.isfinite(depth) & (depth > 0)
    depth = torch.where(mask, depth, torch.zeros_like(depth))
    pts, mask = sg.frame_points(depth, mask, inc, H, W, data_type, s2e)
    return pts, depth, mask, prim


def yaw_pose(x, y, yaw, z=0.0):
    T = np.eye(4)
    T[:2, :2] = [[math.cos(yaw), -math.sin(yaw)], [math.sin(yaw), math.cos(yaw)]]
    T[:3, 3] = (x, y, z)
    return T


SCENARIO = dict(H=32, W=2048, F=8, inc=list(rc.BOUNDS))
B_YAW = math.atan2(0.3, -0.5)


def scenario_boxes(k):
    """[(centre, yaw)] of A, B, C in frame k."""
    return [(np.array([-0.2 + 0.6 * k, -3.0, BOX_Z]), 0.0), (np.array([4.2 - 0.5 * k, 1.3 + 0.3 * k, BOX_Z]), B_YAW), (np.array([-4.0, 2.5, BOX_Z]), 0.5 * math.pi)]


def scenario_pose(k):
    return yaw_pose(-2.5 + 0.4 * k, -0.5, 0.01 * k, z=-1.8 + SENSOR_HEIGHT)


@functools.lru_cache(maxsize=None)
def scenario():
    """frames {id: (points, depth, mask)}, poses {id: (4, 4)}, prim {id: (H, W)}, kw: the sensor model."""
    s = SCENARIO
    frames, poses, prim = {}, {}, {}
    for k in range(s["F"]):
        fid = 100 + k
        poses[fid] = scenario_pose(k)
        pts, depth, mask, pr = world_frame(s["H"], s["W"], s["inc"], "KITTI", None, poses[fid], scenario_boxes(k))
        frames[fid], prim[fid] = (pts, depth, mask), pr
    return SimpleNamespace(frames=frames, poses=poses, prim=prim, ids=sorted(frames), kw=dict(inclination=s["inc"], data_type="KITTI", sensor2ego=None))


@functools.lru_cache(maxsize=None)
def scenario_result():
    """actors.discover on the scenario with the twins, computed once and shared."""
    from lidar_rt_amd import actors
    sc = scenario()
    return actors.discover(sc.frames, sc.poses, SENSOR_HEIGHT, **sc.kw)


# per actor (A, B): the largest centre error [m], yaw error [rad] and size excess [m] the committed twin gives (tests/test_actors.py prints them)
RECORDED = {"A": (4.159e-01, 1.163e-01, 7.748e-01), "B": (1.013e+00, 2.083e-01, 1.700e+00)}


# ---- ground, free space, bounds -------------------------------------------------------------------------------------------------------------------------------

def ground_columns():
    """Analytic columns, 6 rows x 4 columns, bounds with the last inclination the larger (rows are visited from row 5 up to row 0), sensor 1.8 m up:
    column 0: floor, floor, a car (two pixels), the floor again behind it, a wall;  column 1: nothing in the band -- no ground at all;
    column 2: the first pixel is masked out, then floor, then a ramp steeper than the slope;  column 3: a ramp gentler than the slope, climbing out of the band."""
    z = -1.8
    cols = [[(3.0, 0.0, z), (4.0, 0.0, z), (5.0, 0.0, z + 0.6), (5.0, 0.0, z + 1.2), (9.0, 0.0, z + 0.02), (12.0, 0.0, 1.0)],
            [(3.0, 1.0, -0.9), (4.0, 1.0, -0.8), (5.0, 1.0, -0.7), (6.0, 1.0, -0.6), (7.0, 1.0, -0.5), (8.0, 1.0, 0.0)],
            [(3.0, 2.0, z), (4.0, 2.0, z), (5.0, 2.0, z + 0.01), (6.0, 2.0, z + 0.5), (7.0, 2.0, z + 1.0), (8.0, 2.0, z + 1.5)],
            [(3.0, 3.0, z), (4.0, 3.0, z + 0.1), (5.0, 3.0, z + 0.2), (6.0, 3.0, z + 0.3), (7.0, 3.0, z + 0.45), (8.0, 3.0, z + 0.6)]]
    p = np.zeros((6, 4, 3), np.float32)
    for w, col in enumerate(cols):
        for k, v in enumerate(col):
            p[5 - k, w] = v                                                  # k-th visited pixel sits in row 5 - k
    m = np.ones((6, 4), bool)
    m[5, 2] = False
    want = np.zeros((6, 4), np.uint8)
    for w, flags in enumerate([(1, 1, 0, 0, 1, 0), (0, 0, 0, 0, 0, 0), (0, 1, 1, 0, 0, 0), (1, 1, 1, 1, 1, 1)]):
        for k, v in enumerate(flags):
            want[5 - k, w] = v
    return torch.from_numpy(p), torch.from_numpy(m), [-0.4, 0.1], torch.from_numpy(want)


_FREE = {"room": (16, 128, rc.BOUNDS, "KITTI", None, rc.twist(41, 0.4, 1.0)), "waymo": (8, 40, "table", "Waymo", rc.WAYMO_S2E, rc.twist(42, 0.15, 1.5)),
         "yaw": (16, 128, rc.BOUNDS, "KITTI", None, rc.twist(43, 0.05, 8.0, yaw_only=True)), "empty": (16, 128, rc.BOUNDS, "KITTI", None, rc.twist(44, 0.3, 1.0))}
FREE_KEYS = tuple(_FREE)


@functools.lru_cache(maxsize=None)
def free_case(key):
    """src (points, mask), tgt (range, mask), X (3, 4): the target sensor at the identity with a slab at one place, the source at Exp(xi) with the slab moved."""
    H, W, inc, data_type, s2e, xi = _FREE[key]
    inc = rc.waymo_table(H) if inc == "table" else list(inc)
    X = rc.exp4(xi)
    slab = lambda y: [(np.array([4.5, y, BOX_Z]), 0.3)]
    sp, _, sm, _ = world_frame(H, W, inc, data_type, s2e, X, slab(1.0))
    _, tr, tm, _ = world_frame(H, W, inc, data_type, s2e, np.eye(4), slab(-2.5))
    if key == "empty":
        tm = torch.zeros_like(tm)
    return SimpleNamespace(key=key, H=H, W=W, src=(sp, sm), tgt=(tr, tm), X=torch.from_numpy(X[:3].copy()), kw=dict(inclination=inc, data_type=data_type, sensor2ego=s2e))


@functools.lru_cache(maxsize=None)
def bounds_case():
    """Two tracks over three frames of 8 x 64: points, seg, track_of (3, 8), pose (2, 3, 3, 4)."""
    rng = np.random.default_rng(77)
    F, H, W, S = 3, 8, 64, 8
    p = rng.normal(0.0, 6.0, (F, H, W, 3)).astype(np.float32)
    seg = rng.integers(-1, S, (F, H, W)).astype(np.int32)
    track_of = np.array([[0, -1, 1, -1, 0, -1, -1, 1], [-1, 0, -1, 1, -1, -1, 0, -1], [1, 1, -1, -1, -1, 0, -1, -1]], np.int32)
    pose = np.stack([np.stack([rc.exp4(rc.twist(200 + 10 * t + f, 3.0, 40.0))[:3] for f in range(F)]) for t in range(2)])
    return SimpleNamespace(points=torch.from_numpy(p), seg=torch.from_numpy(seg), track_of=torch.from_numpy(track_of), pose=torch.from_numpy(pose))
