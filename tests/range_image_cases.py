"""Seeded cases of the range-image projection, shared by tests/test_range_image.py and tests/test_range_image_gpu.py.

A case is the arguments of ``project_points`` (numpy points) and the twin's result, computed once on the CPU.  Every builder asserts
``margin >= MARGIN`` from the twin: the condition under which two evaluations of the rule whose ``atan2`` differ in the last bits (glibc, the
device's library) must agree on every pixel.  It is a condition on the inputs, not a filter: no point is ever left out of a comparison.
Measured: seeded random clouds of 1 k and 200 k points 3e-4 and 8.6e-6, the grids 0.4999."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from lidar_rt_amd import range_image as ri
from lidar_rt_amd.training import RangeFrames

MARGIN = 1e-9
KITTI_INC = (math.radians(-24.9), math.radians(2.0))
WAYMO_INC = (-0.3125, 0.046875)
YAW = 0.3
SIZES = [(8, 64), (5, 37)]
CONVENTIONS = ("kitti_bounds", "waymo_bounds_yaw", "waymo_table_yaw", "kitti_table_descending")


def sensor2ego(yaw=YAW):
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([[c, -s, 0, 1.5], [s, c, 0, 0.0], [0, 0, 1, 2.0], [0, 0, 0, 1]], np.float32)


def table(H, descending=False, seed=3):
    """H float32-representable beam angles, unevenly spaced, ascending (Waymo's order) or descending."""
    rng = np.random.default_rng(seed)
    t = np.linspace(-0.31, 0.04, H) + rng.uniform(-0.2, 0.2, H) * (0.35 / max(H - 1, 1))
    t = np.sort(t).astype(np.float32).astype(np.float64)
    return (t[::-1] if descending else t).tolist()


def convention(name, H):
    """-> dict(inclination, data_type, sensor2ego)."""
    if name == "kitti_bounds":
        return dict(inclination=list(KITTI_INC), data_type="KITTI", sensor2ego=None)
    if name == "waymo_bounds_yaw":
        return dict(inclination=list(WAYMO_INC), data_type="Waymo", sensor2ego=sensor2ego())
    if name == "waymo_table_yaw":
        return dict(inclination=table(H), data_type="Waymo", sensor2ego=sensor2ego())
    if name == "kitti_table_descending":
        return dict(inclination=table(H, descending=True), data_type="KITTI", sensor2ego=None)
    raise KeyError(name)


def pose(seed):
    """A sensor2world (4, 4) float64: a rotation about a tilted axis and a translation."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(3); a /= np.linalg.norm(a)
    th = rng.uniform(-1.0, 1.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    M = np.eye(4); M[:3, :3] = R; M[:3, 3] = rng.uniform(-30, 30, 3)
    return M


_CACHE = {}


def finish(key, points, H, W, conv, offsets=None, points2sensor=None, max_depth=80.0, min_depth=0.0, wrap=True, check_margin=True, **extra):
    """The case with its twin, computed once per key and left unchanged."""
    if key in _CACHE:
        return _CACHE[key]
    points = np.ascontiguousarray(points, np.float32)
    points.setflags(write=False)
    kw = dict(H=H, W=W, inclination=conv["inclination"], offsets=None if offsets is None else np.asarray(offsets, np.int64), data_type=conv["data_type"],
              sensor2ego=conv["sensor2ego"], points2sensor=points2sensor, max_depth=max_depth, min_depth=min_depth, wrap=wrap)
    twin = ri.project_points_reference(points, **kw)
    if check_margin:
        assert twin.margin >= MARGIN, (key, twin.margin)
    c = SimpleNamespace(key=key, points=points, kw=kw, twin=twin, **extra)
    _CACHE[key] = c
    return c


def ragged_offsets(N, F, rng):
    """F frames over N rows with an EMPTY middle frame (F >= 3) and unequal sizes."""
    if F == 1:
        return np.array([0, N], np.int64)
    cuts = np.sort(rng.integers(0, N + 1, F - 1))
    off = np.concatenate([[0], cuts, [N]]).astype(np.int64)
    if F >= 3:
        off[F // 2 + 1] = off[F // 2]                                          # frame F // 2 is empty
        off = np.maximum.accumulate(off)
    return off


def random_cloud(N, F, H, W, conv_name, seed, wrap=True, transform=False):
    """randn * (20, 20, 2) metres, uniform intensity; a few non-finite rows, the origin and far points among them (N >= 64)."""
    key = ("cloud", N, F, H, W, conv_name, seed, wrap, transform)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng([seed, N, F, H, W])
    pts = np.concatenate([rng.standard_normal((N, 3)) * (20.0, 20.0, 2.0), rng.uniform(0, 1, (N, 1))], 1).astype(np.float32)
    if N >= 64:
        pts[5, 0] = np.nan; pts[17, 2] = np.inf; pts[23, :3] = 0.0; pts[31, :3] = (70.0, 60.0, 1.0)
    off = ragged_offsets(N, F, rng)
    T = None
    if transform:
        T = np.stack([np.linalg.inv(pose(seed + 10 * f)) for f in range(F)])
        # the points as some other frame sees them: the cloud, moved by the poses, comes back under points2sensor
        fr = np.repeat(np.arange(F), np.diff(off))
        P = np.stack([pose(seed + 10 * f) for f in range(F)])[fr]
        with np.errstate(all="ignore"):
            pts[:, :3] = (np.einsum("nij,nj->ni", P[:, :3, :3], pts[:, :3].astype(np.float64)) + P[:, :3, 3]).astype(np.float32)
    return finish(key, pts, H, W, convention(conv_name, H), offsets=off if F > 1 else None, points2sensor=T, wrap=wrap)


def grid(H, W, conv_name, seed, posed=False, wrap=True):
    """Every ray of this repository's grid times a random range in [1, 71) m: the point of pixel (h, w) is row h W + w."""
    key = ("grid", H, W, conv_name, seed, posed, wrap)
    if key in _CACHE:
        return _CACHE[key]
    conv = convention(conv_name, H)
    rng = np.random.default_rng([seed, H, W])
    s2w = pose(seed) if posed else np.eye(4)
    s2e = None if conv["sensor2ego"] is None else torch.tensor(conv["sensor2ego"])
    inc = conv["inclination"]
    o, d = RangeFrames.range_rays(H, W, inc if len(inc) > 2 else (inc[0], inc[1]), torch.tensor(s2w, dtype=torch.float32), conv["data_type"], s2e)
    r = rng.uniform(1.0, 71.0, (H, W, 1)).astype(np.float32)
    xyz = (o.numpy() + d.numpy() * r).reshape(-1, 3)
    pts = np.concatenate([xyz, rng.uniform(0, 1, (H * W, 1)).astype(np.float32)], 1)
    # the pose as float32 holds it, inverted in float64: what a converter hands over
    T = np.linalg.inv(torch.tensor(s2w, dtype=torch.float32).double().numpy())[None] if posed else None
    return finish(key, pts, H, W, conv, points2sensor=T, wrap=wrap, ranges=r.reshape(-1), sensor2world=s2w)


def one_ray(n, H=8, W=64, equal=False, seed=1):
    """n points on the ray of pixel (3, 20) of the KITTI grid: distinct ranges in shuffled order, or (equal) all at one range."""
    key = ("one_ray", n, H, W, equal, seed)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(seed)
    conv = convention("kitti_bounds", H)
    _, d = RangeFrames.range_rays(H, W, (conv["inclination"][0], conv["inclination"][1]), torch.eye(4), "KITTI", None)
    ray = d[3, 20].numpy().astype(np.float64)
    r = np.full(n, 12.5) if equal else rng.permutation(np.linspace(2.0, 60.0, n))
    if equal:
        pts = np.tile(np.concatenate([(ray * 12.5).astype(np.float32), [0.0]]).astype(np.float32), (n, 1))    # one point, n times: one r32
    else:
        pts = np.concatenate([ray[None, :] * r[:, None], np.zeros((n, 1))], 1).astype(np.float32)
    pts[:, 3] = rng.uniform(0, 1, n).astype(np.float32)
    return finish(key, pts, H, W, conv, ranges=r)


def all_cases_small():
    """The cases the host program is compared on: every convention, both sizes, clouds with and without transforms and wrap, grids, one ray."""
    out = []
    for H, W in SIZES:
        for cn in CONVENTIONS:
            out.append(random_cloud(1000, 3, H, W, cn, 11, wrap=True, transform=False))
            out.append(random_cloud(257, 1, H, W, cn, 12, wrap=False, transform=True))
            out.append(grid(H, W, cn, 13))
            out.append(grid(H, W, cn, 14, posed=True))
    out.append(one_ray(1000)); out.append(one_ray(300, equal=True))
    out += [constructed(m, w) for m in ("bounds", "table") for w in (True, False)]
    return out


def constructed(mode="bounds", wrap=True, H=8, W=64):
    """Points whose fate is known: `expect` holds (drop class, column or None) per row.  KITTI convention, min_depth 1, max_depth 80."""
    key = ("constructed", mode, wrap, H, W)
    if key in _CACHE:
        return _CACHE[key]
    conv = convention("kitti_bounds" if mode == "bounds" else "kitti_table_descending", H)
    inc = np.asarray(conv["inclination"], np.float64)
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))
    at = lambda el, r=10.0: (r * math.cos(el), 0.0, r * math.sin(el))                     # azimuth 0: column W / 2
    rows = [((2.0, 0.0, 0.0), ri.KEEP, W // 2), ((-2.0, 0.0, 0.0), ri.KEEP, 0),
            ((-2.0, -0.0, 0.0), ri.KEEP if wrap else ri.OUT_OF_VIEW, 0 if wrap else None),
            ((np.nan, 1.0, 0.0), ri.INVALID, None), ((1.0, np.inf, 0.0), ri.INVALID, None), ((1.0, 2.0, -np.inf), ri.INVALID, None), ((0.0, 0.0, 0.0), ri.INVALID, None),
            ((80.0, 0.0, 0.0), ri.KEEP, W // 2), ((up(80.0), 0.0, 0.0), ri.OUT_OF_RANGE, None),
            ((1.0, 0.0, 0.0), ri.OUT_OF_RANGE, None), ((up(1.0), 0.0, 0.0), ri.KEEP, W // 2)]
    eps = 1e-3                                                                           # of a pixel, or of a half gap: far above float32's rounding of the coordinates
    if mode == "bounds":
        span = inc[1] - inc[0]
        top, bottom = inc[1] + 0.5 / H * span, inc[0] + 0.5 / H * span                  # v = -0.5 and v = H - 0.5 (off = 0)
        rows += [(at(top + eps / H * span), ri.OUT_OF_VIEW, None), (at(top - eps / H * span), ri.KEEP, W // 2),
                 (at(bottom - eps / H * span), ri.OUT_OF_VIEW, None), (at(bottom + eps / H * span), ri.KEEP, W // 2)]
        edge_rows = {len(rows) - 3: 0, len(rows) - 1: H - 1}
    else:
        s = np.sort(inc)
        lo_gap, hi_gap = 0.5 * (s[1] - s[0]), 0.5 * (s[-1] - s[-2])
        rows += [(at(s[0] - lo_gap * (1 + eps)), ri.OUT_OF_VIEW, None), (at(s[0] - lo_gap * (1 - eps)), ri.KEEP, W // 2),
                 (at(s[-1] + hi_gap * (1 + eps)), ri.OUT_OF_VIEW, None), (at(s[-1] + hi_gap * (1 - eps)), ri.KEEP, W // 2),
                 (at(0.5 * (s[2] + s[3]) + 1e-4 * (s[3] - s[2])), ri.KEEP, W // 2), (at(0.5 * (s[2] + s[3]) - 1e-4 * (s[3] - s[2])), ri.KEEP, W // 2)]
        # descending table: row h has inc[H - 1 - h] = the (h + 1)-th smallest
        edge_rows = {len(rows) - 5: 0, len(rows) - 3: H - 1, len(rows) - 2: 3, len(rows) - 1: 2}
    pts = np.array([list(p) + [0.25 + 0.01 * k] for k, (p, _, _) in enumerate(rows)], np.float32)
    return finish(key, pts, H, W, conv, wrap=wrap, min_depth=1.0, expect=[(c, w) for _, c, w in rows], edge_rows=edge_rows)


def ingest_clouds(seed=5, H=8, W=64):
    """Clouds for the ingest tests, made from synthetic range images: per frame (id, points in the sensor frame, sensor2world) plus what has to
    come back (depth, intensity, mask, the numbers of extra farther returns and of out-of-view points).  Frame 5 is empty."""
    rng = np.random.default_rng(seed)
    inc = list(KITTI_INC)
    _, d = RangeFrames.range_rays(H, W, (inc[0], inc[1]), torch.eye(4), "KITTI", None)
    d = d.numpy().reshape(-1, 3)
    out = []
    for fid in (3, 4, 5, 7):
        s2w = pose(seed + fid)
        if fid == 5:
            out.append(SimpleNamespace(id=fid, points=np.zeros((0, 4), np.float32), sensor2world=s2w, depth=np.zeros((H, W), np.float32),
                                       intensity=np.zeros((H, W), np.float32), mask=np.zeros((H, W), bool), n_extra=0, n_out=0))
            continue
        mask = rng.uniform(size=H * W) < 0.8
        depth = np.where(mask, rng.uniform(2.0, 60.0, H * W), 0.0).astype(np.float32)
        inten = np.where(mask, rng.uniform(0.0, 1.0, H * W), 0.0).astype(np.float32)
        own = np.concatenate([d[mask] * depth[mask, None], inten[mask, None]], 1)
        behind = np.flatnonzero(mask)[rng.uniform(size=int(mask.sum())) < 0.4]             # a second, farther return on the same ray
        extra = np.concatenate([d[behind] * (depth[behind, None] * np.float32(1.3)), rng.uniform(0, 1, (behind.size, 1))], 1)
        n_out = 17
        oov = np.concatenate([rng.uniform(-3, 3, (n_out, 2)), rng.uniform(15, 25, (n_out, 1)), rng.uniform(0, 1, (n_out, 1))], 1)      # far above the top beam
        pts = np.concatenate([own, extra, oov]).astype(np.float32)
        pts = pts[rng.permutation(pts.shape[0])]
        out.append(SimpleNamespace(id=fid, points=pts, sensor2world=s2w, depth=depth.reshape(H, W), intensity=inten.reshape(H, W), mask=mask.reshape(H, W),
                                   n_extra=int(behind.size), n_out=n_out))
    return SimpleNamespace(frames=out, H=H, W=W, inclination=inc)
