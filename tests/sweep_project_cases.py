"""Seeded cases of the range-image projection under the sweep model, shared by tests/test_sweep_project.py and tests/test_sweep_project_gpu.py.

A case is the arguments of ``project_points_sweep`` (numpy points) and the twin's result, computed once on the CPU and left unchanged.  Every
builder asserts ``twin.margin >= MARGIN`` and ``twin.range_margin >= RANGE_MARGIN``: every evaluated column coordinate and the row coordinate
stay off their rounding boundaries, and every kept range off a float32 rounding boundary -- the conditions under which two evaluations of the
rule that differ in the last float64 bits (a fused multiply-add in Exp, another sincos or atan2) agree on every pixel, class and depth bit.
They are conditions on the inputs, not filters: no point is ever left out of a comparison; a seeded case that misses one gets another seed.
Measured on the cases below: margin 9.8e-7 .. 4.6e-4 on the clouds of at most 1000 points (70 000 points: 3.2e-8 .. 1.1e-6), 1.5e-4 .. 4e-2 on
the ray grids; range_margin 1.2e-12 .. 4e-10 on the clouds of at most 1000 points, 2.7e-13 .. 9.6e-13 on those of 70 000 (a seed in four
misses 1e-13 at that size and is replaced: CLOUD_SEEDS), 3e-12 .. 5e-10 on the grids."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from lidar_rt_amd import sweep, sweep_project as sp
from tests import range_image_cases as rc

MARGIN = 1e-9
RANGE_MARGIN = 1e-13
ZERO = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
MODERATE = (1.5, 0.2, 0.0, 0.0, 0.0, 0.05)
STRONG = (3.0, 0.0, 0.0, 0.0, 0.0, 0.3)                                       # adjacent 2-cycles, up to 8 evaluations
CLOSED = (0.0, 0.0, 0.0, 0.0, 0.0, 1.2)                                       # |tau phi|^2 >= 0.25 at the ends of the sweep: sw_coef's closed forms
PER_FRAME = ((1.5, 0.2, 0.0, 0.0, 0.0, 0.05), (-0.8, 0.4, 0.1, 0.01, -0.02, -0.08), (2.2, -0.3, 0.05, -0.01, 0.015, 0.12))
INGEST_TWISTS = ((1.5, 0.2, 0.0, 0.0, 0.0, 0.05), (0.8, -0.4, 0.1, 0.01, -0.02, 0.08), (2.2, -0.3, 0.05, -0.01, 0.015, 0.12))     # "cw": they turn with the column order
SIZES = rc.SIZES
GRID_SEED = 21                                                                # of the ray grids: see grid()
CLOUD_SEEDS = {(70_000, 1): 12}                                               # (N, F) of the 8 x 64 clouds whose seed 11 misses RANGE_MARGIN
CONVENTIONS = rc.CONVENTIONS


def tau_table(W, seed=7):
    """The explicit column times: the default ones plus a seeded jitter of 0.2 / W."""
    rng = np.random.default_rng([seed, W])
    return sweep.column_times(W).numpy() + rng.uniform(-0.2, 0.2, W) / W


def motion(name, W, F=1):
    """-> dict(twist, tau, t_ref, direction): the twist (per frame for F == 3) and the column times of a named motion."""
    per = lambda one: np.array(PER_FRAME if F == 3 else one, np.float64)
    if name == "zero":
        return dict(twist=np.array(ZERO), tau=None, t_ref=0.5, direction="cw")
    if name == "moderate_cw":
        return dict(twist=per(MODERATE), tau=None, t_ref=0.5, direction="cw")
    if name == "moderate_ccw":
        return dict(twist=per(MODERATE), tau=None, t_ref=0.0, direction="ccw")
    if name == "strong_cw":
        return dict(twist=np.array(STRONG), tau=None, t_ref=0.5, direction="cw")
    if name == "strong_ccw":
        return dict(twist=np.array(STRONG) * (np.array([1.0, 0.8, -0.6])[:, None] if F == 3 else 1.0), tau=None, t_ref=0.0, direction="ccw")
    if name == "minus_strong_ccw":
        return dict(twist=-np.array(STRONG), tau=None, t_ref=0.5, direction="ccw")
    if name == "minus_strong_cw":
        return dict(twist=-np.array(STRONG), tau=None, t_ref=0.5, direction="cw")
    if name == "table":
        return dict(twist=per(MODERATE), tau=tau_table(W), t_ref=0.5, direction="cw")
    if name == "closed":
        return dict(twist=np.array(CLOSED), tau=None, t_ref=0.5, direction="cw")
    raise KeyError(name)


def column_times(mo, W):
    """The (W,) float64 column times a motion stands for."""
    return np.asarray(mo["tau"], np.float64) if mo["tau"] is not None else sweep.column_times(W, mo["t_ref"], mo["direction"]).numpy()


_CACHE = {}


def finish(key, points, H, W, conv, mo, offsets=None, points2sensor=None, max_depth=80.0, min_depth=0.0, wrap=True, **extra):
    """The case with its twin, computed once per key and left unchanged."""
    if key in _CACHE:
        return _CACHE[key]
    points = np.ascontiguousarray(points, np.float32)
    points.setflags(write=False)
    kw = dict(H=H, W=W, inclination=conv["inclination"], twist=mo["twist"], offsets=None if offsets is None else np.asarray(offsets, np.int64),
              data_type=conv["data_type"], sensor2ego=conv["sensor2ego"], points2sensor=points2sensor, tau=mo["tau"], t_ref=mo["t_ref"], direction=mo["direction"],
              max_depth=max_depth, min_depth=min_depth, wrap=wrap)
    twin = sp.project_points_sweep_reference(points, **kw)
    assert twin.margin >= MARGIN, (key, twin.margin)
    assert twin.range_margin >= RANGE_MARGIN, (key, twin.range_margin)
    c = SimpleNamespace(key=key, points=points, kw=kw, twin=twin, **extra)
    _CACHE[key] = c
    return c


def static_kw(kw):
    """The arguments of range_image.project_points in those of a case."""
    return {k: v for k, v in kw.items() if k not in ("twist", "tau", "t_ref", "direction")}


def random_cloud(N, F, H, W, conv_name, seed, mo_name="moderate_cw", wrap=True, transform=False):
    """The cloud of range_image_cases.random_cloud (randn * (20, 20, 2) m, non-finite rows, the origin and a far point among them) under a motion."""
    key = ("cloud", N, F, H, W, conv_name, seed, mo_name, wrap, transform)
    if key in _CACHE:
        return _CACHE[key]
    base = rc.random_cloud(N, F, H, W, conv_name, seed, wrap=wrap, transform=transform)
    return finish(key, base.points, H, W, rc.convention(conv_name, H), motion(mo_name, W, F), offsets=base.kw["offsets"], points2sensor=base.kw["points2sensor"], wrap=wrap)


def sweep_rays64(H, W, conv, mo, s2w=None):
    """(o, d) (H, W, 3) float64 numpy of sweep_rays_reference for one frame of a motion (its first twist)."""
    P = torch.tensor(np.eye(4) if s2w is None else s2w, dtype=torch.float64)
    xi = torch.tensor(np.asarray(mo["twist"], np.float64).reshape(-1, 6)[0])
    s2e = None if conv["sensor2ego"] is None else torch.tensor(conv["sensor2ego"])
    o, d = sweep.sweep_rays_reference(P, xi, H, W, conv["inclination"], conv["data_type"], s2e, tau=torch.tensor(column_times(mo, W)))
    return o.numpy(), d.numpy()


def grid(H, W, conv_name, seed, mo_name, posed=False, own_pixel=True):
    """Every ray of the sweep grid times a random range in [2, 62) m: the point of pixel (h, w) is row h W + w.  ``own_pixel``: the builder
    asserts that the twin alone brings every point back to its own pixel.  The motions whose seam has a gap allow it; what a translating
    sensor adds is parallax, which for a NEAR point next to the seam can exceed the gap, so that two columns a sweep apart both see the point and
    the search from the static column reaches the other one.  GRID_SEED is a seed whose ranges put no such point on the grids used here.  In
    the other direction the seam overlaps for every range (own_pixel=False)."""
    key = ("grid", H, W, conv_name, seed, mo_name, posed)
    if key in _CACHE:
        return _CACHE[key]
    conv, mo = rc.convention(conv_name, H), motion(mo_name, W)
    rng = np.random.default_rng([seed, H, W])
    s2w = rc.pose(seed) if posed else None
    o, d = sweep_rays64(H, W, conv, mo, s2w)
    r = rng.uniform(2.0, 62.0, (H, W, 1))
    pts = np.concatenate([(o + d * r).reshape(-1, 3), rng.uniform(0, 1, (H * W, 1))], 1).astype(np.float32)
    T = np.linalg.inv(s2w)[None] if posed else None
    c = finish(key, pts, H, W, conv, mo, points2sensor=T, ranges=r.reshape(-1), origins=o, directions=d)
    if own_pixel:
        assert torch.equal(c.twin.index.reshape(-1), torch.arange(H * W, dtype=torch.int32)), key
    return c


def one_ray(n, H=8, W=64, equal=False, seed=1, mo_name="moderate_cw"):
    """n points on the sweep ray of pixel (3, 20): distinct ranges in shuffled order, or (equal) one point n times."""
    key = ("one_ray", n, H, W, equal, seed, mo_name)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(seed)
    conv, mo = rc.convention("kitti_bounds", H), motion(mo_name, W)
    o, d = sweep_rays64(H, W, conv, mo)
    r = np.full(n, 12.5) if equal else rng.permutation(np.linspace(2.0, 60.0, n))
    xyz = (o[3, 20][None, :] + d[3, 20][None, :] * r[:, None]).astype(np.float32)
    if equal:
        xyz = np.tile(xyz[:1], (n, 1))
    pts = np.concatenate([xyz, rng.uniform(0, 1, (n, 1)).astype(np.float32)], 1)
    return finish(key, pts, H, W, conv, mo, ranges=r)


def between_columns(H=8, W=64, pairs=(10, 41), r=30.0):
    """Constructed points that no column sees: STRONG turning against the column order ("ccw") opens a gap between the bins of every adjacent
    pair of columns, taken at their own instants.  Point k lies in the middle of the gap between columns pairs[k] and pairs[k] + 1, on row 3's
    elevation: each of the two columns sees it in the other's bin.  A third point is an ordinary seen one."""
    key = ("between", H, W, pairs, r)
    if key in _CACHE:
        return _CACHE[key]
    conv, mo = rc.convention("kitti_bounds", H), motion("strong_ccw", W)
    tau = column_times(mo, W)
    R, t = sweep.column_poses_reference(torch.eye(4, dtype=torch.float64)[None, :3], torch.tensor(mo["twist"])[None], torch.tensor(tau))
    R, t = R[0].numpy(), t[0].numpy()
    inc = conv["inclination"]
    el = inc[0] + (H - 3) / H * (inc[1] - inc[0])
    rows = []
    for w in pairs:
        az = math.pi - (w + 0.5) * 2.0 * math.pi / W                        # u = w + 0.5: the edge the two bins share in their own frames
        l = np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
        rows.append(0.5 * ((t[w] + R[w] @ l * r) + (t[w + 1] + R[w + 1] @ l * r)))
    o, d = sweep_rays64(H, W, conv, mo)
    rows.append(o[3, 20] + d[3, 20] * r)
    pts = np.concatenate([np.array(rows), np.full((len(rows), 1), 0.5)], 1).astype(np.float32)
    c = finish(key, pts, H, W, conv, mo, pairs=pairs)
    assert c.twin.drop.tolist() == [sp.UNSEEN] * len(pairs) + [sp.KEEP] and c.twin.evals.tolist()[:len(pairs)] == [sp.MAX_EVAL] * len(pairs), key
    return c


def beyond_the_edge(H=8, W=64):
    """wrap=False: a point next to azimuth -pi, beyond the last column's bin (u = W - 0.25), and an ordinary one."""
    key = ("edge", H, W)
    if key in _CACHE:
        return _CACHE[key]
    a = -math.pi + 0.25 * 2.0 * math.pi / W
    pts = np.array([[20.0 * math.cos(a), 20.0 * math.sin(a), -2.0, 0.5], [20.0, 1.0, -2.0, 0.25]], np.float32)
    c = finish(key, pts, H, W, rc.convention("kitti_bounds", H), motion("moderate_cw", W), wrap=False)
    assert c.twin.drop.tolist() == [sp.OUT_OF_VIEW, sp.KEEP] and int(c.twin.counts[4]) == 0, key
    return c


def all_cases_small():
    """The cases the host program is compared on: clouds in every convention and motion at both sizes, grids, one ray, the constructed points,
    and the sizes 1 x 1 and 2 x 3."""
    out = []
    for H, W in SIZES:
        for cn in CONVENTIONS:
            out.append(random_cloud(1000, 3, H, W, cn, 11, "moderate_cw"))
            out.append(random_cloud(257, 1, H, W, cn, 12, "strong_ccw", wrap=False, transform=True))
            out.append(random_cloud(1000, 3, H, W, cn, 11, "table", transform=True))
            out.append(grid(H, W, cn, GRID_SEED, "moderate_cw"))
            out.append(grid(H, W, cn, GRID_SEED, "moderate_ccw", posed=True))
        out.append(random_cloud(1000, 1, H, W, "kitti_bounds", 11, "closed"))
        out.append(random_cloud(1000, 1, H, W, "kitti_bounds", 11, "strong_cw"))
        out.append(random_cloud(1000, 1, H, W, "kitti_bounds", 11, "zero"))
    for H, W in ((1, 1), (2, 3)):
        for wrap in (True, False):
            out.append(random_cloud(257, 1, H, W, "kitti_bounds", 12, "strong_ccw", wrap=wrap))
    out += [one_ray(1000), one_ray(300, equal=True), between_columns(), beyond_the_edge()]
    return out


def ingest_clouds(seed=5, H=8, W=64, direction="cw", t_ref=0.5):
    """Compensated clouds for the ingest tests, made from synthetic range images of a SWEEPING sensor: per frame (id, points in the sensor frame of
    the reference instant, sensor2world, twist) plus what has to come back (depth, intensity, mask, the number of extra farther returns and of
    points above the view).  A pixel's point is o[h, w] + d[h, w] depth on the sweep grid of the frame's twist, a second return lies 1.3 times as
    far along the same ray.  Frame 5 is empty.  The twists turn with the column order (negated for "ccw"), so that the seam has a gap and every
    pixel's own point is the only one its column sees; the builder asserts that the twin alone returns the masks."""
    rng = np.random.default_rng([seed, direction == "cw"])
    inc = list(rc.KITTI_INC)
    conv = rc.convention("kitti_bounds", H)
    out = []
    for k, fid in enumerate((3, 4, 5, 7)):
        s2w = rc.pose(seed + fid)
        twist = np.array(INGEST_TWISTS[k % 3], np.float64) * (1.0 if k < 3 else 0.5) * (1.0 if direction == "cw" else -1.0)
        if fid == 5:
            out.append(SimpleNamespace(id=fid, points=np.zeros((0, 4), np.float32), sensor2world=s2w, twist=twist, depth=np.zeros((H, W), np.float32),
                                       intensity=np.zeros((H, W), np.float32), mask=np.zeros((H, W), bool), n_extra=0, n_out=0))
            continue
        o, d = sweep_rays64(H, W, conv, dict(twist=twist, tau=None, t_ref=t_ref, direction=direction))
        o, d = o.reshape(-1, 3), d.reshape(-1, 3)
        mask = rng.uniform(size=H * W) < 0.8
        depth = np.where(mask, rng.uniform(2.0, 60.0, H * W), 0.0).astype(np.float32)
        inten = np.where(mask, rng.uniform(0.0, 1.0, H * W), 0.0).astype(np.float32)
        own = np.concatenate([o[mask] + d[mask] * depth[mask, None].astype(np.float64), inten[mask, None]], 1)
        behind = np.flatnonzero(mask)[rng.uniform(size=int(mask.sum())) < 0.4]             # a second, farther return on the same ray
        extra = np.concatenate([o[behind] + d[behind] * (depth[behind, None].astype(np.float64) * 1.3), rng.uniform(0, 1, (behind.size, 1))], 1)
        n_out = 17
        oov = np.concatenate([rng.uniform(-3, 3, (n_out, 2)), rng.uniform(15, 25, (n_out, 1)), rng.uniform(0, 1, (n_out, 1))], 1)      # far above the top beam
        pts = np.concatenate([own, extra, oov]).astype(np.float32)
        pts = pts[rng.permutation(pts.shape[0])]
        twin = sp.project_points_sweep_reference(pts, H, W, inc, twist, t_ref=t_ref, direction=direction)
        assert twin.margin >= MARGIN and twin.range_margin >= RANGE_MARGIN, (fid, twin.margin, twin.range_margin)
        assert np.array_equal(twin.mask.numpy().reshape(-1), mask), fid
        out.append(SimpleNamespace(id=fid, points=pts, sensor2world=s2w, twist=twist, depth=depth.reshape(H, W), intensity=inten.reshape(H, W), mask=mask.reshape(H, W),
                                   n_extra=int(behind.size), n_out=n_out, twin=twin))
    return SimpleNamespace(frames=out, H=H, W=W, inclination=inc, direction=direction, t_ref=t_ref)
