"""Shared inputs of the un-projection tests (tests/test_unproject.py on the CPU, tests/test_unproject_gpu.py on the device): every case is built
once per key, with the twin's result, and left unchanged."""
from types import SimpleNamespace

import numpy as np
import torch

from lidar_rt_amd import simulate, sweep, unproject as up
from lidar_rt_amd.training import RangeFrames
from tests import range_image_cases as rc

FAR = (1234.5, -987.25, 12.5)                                                # the sensor's place in the round trips: 1.6 km from the origin
BOUND = 8.0                                                                  # |depth' - depth| <= BOUND * 2^-24 * depth
UNIT = 2.0 ** -24
ROUND_TRIP_SIZES = [(1, 1), (2, 3), (5, 37), (8, 64), (66, 1030)]
GPU_SIZES = [(1, 1), (1, 63), (1, 64), (1, 65), (1, 255), (1, 256), (1, 257), (5, 37), (8, 64), (66, 1030)]
PATTERNS = ("all", "none", "last", "gap", "random")
USES = ("keep", "raydrop", "both")
TRANSFORMS = ("none", "frame", "column")
RATIO = 0.4
# the sensor's motion over one sweep in the round trips under a twist: 0.3 m forward and a turn of 0.3 rad.  The depths start at 1 m, where a
# translation rho shows as a parallax of |rho| / 1 m between the first and the last column; the turn opens a gap of 0.3 rad at the seam, which
# that parallax does not exceed, so no point is seen by two columns a sweep apart (tests/sweep_project_cases.py, grid())
TWIST = (0.3, 0.04, 0.0, 0.0, 0.0, 0.3)

_CACHE = {}


def far_pose(seed=3):
    """(4, 4) float32-representable: the rotation of range_image_cases.pose and the translation FAR."""
    M = rc.pose(seed)
    M[:3, 3] = FAR
    return M.astype(np.float32).astype(np.float64)


def conventions(H):
    """Both conventions with bounds, and a beam table where the image has the three rows one needs."""
    return ("kitti_bounds", "waymo_bounds_yaw") + (("waymo_table_yaw",) if H >= 3 else ())


def static_grid(H, W, conv_name, seed=5):
    """The ray grid of RangeFrames.range_rays at the far pose (float32, as the loops hold it) and depths in [1, 80] m."""
    key = ("static", H, W, conv_name, seed)
    if key not in _CACHE:
        conv = rc.convention(conv_name, H)
        P = far_pose()
        s2e = None if conv["sensor2ego"] is None else torch.tensor(conv["sensor2ego"])
        inc = conv["inclination"]
        o, d = RangeFrames.range_rays(H, W, inc if len(inc) > 2 else (inc[0], inc[1]), torch.tensor(P, dtype=torch.float32), conv["data_type"], s2e)
        r = torch.tensor(np.random.default_rng([seed, H, W]).uniform(1.0, 80.0, (H, W)).astype(np.float32))
        _CACHE[key] = SimpleNamespace(H=H, W=W, conv=conv, pose=P, o=o, d=d, depth=r)
    return _CACHE[key]


def sweep_grid(H, W, conv_name, seed=5):
    """The grid of the sweep-ray twin at the far pose under TWIST, rounded to float32 as the operator's rays are, and depths in [1, 80] m."""
    key = ("sweep", H, W, conv_name, seed)
    if key not in _CACHE:
        conv = rc.convention(conv_name, H)
        P = far_pose()
        xi = np.asarray(TWIST, np.float32).astype(np.float64)
        tau = sweep.column_times(W).to(torch.float32).to(torch.float64)
        s2e = None if conv["sensor2ego"] is None else torch.tensor(conv["sensor2ego"])
        o, d = sweep.sweep_rays_reference(torch.tensor(P), torch.tensor(xi), H, W, conv["inclination"], conv["data_type"], s2e, tau=tau)
        r = torch.tensor(np.random.default_rng([seed, H, W, 1]).uniform(1.0, 80.0, (H, W)).astype(np.float32))
        _CACHE[key] = SimpleNamespace(H=H, W=W, conv=conv, pose=P, twist=xi, tau=tau.numpy(), o=o.to(torch.float32).contiguous(), d=d.to(torch.float32).contiguous(), depth=r)
    return _CACHE[key]


def keep_pattern(name, F, H, W, rng):
    """(F, H, W) bool.  "gap": a whole workgroup of 256 pixels dropped between two kept ones (all kept where the frame has no third workgroup);
    "last": only the last pixel of each frame."""
    hw = H * W
    k = np.zeros((F, hw), bool)
    if name == "all":
        k[:] = True
    elif name == "last":
        k[:, -1] = True
    elif name == "gap":
        k[:] = True
        k[:, up.BLOCK:2 * up.BLOCK] = False
    elif name == "random":
        k[:] = rng.random((F, hw)) < 0.5
    elif name != "none":
        raise KeyError(name)
    return k.reshape(F, H, W)


def transforms(kind, F, W, seed):
    """world2out: None, (F, 3, 4) or (F, W, 4, 4) float64 rigid transforms."""
    if kind == "none":
        return None
    if kind == "frame":
        return np.stack([np.linalg.inv(rc.pose(seed + f))[:3] for f in range(F)])
    rng = np.random.default_rng([seed, F, W])
    out = np.stack([np.broadcast_to(np.linalg.inv(rc.pose(seed + f)), (W, 4, 4)) for f in range(F)]).copy()
    out[:, :, :3, 3] += rng.uniform(-0.5, 0.5, (F, W, 3))                    # every column its own shift behind the frame's transform
    return out


def random_frames(F, H, W, pattern="random", use="both", transform="none", seed=11, empty_middle=True, cache=True):
    """F frames of random rays (origins within 30 m, unit directions to float32) and depths in (0, 90) m with a few specials: NaN and infinite depths,
    a NaN origin, an infinite direction, depth 0 and depths beyond max_depth 80 and below min_depth 0.5.  `pattern` chooses the pixels that survive
    the mask (through keep, raydrop or both); with F == 3 the middle frame keeps nothing.  ``cache=False``: a large case is built for its one test
    and not kept."""
    key = ("random", F, H, W, pattern, use, transform, seed, empty_middle)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng([seed, F, H, W])
    hw = H * W
    depth = rng.uniform(0.6, 79.0, (F, H, W)).astype(np.float32)
    o = np.broadcast_to(rng.uniform(-30, 30, (F, 1, 1, 3)), (F, H, W, 3)).astype(np.float32).copy()
    d = rng.standard_normal((F, H, W, 3))
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    inten = rng.uniform(0, 1, (F, H, W)).astype(np.float32)
    if hw >= 37:                                                             # the specials, on the pixels the patterns other than "none" / "last" keep
        flat = depth.reshape(F, hw)
        flat[:, 3], flat[:, 5], flat[:, 7], flat[:, 11], flat[:, 13], flat[:, 17] = np.nan, np.inf, 0.0, 85.0, 0.25, -1.0
        o.reshape(F, hw, 3)[:, 19, 1] = np.nan
        d.reshape(F, hw, 3)[:, 23, 2] = np.inf
    want = keep_pattern(pattern, F, H, W, rng)
    if F == 3 and empty_middle:
        want[1] = False
    keep = drop = None
    if use == "keep":
        keep = want
    elif use == "raydrop":
        drop = np.where(want, rng.uniform(0.0, 0.39, want.shape), rng.uniform(0.4, 1.0, want.shape)).astype(np.float32)
    else:                                                                    # both: each pixel that goes is taken out by one of the two, or by both
        third = rng.integers(0, 3, want.shape)
        keep = want | (third == 0)
        drop = np.where(want | (third == 1), rng.uniform(0.0, 0.39, want.shape), rng.uniform(0.4, 1.0, want.shape)).astype(np.float32)
    T = transforms(transform, F, W, seed)
    kw = dict(intensity=inten, keep=keep, raydrop=drop, raydrop_ratio=RATIO, world2out=T, min_depth=0.5, max_depth=80.0)
    for a in (depth, o, d, inten, keep, drop):
        if a is not None:
            a.setflags(write=False)
    twin = up.points_from_range_images_reference(depth, o, d, **kw)
    c = SimpleNamespace(key=key, F=F, H=H, W=W, depth=depth, o=o, d=d, kw=kw, twin=twin, want=want)
    if cache:
        _CACHE[key] = c
    return c


def small_cases():
    """What the host program is compared on: every pattern, use and transform at 5 x 37 and 8 x 64 with three frames, and the smallest images."""
    out = [random_frames(3, H, W, p, u, t) for H, W in ((5, 37), (8, 64)) for p in PATTERNS for u in USES for t in TRANSFORMS]
    out += [random_frames(F, H, W, "random", "both", t) for F in (1, 3) for H, W in ((1, 1), (2, 3), (1, 257)) for t in TRANSFORMS]
    return out


def round_trip_error(depth_back, depth):
    """max |depth' - depth| / (2^-24 depth), both float32 tensors, in float64."""
    a, b = depth_back.double().reshape(-1), depth.double().reshape(-1)
    return float(((a - b).abs() / (UNIT * b)).max())


def sensor_table(g, frame):
    return simulate.column_transforms(frame, g.pose, getattr(g, "twist", None), getattr(g, "tau", None), origins=g.o[0] if hasattr(g, "twist") else None)
