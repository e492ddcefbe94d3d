"""Place recognition through ``csrc/liblrt_place.so``: which earlier scan does a scan revisit, and at which yaw -- the hot path under
``pose_graph.close_loops``, which turns the odometry chain of ``registration.odometry`` into a pose graph with loop edges.

    desc, sums     = describe(points, mask, z_lo, rings=20, sectors=60, r_min=2.0, r_max=80.0, z_step=0.025, up=(0, 0, 1))
    best_d, best_s = match(desc, gap=20)                                  # (F, F) int32 each, -1 outside j + gap <= i
    sc             = score(best_d, sums)                                  # (F, F) float64 in [0, 1]; NaN outside the triangle
    pairs          = candidates(best_d, best_s, sums, top=2, max_score=DEFAULT_MAX_SCORE)      # [(i, j, score, s)]
    X0             = shift_to_init(s, sectors, up=(0, 0, 1))              # (3, 4) float64: the init of registration.align, source i onto target j

``points (F, H, W, 3)`` float32 are sensor-frame points with their ``mask (F, H, W)`` (``registration.frame_geometry`` or
``segmentation.frame_points``).  ``include/lrt_place.h`` states every rule and ``csrc/lrt_place_math.h`` is its text for the device and the host.
EVERY RESULT IS AN INTEGER that does not depend on the order in which lanes arrive, so the numpy twins (``*_reference``) are exact: the tests are
equalities.

* The descriptor: ``rings x sectors`` cells, one byte each, ``desc (F, sectors, rings rounded up to a multiple of 4)`` uint8, sector-major.  A kept
  pixel (``r_min <= rho < r_max`` on the ground plane and ``h >= z_lo`` along ``up``) raises its cell to ``min(255, 1 + floor((h - z_lo) / z_step))``;
  the ring is ``floor((rho - r_min) rings / (r_max - r_min))`` and the SECTOR IS THE PIXEL'S OWN COLUMN, ``(w sectors) // W``: the image is the
  index, no ``atan2`` is taken, and a yaw of the sensor is a circular shift of the sectors.  ``sums (F)`` int32 is the sum of a descriptor's bytes.
  ``z_lo`` is an argument (minus the sensor's height above the ground, as in ``segmentation``); nothing is guessed from the data.
* ``match``: ``D(i, j, s) = sum |a_i[r, (c + s) mod sectors] - a_j[r, c]|``, ``best_d`` its minimum over ``s`` and ``best_s`` the lowest ``s`` that
  attains it, for every ``j + gap <= i``.
* ``score = best_d / (sum_i + sum_j)`` lies in [0, 1] because ``|a - b| <= a + b``: 0 is identical, 1 is disjoint, and 0 / 0 is defined as 1.
* HIP tensors go through the library (``describe`` and ``match`` are one launch each, whatever the images hold; no host wait, no allocation inside
  the call, stream-ordered).  A missing library is a ``PlaceError``, not a quiet fall-back.  CPU tensors go to the twins, which run anywhere.
  ``score``, ``candidates`` and ``shift_to_init`` are host code, shared by both paths.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LRT_PLACE_LIB") or os.path.join(HERE, "csrc", "liblrt_place.so")
EXPORTS = ("lrt_place_abi_version", "lrt_place_last_error", "lrt_place_describe", "lrt_place_match")     # include/lrt_place.h
ABI_VERSION = 1
BLOCK = 256                                                                  # LRT_PLACE_BLOCK
DESCRIBE_BLOCK = 512                                                         # LRT_PLACE_DESCRIBE_BLOCK
TILE = 16                                                                    # LRT_PLACE_TILE
MAX_RINGS, MAX_SECTORS, MAX_FRAMES = 32, 128, 32768
MAX_PIXELS = (2 ** 31 - 1) // 3                                              # LRT_PLACE_MAX_PIXELS
DEFAULT_RINGS, DEFAULT_SECTORS = 20, 60
DEFAULT_R_MIN, DEFAULT_R_MAX, DEFAULT_Z_STEP = 2.0, 80.0, 0.025
DEFAULT_GAP, DEFAULT_TOP = 20, 2
# Halfway between the true revisit (0.208) and the best pair that is none (0.354) as the twin saw them on the room tour of tests/place_cases.py:
# the table is in profiles/place.md.  Scenes of tools/make_sequence.py and real scans were not measured.
DEFAULT_MAX_SCORE = 0.28

_lib = None


class PlaceError(RuntimeError):
    pass


def load():
    """Load liblrt_place.so (after torch, so that both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PlaceError(f"{LIB_PATH} is missing: build it with `python -m lidar_rt_amd.build` (hipcc --offload-arch=gfx950). "
                         "place has no fall-back on a HIP device.")
    lib = C.CDLL(LIB_PATH)
    vp, ci, ll, d = C.c_void_p, C.c_int, C.c_longlong, C.c_double
    lib.lrt_place_abi_version.restype = ci
    lib.lrt_place_last_error.restype = C.c_char_p
    lib.lrt_place_describe.restype = ci
    lib.lrt_place_describe.argtypes = [ci, ll, ci, ci, vp, vp, ci, ci, d, d, d, d, d, d, d, vp, vp, vp]
    lib.lrt_place_match.restype = ci
    lib.lrt_place_match.argtypes = [ci, ll, ci, ci, vp, ll, vp, vp, vp]
    if lib.lrt_place_abi_version() != ABI_VERSION:
        raise PlaceError("liblrt_place.so ABI version mismatch; rebuild with `python -m lidar_rt_amd.build --force`")
    _lib = lib
    return lib


# ---- the arguments ------------------------------------------------------------------------------------------------------------------------------------------

def padded(rings: int) -> int:
    """The bytes of one sector: ``rings`` rounded up to a multiple of 4 (pl_padded)."""
    return (int(rings) + 3) // 4 * 4


def _frames(points, mask):
    if not torch.is_tensor(points) or points.dim() not in (3, 4) or points.shape[-1] != 3 or points.dtype != torch.float32:
        raise PlaceError("describe: points must be a float32 (H, W, 3) or (F, H, W, 3) tensor")
    batched = points.dim() == 4
    points = points.detach().contiguous()
    points = points if batched else points[None]
    F, H, W = (int(x) for x in points.shape[:3])
    if F < 1 or F > MAX_FRAMES or H < 1 or W < 1 or F * H * W > MAX_PIXELS:
        raise PlaceError(f"describe: {F} frames of {H} x {W} pixels (each at least 1, at most {MAX_FRAMES} frames, F H W at most {MAX_PIXELS})")
    shape = (F, H, W) if batched else (H, W)
    if not torch.is_tensor(mask) or tuple(mask.shape) != shape or mask.device != points.device:
        raise PlaceError(f"describe: mask must be a {shape} tensor on {points.device}")
    mask = mask.detach()
    if mask.dtype == torch.bool:
        mask = mask.contiguous().view(torch.uint8)                             # a bool is a byte of 0 or 1: no kernel
    else:
        mask = mask.contiguous() if mask.dtype == torch.uint8 else (mask != 0).view(torch.uint8)
    return points, (mask if batched else mask[None]), batched, F, H, W


def _rule(z_lo, rings, sectors, r_min, r_max, z_step, up, W):
    rings, sectors = int(rings), int(sectors)
    if rings < 1 or rings > MAX_RINGS or sectors < 1 or sectors > MAX_SECTORS:
        raise PlaceError(f"describe: a descriptor of {rings} rings x {sectors} sectors (1 to {MAX_RINGS} rings, 1 to {MAX_SECTORS} sectors)")
    if sectors > W:
        raise PlaceError(f"describe: {sectors} sectors over {W} columns (a sector is at least one column)")
    if z_lo is None:
        raise PlaceError("describe: z_lo is required (minus the height of the sensor above the ground, metres): nothing is guessed from the data")
    up = np.asarray(up, np.float64).reshape(-1)
    if up.size != 3 or not abs(float(up @ up) - 1.0) < 1e-6:
        raise PlaceError(f"describe: up {up.tolist()} is not a unit vector")
    r_min, r_max, z_lo, z_step = float(r_min), float(r_max), float(z_lo), float(z_step)
    if not (0.0 <= r_min < r_max and math.isfinite(r_max)):
        raise PlaceError(f"describe: the ground range [{r_min}, {r_max}) (0 <= r_min < r_max)")
    if not math.isfinite(z_lo):
        raise PlaceError(f"describe: z_lo {z_lo}")
    if not (z_step > 0.0 and math.isfinite(z_step)):
        raise PlaceError(f"describe: z_step {z_step} (positive)")
    return rings, sectors, r_min, r_max, z_lo, z_step, up


def _descriptors(desc):
    if not torch.is_tensor(desc) or desc.dim() != 3 or desc.dtype != torch.uint8:
        raise PlaceError("match: desc must be the (F, sectors, padded rings) uint8 tensor of describe")
    F, NS, NRP = (int(x) for x in desc.shape)
    if F < 1 or F > MAX_FRAMES:
        raise PlaceError(f"match: {F} frames (1 to {MAX_FRAMES})")
    if NS < 1 or NS > MAX_SECTORS or NRP < 4 or NRP > MAX_RINGS or NRP % 4:
        raise PlaceError(f"match: descriptors of {NS} sectors x {NRP} bytes (1 to {MAX_SECTORS} sectors; 4 to {MAX_RINGS} bytes, a multiple of 4)")
    return desc.detach().contiguous(), F, NS, NRP


def _gap(gap):
    gap = int(gap)
    if gap < 0:
        raise PlaceError(f"match: a gap of {gap} frames (not negative)")
    return gap


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


# ---- 1. the descriptors -------------------------------------------------------------------------------------------------------------------------------------

@torch.no_grad()
def describe_reference(points, mask, z_lo=None, rings=DEFAULT_RINGS, sectors=DEFAULT_SECTORS, r_min=DEFAULT_R_MIN, r_max=DEFAULT_R_MAX,
                       z_step=DEFAULT_Z_STEP, up=(0.0, 0.0, 1.0)):
    """The numpy twin of ``describe``: (desc uint8, sums int32) as CPU tensors."""
    pts, m, batched, F, H, W = _frames(points, mask)
    NR, NS, r_min, r_max, z_lo, z_step, up = _rule(z_lo, rings, sectors, r_min, r_max, z_step, up, W)
    p = pts.cpu().numpy().astype(np.float64)
    valid = m.cpu().numpy() != 0
    with np.errstate(all="ignore"):
        x, y, z = p[..., 0], p[..., 1], p[..., 2]
        h = up[0] * x + up[1] * y + up[2] * z
        gx, gy, gz = x - h * up[0], y - h * up[1], z - h * up[2]
        rho = np.sqrt(gx * gx + gy * gy + gz * gz)
        kept = valid & (rho >= r_min) & (rho < r_max) & (h >= z_lo)
        fr = np.floor((rho - r_min) * float(NR) / (r_max - r_min))
        fv = np.floor((h - z_lo) / z_step)
    ring = np.where(kept, np.where(fr >= NR - 1, NR - 1, fr), 0).astype(np.int64)
    value = np.where(kept, np.where(fv >= 254.0, 255, 1 + np.where(kept, fv, 0)), 0).astype(np.int64)
    sector = np.broadcast_to((np.arange(W, dtype=np.int64) * NS) // W, (F, H, W))
    frame = np.broadcast_to(np.arange(F, dtype=np.int64)[:, None, None], (F, H, W))
    desc = np.zeros((F, NS, padded(NR)), np.int64)
    np.maximum.at(desc, (frame[kept], sector[kept], ring[kept]), value[kept])
    sums = desc.sum((1, 2)).astype(np.int32)
    desc, sums = torch.from_numpy(desc.astype(np.uint8)), torch.from_numpy(sums)
    return (desc, sums) if batched else (desc[0], sums[0])


@torch.no_grad()
def describe(points, mask, z_lo=None, rings=DEFAULT_RINGS, sectors=DEFAULT_SECTORS, r_min=DEFAULT_R_MIN, r_max=DEFAULT_R_MAX, z_step=DEFAULT_Z_STEP,
             up=(0.0, 0.0, 1.0)):
    """(desc (F, sectors, padded(rings)) uint8, sums (F) int32) of F frames (see the module text); without a frame axis in, without one out."""
    pts, m, batched, F, H, W = _frames(points, mask)
    dev = pts.device
    if dev.type != "cuda":
        return describe_reference(points, mask, z_lo, rings, sectors, r_min, r_max, z_step, up)
    NR, NS, r_min, r_max, z_lo, z_step, up = _rule(z_lo, rings, sectors, r_min, r_max, z_step, up, W)
    lib = load()
    desc = torch.empty((F, NS, padded(NR)), dtype=torch.uint8, device=dev)
    sums = torch.empty((F,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.lrt_place_describe(dev.index, F, H, W, pts.data_ptr(), m.data_ptr(), NR, NS, float(up[0]), float(up[1]), float(up[2]), r_min, r_max,
                                    z_lo, z_step, desc.data_ptr(), sums.data_ptr(), _stream(dev))
    if rc != 0:
        raise PlaceError(f"lrt_place_describe failed ({rc}): {lib.lrt_place_last_error().decode()}")
    return (desc, sums) if batched else (desc[0], sums[0])


# ---- 2. the matcher -----------------------------------------------------------------------------------------------------------------------------------------

@torch.no_grad()
def match_reference(desc, gap=DEFAULT_GAP):
    """The numpy twin of ``match``: (best_d, best_s) (F, F) int32 CPU tensors.  A roll, an absolute difference and a sum per shift -- deliberately
    not the device's walk."""
    d, F, NS, NRP = _descriptors(desc)
    gap = _gap(gap)
    a = d.cpu().numpy().astype(np.int32)
    best_d = np.full((F, F), np.iinfo(np.int32).max, np.int64)
    best_s = np.zeros((F, F), np.int64)
    for s in range(NS):
        q = np.roll(a, -s, axis=1)                                          # q[i, c] = a[i, (c + s) mod NS]
        D = np.stack([np.abs(q[i][None] - a).sum((1, 2)) for i in range(F)])
        better = D < best_d                                                 # strictly: the lowest shift keeps a tie
        best_d = np.where(better, D, best_d)
        best_s = np.where(better, s, best_s)
    i, j = np.meshgrid(np.arange(F), np.arange(F), indexing="ij")
    inside = j + gap <= i
    return (torch.from_numpy(np.where(inside, best_d, -1).astype(np.int32)), torch.from_numpy(np.where(inside, best_s, -1).astype(np.int32)))


@torch.no_grad()
def match(desc, gap=DEFAULT_GAP):
    """(best_d, best_s) (F, F) int32: every query i against every candidate j with ``j + gap <= i`` at every shift (see the module text)."""
    d, F, NS, NRP = _descriptors(desc)
    dev = d.device
    if dev.type != "cuda":
        return match_reference(desc, gap)
    gap = _gap(gap)
    lib = load()
    best_d = torch.empty((F, F), dtype=torch.int32, device=dev)
    best_s = torch.empty((F, F), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.lrt_place_match(dev.index, F, NRP, NS, d.data_ptr(), gap, best_d.data_ptr(), best_s.data_ptr(), _stream(dev))
    if rc != 0:
        raise PlaceError(f"lrt_place_match failed ({rc}): {lib.lrt_place_last_error().decode()}")
    return best_d, best_s


# ---- 3. host code, shared by both paths ---------------------------------------------------------------------------------------------------------------------

def _host(t, dtype):
    return np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype)


def score(best_d, sums):
    """(F, F) float64: ``best_d / (sum_i + sum_j)`` in [0, 1]; 0 / 0 is 1 (two empty descriptors are not alike); NaN outside the triangle."""
    bd, sm = _host(best_d, np.int64), _host(sums, np.int64).reshape(-1)
    if bd.ndim != 2 or bd.shape[0] != bd.shape[1] or sm.size != bd.shape[0]:
        raise PlaceError(f"score: best_d {bd.shape} and sums {sm.shape} (an (F, F) table and F sums)")
    den = sm[:, None] + sm[None, :]
    out = np.where(den > 0, bd / np.maximum(den, 1), 1.0)
    return np.where(bd >= 0, out, np.nan)


def candidates(best_d, best_s, sums, top=DEFAULT_TOP, max_score=DEFAULT_MAX_SCORE):
    """[(i, j, score, s)]: per query ``i`` the ``top`` lowest scores at or below ``max_score``, ties to the lower ``j``; queries ascend.  A pair of
    empty descriptors is no candidate whatever ``max_score`` says."""
    top, max_score = int(top), float(max_score)
    if top < 1:
        raise PlaceError(f"candidates: top {top} (at least 1)")
    if not 0.0 <= max_score <= 1.0:
        raise PlaceError(f"candidates: max_score {max_score} (a score lies in [0, 1])")
    sc = score(best_d, sums)
    bs, sm = _host(best_s, np.int64), _host(sums, np.int64).reshape(-1)
    out = []
    for i in range(sc.shape[0]):
        row = [(float(sc[i, j]), j) for j in range(sc.shape[1]) if not math.isnan(sc[i, j]) and sc[i, j] <= max_score and sm[i] + sm[j] > 0]
        for s_, j in sorted(row)[:top]:
            out.append((i, j, s_, int(bs[i, j])))
    return out


def shift_to_init(s, sectors, up=(0.0, 0.0, 1.0)):
    """The (3, 4) float64 initial guess of ``registration.align``, source ``i`` onto target ``j``, for ``best_s[i, j] = s``: a rotation about ``up``
    and no translation.

    The sign.  Column ``w`` of the ray grid has the azimuth ``(W - w - off) / W 2 pi - pi - yaw`` (``RangeFrames.range_rays``): it FALLS as ``w``
    grows, by ``2 pi / sectors`` per sector.  ``D(i, j, s)`` compares ``a_i[c + s]`` with ``a_j[c]``, so what frame ``j`` sees in sector ``c``
    frame ``i`` sees ``s`` sectors later, at an azimuth that is ``2 pi s / sectors`` smaller.  ``X = T_j^-1 T_i`` takes a point of ``i`` to ``j``,
    where its azimuth is that much LARGER: a rotation about ``up`` by ``+ 2 pi s / sectors``."""
    sectors, s = int(sectors), int(s)
    if sectors < 1 or not 0 <= s < sectors:
        raise PlaceError(f"shift_to_init: shift {s} of {sectors} sectors")
    u = np.asarray(up, np.float64).reshape(-1)
    if u.size != 3 or not abs(float(u @ u) - 1.0) < 1e-6:
        raise PlaceError(f"shift_to_init: up {u.tolist()} is not a unit vector")
    a = 2.0 * math.pi * s / sectors
    K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    X = np.zeros((3, 4))
    X[:, :3] = np.eye(3) + math.sin(a) * K + (1.0 - math.cos(a)) * (K @ K)
    return X
