"""Range-image segmentation through ``csrc/liblrt_segment.so``: the five operators under ``actors.discover``, which turns a sequence of scans with
poses into the tracking boxes of its moving actors -- the last input of a dynamic scene that used to come from a dataset's labels.

    pts, mask   = frame_points(depth, mask, inclination, H, W, data_type="KITTI", sensor2ego=None)
    g           = ground(pts, mask, sensor_height, inclination, up=(0, 0, 1), slope=tan(10 deg))      # (F, H, W) uint8
    lab         = label(pts, mask, exclude=g, inclination=..., d_abs=0.15, c_h=None, c_v=None)        # (F, H, W) int32
    ev          = freespace((pts, mask), (tgt_range, tgt_mask), X, inclination=..., window=(1, 2))    # (F, H, W) int8
    st          = stats(pts, lab, (ev_prev, ev_next), s_max)                                          # seg, n_seg, overflow, table
    bounds, cnt = track_bounds(pts, st.seg, track_of, pose)                                            # (NT, 6) int64, (NT) int64

All take ``F`` frames of one ``H x W`` sensor model (or one frame without the leading axis); a frame's result does not depend on the frames beside
it.  ``include/lrt_segment.h`` states every rule and ``csrc/lrt_segment_math.h`` is its text for the device and the host.  EVERY RESULT IS AN
INTEGER that does not depend on the order in which lanes arrive, so the numpy twins (``*_reference``) are exact: the tests are equalities.

* HIP tensors go through the library (ground 1 launch, label 3, freespace 1, stats 5, track_bounds 2, whatever the images hold; no host wait).  A
  missing library is an error, not a quiet fall-back.  CPU tensors go to the twins, which run anywhere; their integer tables are int64 numpy
  underneath.  The labelling twin is a plain breadth-first flood in ascending index -- deliberately not the device's union-find.
* ``label``: the SMALLEST linear pixel index ``h W + w`` of the pixel's component, -1 for a pixel that is not kept.  With the defaults
  ``d_abs = 0.15`` m, ``c_h = 4 * 2 pi / W`` and ``c_v = 4 * (inclination span) / (H - 1)`` a surface stays connected up to an incidence of about
  76 degrees: neighbouring returns on it are ``r dtheta / cos(incidence)`` apart, and ``1 / cos = 4`` there.
* ``ground``: nothing is guessed from the data -- ``sensor_height`` (the sensor above the ground, metres) is required, and the band of the first
  ground pixel of a column is ``-(sensor_height +- 0.4)`` along ``up`` unless ``z_lo`` / ``z_hi`` say otherwise.
* ``stats``: a table row is ``root, count, free_0, known_0, free_1, known_1, sum q (3), min q (3), max q (3), 0`` with ``q = llrint(p * 1024)``.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from collections import deque
from types import SimpleNamespace

import numpy as np
import torch

from . import range_image, registration as rg, sweep as sw

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LRT_SEGMENT_LIB") or os.path.join(HERE, "csrc", "liblrt_segment.so")
EXPORTS = ("lrt_segment_abi_version", "lrt_segment_last_error", "lrt_seg_work_bytes", "lrt_seg_ground", "lrt_seg_label", "lrt_seg_freespace",
           "lrt_seg_stats", "lrt_seg_track_bounds")                          # include/lrt_segment.h
ABI_VERSION = 1
BLOCK = 256                                                                  # LRT_SEGMENT_BLOCK
NCOL = 16                                                                    # LRT_SEGMENT_NCOL
MAX_RH, MAX_RW, MAX_FRAMES, MAX_SEGMENTS, MAX_TRACKS = 4, 16, 65535, 1048576, 65535
MAX_PIXELS = (2 ** 31 - 1) // 3                                              # LRT_SEGMENT_MAX_PIXELS
COL_ROOT, COL_COUNT, COL_EV, COL_SUM, COL_MIN, COL_MAX = 0, 1, 2, 6, 9, 12
QUANT = 1024.0
QUANT_LIMIT = 9.0e15
I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min
FLT_MAX = rg.FLT_MAX
DEFAULT_SLOPE = math.tan(math.radians(10.0))
DEFAULT_BAND = 0.4
DEFAULT_D_ABS = 0.15
DEFAULT_WINDOW = (1, 2)
DEFAULT_M_ABS, DEFAULT_M_REL = 0.5, 0.02

_lib = None


class SegmentationError(RuntimeError):
    pass


class Stats(SimpleNamespace):
    """seg (F, H, W) int32, n_seg (F) int32, overflow (F) int32, table (F, S_max, 16) int64; without a frame axis in the inputs, without one here."""

    def __iter__(self):
        return iter((self.seg, self.n_seg, self.overflow, self.table))


def load():
    """Load liblrt_segment.so (after torch, so that both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SegmentationError(f"{LIB_PATH} is missing: build it with `python -m lidar_rt_amd.build` (hipcc --offload-arch=gfx950). "
                                "segmentation has no fall-back on a HIP device.")
    lib = C.CDLL(LIB_PATH)
    vp, ci, ll, d = C.c_void_p, C.c_int, C.c_longlong, C.c_double
    lib.lrt_segment_abi_version.restype = ci
    lib.lrt_segment_last_error.restype = C.c_char_p
    lib.lrt_seg_work_bytes.restype = ll
    lib.lrt_seg_work_bytes.argtypes = [ll, ci, ci]
    head = [ci, ll, ci, ci]
    lib.lrt_seg_ground.restype = ci
    lib.lrt_seg_ground.argtypes = head + [vp, ci, vp, vp, d, d, d, d, d, d, vp, vp]
    lib.lrt_seg_label.restype = ci
    lib.lrt_seg_label.argtypes = head + [vp, vp, vp, d, d, d, vp, vp]
    lib.lrt_seg_freespace.restype = ci
    lib.lrt_seg_freespace.argtypes = head + [vp, ci, d, d, d, d, vp, vp, vp, vp, vp, ci, ci, d, d, vp, vp]
    lib.lrt_seg_stats.restype = ci
    lib.lrt_seg_stats.argtypes = head + [vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, ll, vp]
    lib.lrt_seg_track_bounds.restype = ci
    lib.lrt_seg_track_bounds.argtypes = head + [vp, vp, ci, vp, ci, vp, vp, vp, vp]
    if lib.lrt_segment_abi_version() != ABI_VERSION:
        raise SegmentationError("liblrt_segment.so ABI version mismatch; rebuild with `python -m lidar_rt_amd.build --force`")
    _lib = lib
    return lib


# ---- the arguments ------------------------------------------------------------------------------------------------------------------------------------------

def _frames(fn, points, mask=None):
    """(points (F, H, W, 3) float32, mask (F, H, W) uint8 or None, batched, F, H, W)."""
    if not torch.is_tensor(points) or points.dim() not in (3, 4) or points.shape[-1] != 3 or points.dtype != torch.float32:
        raise SegmentationError(f"{fn}: points must be a float32 (H, W, 3) or (F, H, W, 3) tensor")
    batched = points.dim() == 4
    points = points.detach().contiguous()
    points = points if batched else points[None]
    F, H, W = (int(x) for x in points.shape[:3])
    if F < 1 or F > MAX_FRAMES or H < 1 or W < 1 or F * H * W > MAX_PIXELS:
        raise SegmentationError(f"{fn}: {F} frames of {H} x {W} pixels (each at least 1, at most {MAX_FRAMES} frames, F H W at most {MAX_PIXELS})")
    if mask is not None:
        mask = _image(fn, "mask", mask, points, batched, None)
    return points, mask, batched, F, H, W


def _image(fn, name, t, points, batched, dtype):
    """An (F, H, W) companion of `points` on its device; dtype None: a mask, made uint8."""
    shape = tuple(points.shape[:3]) if batched else tuple(points.shape[1:3])
    if not torch.is_tensor(t) or tuple(t.shape) != shape or t.device != points.device:
        raise SegmentationError(f"{fn}: {name} must be a {shape} tensor on {points.device}")
    t = t.detach()
    if dtype is None:
        t = rg._mask8(t)
    elif t.dtype != dtype:
        raise SegmentationError(f"{fn}: {name} must be {dtype} (it is {t.dtype})")
    t = t.contiguous()
    return t if batched else t[None]


def _inclination(fn, inclination, H):
    if inclination is None:
        raise SegmentationError(f"{fn}: inclination is required (two bounds or a per-beam table)")
    inc = np.ascontiguousarray(np.asarray(inclination, np.float64).reshape(-1))
    if inc.size != 2 and (inc.size != H or H < 3):
        raise SegmentationError(f"{fn}: {inc.size} inclinations (2 bounds, or one per row of at least 3: {H})")
    return inc


def _model(fn, H, W, inclination, data_type, sensor2ego, min_depth, max_depth):
    try:
        return rg._model(H, W, inclination, data_type, sensor2ego, min_depth, max_depth)
    except rg.RegistrationError as e:
        raise SegmentationError(str(e).replace("registration", fn)) from None


def _np(t):
    return t.detach().cpu().numpy()


def _sq(batched, t):
    return t if batched else t[0]


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _call(name, dev, *args):
    lib = load()
    with torch.cuda.device(dev):
        rc = getattr(lib, name)(dev.index, *args, _stream(dev))
    if rc != 0:
        raise SegmentationError(f"{name} failed ({rc}): {lib.lrt_segment_last_error().decode()}")


def _ptr(t):
    return None if t is None else t.data_ptr()


def row_order(inc, H):
    """The rows in the order of ascending inclination (sg_row_at)."""
    return np.arange(H - 1, -1, -1) if inc[-1] > inc[0] else np.arange(H)


def default_thresholds(H, W, inclination):
    """(c_h, c_v) of ``label``: four times the angular pixel pitch."""
    inc = np.asarray(inclination, np.float64).reshape(-1)
    return 4.0 * 2.0 * math.pi / W, (4.0 * abs(float(inc[-1] - inc[0])) / (H - 1) if H > 1 else 0.0)


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------------------------

@torch.no_grad()
def frame_points(depth, mask, inclination, H=None, W=None, data_type="KITTI", sensor2ego=None):
    """(points (H, W, 3) float32, mask (H, W) bool) of one range image in its SENSOR frame: what ``registration.frame_geometry`` forms, without
    the normals.  HIP tensors stay on the device; there is no host wait."""
    if not torch.is_tensor(depth) or depth.dim() != 2:
        raise SegmentationError("frame_points: depth must be an (H, W) tensor")
    if (H is not None and int(H) != depth.shape[0]) or (W is not None and int(W) != depth.shape[1]):
        raise SegmentationError(f"frame_points: depth is {tuple(depth.shape)}, not ({H}, {W})")
    H, W = int(depth.shape[0]), int(depth.shape[1])
    dev = depth.device
    depth = depth.detach().to(torch.float32).contiguous()
    mask = (mask.detach() != 0).to(dev)
    P = torch.eye(4, dtype=torch.float32, device=dev)[:3].contiguous()
    _, d = sw.sweep_rays(P, None, H, W, inclination, data_type, sensor2ego)
    points = torch.where(mask[..., None], d.contiguous() * depth[..., None], torch.zeros_like(d))
    return points.contiguous(), mask


# ---- 1. ground ------------------------------------------------------------------------------------------------------------------------------------------------

def _ground_arguments(sensor_height, up, slope, z_lo, z_hi):
    if sensor_height is None and (z_lo is None or z_hi is None):
        raise SegmentationError("ground: sensor_height is required (the height of the sensor above the ground, metres): nothing is guessed from the data")
    up = np.asarray(up, np.float64).reshape(-1)
    if up.size != 3 or not abs(float(up @ up) - 1.0) < 1e-6:
        raise SegmentationError(f"ground: up {up.tolist()} is not a unit vector")
    z_lo = -(float(sensor_height) + DEFAULT_BAND) if z_lo is None else float(z_lo)
    z_hi = -(float(sensor_height) - DEFAULT_BAND) if z_hi is None else float(z_hi)
    slope = float(slope)
    if not (math.isfinite(z_lo) and math.isfinite(z_hi) and z_lo <= z_hi):
        raise SegmentationError(f"ground: the height band [{z_lo}, {z_hi}] (z_lo <= z_hi)")
    if not (slope >= 0.0 and math.isfinite(slope)):
        raise SegmentationError(f"ground: slope {slope} (not negative)")
    return up, slope, z_lo, z_hi


@torch.no_grad()
def ground_reference(points, mask, sensor_height=None, inclination=None, up=(0.0, 0.0, 1.0), slope=DEFAULT_SLOPE, z_lo=None, z_hi=None, return_margin=False):
    """The numpy twin of ``ground``: a CPU uint8 tensor.  ``return_margin=True`` adds the smallest relative distance of a decision from its threshold."""
    pts, m, batched, F, H, W = _frames("ground", points, mask)
    inc = _inclination("ground", inclination, H)
    up, slope, z_lo, z_hi = _ground_arguments(sensor_height, up, slope, z_lo, z_hi)
    p, m = _np(pts).astype(np.float64), _np(m) != 0
    out = np.zeros((F, H, W), np.uint8)
    have = np.zeros((F, W), bool)
    hg, gg = np.zeros((F, W)), np.zeros((F, W, 3))
    margin = np.inf
    with np.errstate(all="ignore"):
        for r in row_order(inc, H):
            x, y, z = p[:, r, :, 0], p[:, r, :, 1], p[:, r, :, 2]
            h = up[0] * x + up[1] * y + up[2] * z
            g = np.stack([x - h * up[0], y - h * up[1], z - h * up[2]], -1)
            d = g - gg
            reach = slope * np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
            near = np.abs(h - hg) <= reach
            gr = m[:, r] & np.where(have, near, (h >= z_lo) & (h <= z_hi))
            dist = np.where(have, np.abs(np.abs(h - hg) - reach) / np.maximum(reach, 1e-300), np.minimum(np.abs(h - z_lo), np.abs(h - z_hi)) / max(abs(z_lo), abs(z_hi), 1e-300))
            if m[:, r].any():
                margin = min(margin, float(dist[m[:, r]].min()))
            out[:, r] = gr
            have |= gr
            hg = np.where(gr, h, hg)
            gg = np.where(gr[..., None], g, gg)
    res = _sq(batched, torch.from_numpy(out))
    return (res, margin) if return_margin else res


@torch.no_grad()
def ground(points, mask, sensor_height=None, inclination=None, up=(0.0, 0.0, 1.0), slope=DEFAULT_SLOPE, z_lo=None, z_hi=None):
    """ground (F, H, W) uint8 by the column scan of the module text; ``inclination`` gives the row order."""
    pts, m, batched, F, H, W = _frames("ground", points, mask)
    dev = pts.device
    if dev.type != "cuda":
        return ground_reference(points, mask, sensor_height, inclination, up, slope, z_lo, z_hi)
    inc = _inclination("ground", inclination, H)
    up, slope, z_lo, z_hi = _ground_arguments(sensor_height, up, slope, z_lo, z_hi)
    d_inc = range_image._upload(inc, dev)
    out = torch.empty((F, H, W), dtype=torch.uint8, device=dev)
    _call("lrt_seg_ground", dev, F, H, W, d_inc.data_ptr(), int(inc.size), pts.data_ptr(), m.data_ptr(), float(up[0]), float(up[1]), float(up[2]), z_lo, z_hi,
          slope, out.data_ptr())
    return _sq(batched, out)


# ---- 2. labels ------------------------------------------------------------------------------------------------------------------------------------------------

def _label_arguments(H, W, inclination, d_abs, c_h, c_v):
    if c_h is None or c_v is None:
        if inclination is None:
            raise SegmentationError("label: inclination is required for the default c_h / c_v (or give both)")
        dh, dv = default_thresholds(H, W, inclination)
        c_h, c_v = (dh if c_h is None else c_h), (dv if c_v is None else c_v)
    d_abs, c_h, c_v = float(d_abs), float(c_h), float(c_v)
    if not all(v >= 0.0 and math.isfinite(v) for v in (d_abs, c_h, c_v)):
        raise SegmentationError(f"label: thresholds d_abs {d_abs}, c_h {c_h}, c_v {c_v} (not negative)")
    return d_abs, c_h, c_v


def _fma32(a, b, c):
    """fma(a, b, c) on float32 arrays: the product is exact in float64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _r2(p):
    return _fma32(p[..., 2], p[..., 2], _fma32(p[..., 1], p[..., 1], p[..., 0] * p[..., 0]))


def join_reference(a, b, d_abs, c_dir):
    """sg_join on float32 (..., 3) arrays."""
    with np.errstate(all="ignore"):
        d2 = _r2(a - b)
        ra, rb = _r2(a), _r2(b)
        m = np.where(ra < rb, ra, rb)
        da, cd = np.float32(d_abs), np.float32(c_dir)
        rel = (cd * cd) * m
        bound = np.where((da * da) > rel, da * da, rel)
        return d2 <= bound


def _flood(kept, jr, jd):
    """One frame: breadth-first from every unlabelled kept pixel in ascending index.  jr[h, w]: (h, w) with (h, (w + 1) % W); jd[h, w]: with (h + 1, w)."""
    H, W = kept.shape
    lab = np.full(H * W, -1, np.int32)
    kept, jr, jd = kept.reshape(-1), jr.reshape(-1), jd.reshape(-1)
    for s in np.nonzero(kept)[0]:
        if lab[s] >= 0:
            continue
        lab[s] = s
        todo = deque([int(s)])
        while todo:
            i = todo.popleft()
            h, w = divmod(i, W)
            right, left = h * W + (w + 1) % W, h * W + (w - 1) % W
            for j, ok in ((right, jr[i]), (left, jr[left]), (i + W, h + 1 < H and jd[i]), (i - W, h > 0 and jd[i - W])):
                if ok and j != i and lab[j] < 0:
                    lab[j] = s
                    todo.append(j)
    return lab.reshape(H, W)


@torch.no_grad()
def label_reference(points, mask, exclude=None, inclination=None, d_abs=DEFAULT_D_ABS, c_h=None, c_v=None):
    """The numpy twin of ``label``: a CPU int32 tensor."""
    pts, m, batched, F, H, W = _frames("label", points, mask)
    ex = None if exclude is None else _image("label", "exclude", exclude, pts, batched, None)
    d_abs, c_h, c_v = _label_arguments(H, W, inclination, d_abs, c_h, c_v)
    p = _np(pts)
    kept = (_np(m) != 0) & ((_np(ex) == 0) if ex is not None else True)
    jr = kept & np.roll(kept, -1, 2) & join_reference(p, np.roll(p, -1, 2), d_abs, c_h)
    if W == 1:
        jr[:] = False
    jd = np.zeros_like(kept)
    if H > 1:
        jd[:, :-1] = kept[:, :-1] & kept[:, 1:] & join_reference(p[:, :-1], p[:, 1:], d_abs, c_v)
    out = np.stack([_flood(kept[f], jr[f], jd[f]) for f in range(F)])
    return _sq(batched, torch.from_numpy(out))


@torch.no_grad()
def label(points, mask, exclude=None, inclination=None, d_abs=DEFAULT_D_ABS, c_h=None, c_v=None):
    """label (F, H, W) int32: the smallest linear pixel index of the pixel's component, -1 where not kept (see the module text for the defaults
    and the 76 degrees of incidence they allow).  ``exclude``: pixels to leave out, the ground as a rule."""
    pts, m, batched, F, H, W = _frames("label", points, mask)
    dev = pts.device
    if dev.type != "cuda":
        return label_reference(points, mask, exclude, inclination, d_abs, c_h, c_v)
    ex = None if exclude is None else _image("label", "exclude", exclude, pts, batched, None)
    d_abs, c_h, c_v = _label_arguments(H, W, inclination, d_abs, c_h, c_v)
    out = torch.empty((F, H, W), dtype=torch.int32, device=dev)
    _call("lrt_seg_label", dev, F, H, W, pts.data_ptr(), m.data_ptr(), _ptr(ex), d_abs, c_h, c_v, out.data_ptr())
    return _sq(batched, out)


# ---- 3. free space --------------------------------------------------------------------------------------------------------------------------------------------

def _free_arguments(src, tgt, X, window, m_abs, m_rel):
    if not isinstance(src, (tuple, list)) or len(src) != 2 or not isinstance(tgt, (tuple, list)) or len(tgt) != 2:
        raise SegmentationError("freespace: src must be (points, mask) and tgt (range, mask)")
    sp, sm, batched, F, H, W = _frames("freespace", src[0], src[1])
    tr = _image("freespace", "tgt's range", tgt[0], sp, batched, torch.float32)
    tm = _image("freespace", "tgt's mask", tgt[1], sp, batched, None)
    rh, rw = int(window[0]), int(window[1])
    if not (0 <= rh <= MAX_RH and 0 <= rw <= MAX_RW):
        raise SegmentationError(f"freespace: a window of {rh} rows and {rw} columns either side (at most {MAX_RH} and {MAX_RW})")
    m_abs, m_rel = float(m_abs), float(m_rel)
    if not all(v >= 0.0 and math.isfinite(v) for v in (m_abs, m_rel)):
        raise SegmentationError(f"freespace: margins m_abs {m_abs}, m_rel {m_rel} (not negative)")
    try:
        Xd = rg._poses("X", X, F, batched, sp.device)
    except rg.RegistrationError as e:
        raise SegmentationError(str(e).replace("registration", "freespace")) from None
    return sp, sm, tr, tm, Xd, batched, F, H, W, rh, rw, m_abs, m_rel


@torch.no_grad()
def freespace_reference(src, tgt, X, inclination=None, data_type="KITTI", sensor2ego=None, window=DEFAULT_WINDOW, m_abs=DEFAULT_M_ABS, m_rel=DEFAULT_M_REL,
                        min_depth=0.0, max_depth=FLT_MAX, return_margin=False):
    """The numpy twin of ``freespace``: a CPU int8 tensor.  ``return_margin=True`` adds the smallest relative distance of a float64 decision
    (range against threshold) from its threshold, over the pixels with a verdict: what the test cases are conditioned on."""
    sp, sm, tr, tm, Xd, batched, F, H, W, rh, rw, m_abs, m_rel = _free_arguments(src, tgt, X, window, m_abs, m_rel)
    inc, off, yaw, lo, hi = _model("freespace", H, W, inclination, data_type, sensor2ego, min_depth, max_depth)
    sp, sm, tr, tm, Xn = (_np(t) for t in (sp, sm, tr, tm, Xd))
    out = np.full((F, H * W), -1, np.int8)
    margin = np.inf
    for f in range(F):
        idx = np.nonzero(sm[f].reshape(-1))[0]
        p = sp[f].reshape(-1, 3)[idx].astype(np.float64)
        Xf = Xn[f]
        q = np.stack([Xf[k, 0] * p[:, 0] + Xf[k, 1] * p[:, 1] + Xf[k, 2] * p[:, 2] + Xf[k, 3] for k in range(3)], 1) if idx.size else np.zeros((0, 3))
        keep, h0, w0 = rg._classify(q, H, W, inc, off, yaw, lo, hi)
        with np.errstate(all="ignore"):
            rq = np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2])
            thr = rq + m_abs + m_rel * rq
        trf, tmf = tr[f].reshape(-1).astype(np.float64), tm[f].reshape(-1) != 0
        n, through = np.zeros(idx.size, np.int64), np.ones(idx.size, bool)
        for dh in range(-rh, rh + 1):
            h = h0 + dh
            row_ok = keep & (h >= 0) & (h < H)
            for dw in range(-rw, rw + 1):
                j = np.clip(h, 0, H - 1) * W + (w0 + dw) % W
                seen = row_ok & tmf[j]
                n += seen
                with np.errstate(all="ignore"):
                    through &= ~seen | (trf[j] > thr)
                    if seen.any():
                        margin = min(margin, float(np.nanmin(np.abs(trf[j][seen] - thr[seen]) / thr[seen])))
        out[f, idx] = np.where(n == 0, -1, through.astype(np.int8))
    res = _sq(batched, torch.from_numpy(out.reshape(F, H, W)))
    return (res, margin) if return_margin else res


@torch.no_grad()
def freespace(src, tgt, X, inclination=None, data_type="KITTI", sensor2ego=None, window=DEFAULT_WINDOW, m_abs=DEFAULT_M_ABS, m_rel=DEFAULT_M_REL,
              min_depth=0.0, max_depth=FLT_MAX):
    """ev (F, H, W) int8: has the target frame seen through the place of every source point?  1 free, 0 occupied, -1 unknown.  ``X`` is the source
    sensor's pose in the target sensor's frame, ``X = T_tgt^-1 T_src``, as in ``registration``."""
    sp, sm, tr, tm, Xd, batched, F, H, W, rh, rw, m_abs, m_rel = _free_arguments(src, tgt, X, window, m_abs, m_rel)
    dev = sp.device
    if dev.type != "cuda":
        return freespace_reference(src, tgt, X, inclination, data_type, sensor2ego, window, m_abs, m_rel, min_depth, max_depth)
    inc, off, yaw, lo, hi = _model("freespace", H, W, inclination, data_type, sensor2ego, min_depth, max_depth)
    d_inc = range_image._upload(inc, dev)
    out = torch.empty((F, H, W), dtype=torch.int8, device=dev)
    _call("lrt_seg_freespace", dev, F, H, W, d_inc.data_ptr(), int(inc.size), off, yaw, lo, hi, sp.data_ptr(), sm.data_ptr(), tr.data_ptr(), tm.data_ptr(),
          Xd.data_ptr(), rh, rw, m_abs, m_rel, out.data_ptr())
    return _sq(batched, out)


# ---- 4. the table ---------------------------------------------------------------------------------------------------------------------------------------------

def quant_reference(v):
    """sg_quant64 on a float64 array: int64."""
    with np.errstate(all="ignore"):
        s = v * QUANT
        ok = np.abs(s) < QUANT_LIMIT
        return np.rint(np.where(ok, s, 0.0)).astype(np.int64)


def _stat_arguments(points, lab, ev, s_max):
    pts, _, batched, F, H, W = _frames("stats", points)
    lab = _image("stats", "label", lab, pts, batched, torch.int32)
    ev = tuple(ev) if ev is not None else ()
    if len(ev) > 2:
        raise SegmentationError("stats: at most two evidence images")
    ev = tuple(None if e is None else _image("stats", "an evidence image", e, pts, batched, torch.int8) for e in ev) + (None,) * (2 - len(ev))
    s_max = int(s_max)
    if not (1 <= s_max <= MAX_SEGMENTS and F * s_max <= MAX_PIXELS):
        raise SegmentationError(f"stats: a capacity of {s_max} segments per frame (1 to {MAX_SEGMENTS}, F S_max at most {MAX_PIXELS})")
    return pts, lab, ev, s_max, batched, F, H, W


@torch.no_grad()
def stats_reference(points, lab, ev=(), s_max=4096) -> Stats:
    """The numpy twin of ``stats``; the table is int64 numpy underneath a CPU tensor."""
    pts, lab, ev, s_max, batched, F, H, W = _stat_arguments(points, lab, ev, s_max)
    HW = H * W
    p, L = _np(pts).reshape(F, HW, 3), _np(lab).reshape(F, HW)
    seg = np.full((F, HW), -1, np.int32)
    n_seg, overflow = np.zeros(F, np.int32), np.zeros(F, np.int32)
    table = np.zeros((F, s_max, NCOL), np.int64)
    for f in range(F):
        roots = np.nonzero(L[f] == np.arange(HW))[0]
        n = min(roots.size, s_max)
        n_seg[f], overflow[f] = n, roots.size - n
        dense = np.full(HW, -1, np.int32)
        dense[roots[:n]] = np.arange(n, dtype=np.int32)
        ok = (L[f] >= 0) & (L[f] < HW)
        seg[f] = np.where(ok, dense[np.clip(L[f], 0, HW - 1)], -1)
        px = np.nonzero(seg[f] >= 0)[0]
        s = seg[f][px]
        t = table[f]
        t[:n, COL_ROOT] = roots[:n]
        np.add.at(t[:, COL_COUNT], s, 1)
        for k, e in enumerate(ev):
            if e is not None:
                e = _np(e).reshape(F, HW)[f][px]
                np.add.at(t[:, COL_EV + 2 * k], s, (e == 1).astype(np.int64))
                np.add.at(t[:, COL_EV + 2 * k + 1], s, (e >= 0).astype(np.int64))
        q = quant_reference(p[f][px].astype(np.float64))
        t[:n, COL_MIN:COL_MIN + 3], t[:n, COL_MAX:COL_MAX + 3] = I64_MAX, I64_MIN
        for k in range(3):
            np.add.at(t[:, COL_SUM + k], s, q[:, k])
            np.minimum.at(t[:, COL_MIN + k], s, q[:, k])
            np.maximum.at(t[:, COL_MAX + k], s, q[:, k])
    res = [torch.from_numpy(a) for a in (seg.reshape(F, H, W), n_seg, overflow, table)]
    return Stats(**dict(zip(("seg", "n_seg", "overflow", "table"), (_sq(batched, r) for r in res))))


def work_bytes(F: int, H: int, W: int) -> int:
    """Bytes of the workspace of ``stats``: two counts per workgroup."""
    n = int(load().lrt_seg_work_bytes(int(F), int(H), int(W)))
    if n < 0:
        raise SegmentationError(f"stats: {F} frames of {H} x {W} pixels (each at least 1, at most {MAX_FRAMES} frames, F H W at most {MAX_PIXELS})")
    return n


@torch.no_grad()
def stats(points, lab, ev=(), s_max=4096, workspace=None) -> Stats:
    """One integer row per segment (see the module text).  ``ev``: up to two evidence images of ``freespace``; ``s_max``: the capacity per frame --
    segments numbered at or beyond it are counted in ``overflow`` and their pixels get ``seg = -1``."""
    pts, lab_, ev_, s_max, batched, F, H, W = _stat_arguments(points, lab, ev, s_max)
    dev = pts.device
    if dev.type != "cuda":
        if workspace is not None:
            raise SegmentationError(f"stats: a workspace with tensors on {dev}")
        return stats_reference(points, lab, ev, s_max)
    try:
        ws = rg._workspace(workspace, work_bytes(F, H, W), dev)
    except rg.RegistrationError as e:
        raise SegmentationError(str(e).replace("lrt_reg", "stats")) from None
    seg = torch.empty((F, H, W), dtype=torch.int32, device=dev)
    n_seg = torch.empty((F,), dtype=torch.int32, device=dev)
    overflow = torch.empty((F,), dtype=torch.int32, device=dev)
    table = torch.empty((F, s_max, NCOL), dtype=torch.int64, device=dev)
    _call("lrt_seg_stats", dev, F, H, W, pts.data_ptr(), lab_.data_ptr(), _ptr(ev_[0]), _ptr(ev_[1]), s_max, seg.data_ptr(), n_seg.data_ptr(),
          overflow.data_ptr(), table.data_ptr(), ws.data_ptr(), ws.numel())
    return Stats(seg=_sq(batched, seg), n_seg=_sq(batched, n_seg), overflow=_sq(batched, overflow), table=_sq(batched, table))


# ---- 5. track bounds ------------------------------------------------------------------------------------------------------------------------------------------

def _bound_arguments(points, seg, track_of, pose):
    pts, _, batched, F, H, W = _frames("track_bounds", points)
    seg = _image("track_bounds", "seg", seg, pts, batched, torch.int32)
    dev = pts.device
    if not torch.is_tensor(track_of) or track_of.dtype != torch.int32 or track_of.device != dev or track_of.dim() != (2 if batched else 1) \
            or (batched and track_of.shape[0] != F):
        raise SegmentationError(f"track_bounds: track_of must be an int32 (F, S_max) tensor on {dev}")
    track_of = track_of.detach().contiguous()
    track_of = track_of if batched else track_of[None]
    s_max = int(track_of.shape[1])
    if not (1 <= s_max <= MAX_SEGMENTS and F * s_max <= MAX_PIXELS):
        raise SegmentationError(f"track_bounds: a capacity of {s_max} segments per frame (1 to {MAX_SEGMENTS}, F S_max at most {MAX_PIXELS})")
    want = "(NT, F, 3, 4)" if batched else "(NT, 3, 4)"
    if not torch.is_tensor(pose) or pose.dtype != torch.float64 or pose.device != dev or pose.dim() != (4 if batched else 3) or tuple(pose.shape[-2:]) != (3, 4) \
            or (batched and pose.shape[1] != F) or not 1 <= pose.shape[0] <= MAX_TRACKS:
        raise SegmentationError(f"track_bounds: pose must be a float64 {want} tensor on {dev} with 1 to {MAX_TRACKS} tracks")
    pose = pose.detach().contiguous()
    pose = pose if batched else pose[:, None]
    return pts, seg, track_of, pose.contiguous(), s_max, int(pose.shape[0]), F, H, W


@torch.no_grad()
def track_bounds_reference(points, seg, track_of, pose, return_margin=False):
    """The numpy twin of ``track_bounds``: (bounds (NT, 6) int64, count (NT) int64) as CPU tensors.  ``return_margin=True`` adds the smallest distance
    of an llrint argument from a half."""
    pts, seg, track_of, pose, s_max, NT, F, H, W = _bound_arguments(points, seg, track_of, pose)
    p, S, tof, T = _np(pts).reshape(F, -1, 3).astype(np.float64), _np(seg).reshape(F, -1), _np(track_of), _np(pose)
    bounds = np.empty((NT, 6), np.int64)
    bounds[:, :3], bounds[:, 3:] = I64_MAX, I64_MIN
    count = np.zeros(NT, np.int64)
    margin = np.inf
    for f in range(F):
        ok = (S[f] >= 0) & (S[f] < s_max)
        t = np.where(ok, tof[f][np.clip(S[f], 0, s_max - 1)], -1)
        px = np.nonzero((t >= 0) & (t < NT))[0]
        t = t[px]
        Tf = T[t, f]                                                          # (n, 3, 4)
        d = [p[f][px, k] - Tf[:, k, 3] for k in range(3)]
        a = np.stack([Tf[:, 0, k] * d[0] + Tf[:, 1, k] * d[1] + Tf[:, 2, k] * d[2] for k in range(3)], 1)
        if px.size:
            s = a * QUANT
            margin = min(margin, float(np.abs(np.abs(s - np.floor(s)) - 0.5).min()))
        q = quant_reference(a)
        for k in range(3):
            np.minimum.at(bounds[:, k], t, q[:, k])
            np.maximum.at(bounds[:, 3 + k], t, q[:, k])
        np.add.at(count, t, 1)
    res = (torch.from_numpy(bounds), torch.from_numpy(count))
    return res + (margin,) if return_margin else res


@torch.no_grad()
def track_bounds(points, seg, track_of, pose):
    """(bounds (NT, 6) int64: min x, y, z, max x, y, z of ``llrint(R^T (p - t) * 1024)`` over the pixels of each track's segments, count (NT) int64).
    ``track_of`` (F, S_max) int32: the track of every segment, -1 for none; ``pose`` (NT, F, 3, 4) float64: the actor in the SENSOR frame of that
    frame.  A track without pixels has count 0 and the bounds (INT64_MAX, INT64_MIN)."""
    pts, seg_, track_of_, pose_, s_max, NT, F, H, W = _bound_arguments(points, seg, track_of, pose)
    dev = pts.device
    if dev.type != "cuda":
        return track_bounds_reference(points, seg, track_of, pose)
    bounds = torch.empty((NT, 6), dtype=torch.int64, device=dev)
    count = torch.empty((NT,), dtype=torch.int64, device=dev)
    _call("lrt_seg_track_bounds", dev, F, H, W, pts.data_ptr(), seg_.data_ptr(), s_max, track_of_.data_ptr(), NT, pose_.data_ptr(), bounds.data_ptr(),
          count.data_ptr())
    return bounds, count
