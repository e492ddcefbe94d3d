"""Range images of a fused TSDF grid through ``csrc/liblrt_raycast.so``: what a sensor at a pose would see in the map that ``mesh.integrate`` built.

    r = raycast(grid, rays_o, rays_d, *, min_weight=1, step=None, far_step=None, min_depth=0.0, max_depth=80.0, samples=False)
        # Raycast: depth (...) float32, hit (...) bool, intensity (...) float32 or None, samples (...) int32 or None
    renders = render_frames(grid, sensor, frame_ids, **kw)                   # {frame: {"depth", "intensity", "raydrop"}}, evaluation.render_frames' layout

    python -m lidar_rt_amd.raycast --data DIR [--fuse train|all] [--frames test|train|all] [--voxel 0.1] [--sequence OUT] [--device cuda|cpu] ...

``include/lrt_raycast.h`` states the rule and ``csrc/lrt_raycast_math.h`` is its text for the device and the host.

* A ray is world-frame float32, exactly what the tracer takes (``sensor.rays[frame]``); in the grid frame ``o = ray_o - origin`` and ``u`` is the
  unit direction, in float64.  The ray marches through the box of voxel centres from ``max(min_depth, entry)`` to ``min(max_depth, exit)``:
  samples ``step`` apart (default half a voxel), ``far_step`` apart (default ``trunc - step``) after a known sample whose eight corners all hold
  exactly 1.0.  Its depth is the first crossing from a known positive sample to a known non-positive one, linearly interpolated: a range along the
  unit direction.  A miss is depth 0, hit False, intensity 0.
* HIP tensors go through the library (one launch per call); a missing library is a ``RaycastError``, not a quiet fall-back.  CPU tensors go to
  ``raycast_reference``, the numpy float64 twin, equal to the device bit for bit in depth, hit, intensity and samples.
* ``render_frames`` casts a sensor's own rays, so a sweep (``--sweep stored``) or a beam table applies as it does to ``evaluate``; its output goes to
  ``metrics.frame_metrics`` and ``simulate.clouds_from_renders`` as it is.
* ``--fuse-sweep stored`` FUSES under the sweep model (``sweep_fuse.integrate_sweep`` with each fused frame's stored twist), so that the grid is
  not sheared by the sensor's motion within a sweep; ``--sweep stored`` is how the rays are cast and does not imply it.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

from . import mesh

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LRT_RAYCAST_LIB") or os.path.join(HERE, "csrc", "liblrt_raycast.so")
EXPORTS = ("lrt_raycast_abi_version", "lrt_raycast_last_error", "lrt_raycast")   # include/lrt_raycast.h
ABI_VERSION = 1
BLOCK = 256                                                                  # LRT_RAYCAST_BLOCK
MAX_RAYS = 2 ** 31 - 1                                                       # LRT_RAYCAST_MAX_RAYS
MAX_SAMPLES = 2 ** 24                                                        # LRT_RAYCAST_MAX_SAMPLES

_lib = None


class RaycastError(RuntimeError):
    pass


class Raycast(SimpleNamespace):
    """depth float32, hit bool, intensity float32 or None, samples int32 or None; each shaped like the rays' leading dimensions."""


def load():
    """Load liblrt_raycast.so (after torch, so that both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RaycastError(f"{LIB_PATH} is missing: build it with `python -m lidar_rt_amd.build` (hipcc --offload-arch=gfx950). "
                           "raycast has no fall-back on a HIP device.")
    lib = C.CDLL(LIB_PATH)
    vp, ci, ll, d = C.c_void_p, C.c_int, C.c_longlong, C.c_double
    lib.lrt_raycast_abi_version.restype = ci
    lib.lrt_raycast_last_error.restype = C.c_char_p
    lib.lrt_raycast.restype = ci
    lib.lrt_raycast.argtypes = [ci, ci, ci, ci, d, d, d, d, d, vp, vp, vp, ci, ll, vp, vp, d, d, d, d, vp, vp, vp, vp, vp]
    if lib.lrt_raycast_abi_version() != ABI_VERSION:
        raise RaycastError("liblrt_raycast.so ABI version mismatch; rebuild with `python -m lidar_rt_amd.build --force`")
    _lib = lib
    return lib


# ---- the arguments ------------------------------------------------------------------------------------------------------------------------------------------

def params(grid, min_weight=1, step=None, far_step=None, min_depth=0.0, max_depth=80.0):
    """The checked (min_weight, step, far_step, min_depth, max_depth) of a call; every refusal names its argument, as the library's do."""
    if not isinstance(grid, mesh.TsdfGrid):
        raise RaycastError("raycast: grid must be a mesh.TsdfGrid")
    mw = int(min_weight)
    if mw < 1:
        raise RaycastError(f"raycast: min_weight {mw} (at least 1: weight 0 is unobserved)")
    step = 0.5 * float(grid.voxel) if step is None else float(step)
    far = float(grid.trunc) - step if far_step is None else float(far_step)
    if not (step > 0.0 and math.isfinite(step)):
        raise RaycastError(f"raycast: step {step} (positive)")
    if not (step <= far < float(grid.trunc)):
        raise RaycastError(f"raycast: far_step {far} (step {step} <= far_step < trunc {grid.trunc})")
    min_depth, max_depth = float(min_depth), float(max_depth)
    if not (0.0 <= min_depth < max_depth and math.isfinite(max_depth)):
        raise RaycastError(f"raycast: depths [{min_depth}, {max_depth}] (0 <= min_depth < max_depth)")
    if not (max_depth + step > max_depth):
        raise RaycastError(f"raycast: step {step} does not advance t at max_depth {max_depth}")
    X, Y, Z = grid.dims
    diag = float(grid.voxel) * math.sqrt(float(X) * X + float(Y) * Y + float(Z) * Z)
    if not (diag / step <= MAX_SAMPLES):
        raise RaycastError(f"raycast: step {step}: the grid's diagonal {diag} m is more than {MAX_SAMPLES} steps")
    return mw, step, far, min_depth, max_depth


def _rays(grid, rays_o, rays_d):
    """(o (N, 3), d (N, 3) contiguous float32 on the grid's device, the leading shape)."""
    dev = grid.device
    for name, t in (("rays_o", rays_o), ("rays_d", rays_d)):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() < 1 or t.shape[-1] != 3 or t.device != dev:
            raise RaycastError(f"raycast: {name} must be a float32 (..., 3) tensor on {dev}")
    if rays_o.shape != rays_d.shape:
        raise RaycastError(f"raycast: rays_o {tuple(rays_o.shape)} and rays_d {tuple(rays_d.shape)} differ in shape")
    lead = tuple(rays_o.shape[:-1])
    if math.prod(lead) > MAX_RAYS:
        raise RaycastError(f"raycast: {math.prod(lead)} rays (at most {MAX_RAYS})")
    return rays_o.detach().reshape(-1, 3).contiguous(), rays_d.detach().reshape(-1, 3).contiguous(), lead


# ---- the twin -----------------------------------------------------------------------------------------------------------------------------------------------

def _lerp(a, b, f):
    return a + f * (b - a)


def _tri(v, f):
    """v (M, 8) float64 corners (n = x | y << 1 | z << 2), f (M, 3): lrt_raycast_math.h's rc_tri, the same order."""
    c00, c10 = _lerp(v[:, 0], v[:, 1], f[:, 0]), _lerp(v[:, 2], v[:, 3], f[:, 0])
    c01, c11 = _lerp(v[:, 4], v[:, 5], f[:, 0]), _lerp(v[:, 6], v[:, 7], f[:, 0])
    return _lerp(_lerp(c00, c10, f[:, 1]), _lerp(c01, c11, f[:, 1]), f[:, 2])


CORNER = np.array([[n & 1, n >> 1 & 1, n >> 2 & 1] for n in range(8)], np.int64)


@torch.no_grad()
def raycast_reference(grid, rays_o, rays_d, *, min_weight=1, step=None, far_step=None, min_depth=0.0, max_depth=80.0, samples=False):
    """The numpy float64 twin of ``raycast`` (lrt_raycast_math.h's rc_ray), vectorised over the rays that are still marching; CPU tensors out.
    The rays may lie on any device."""
    mw, step, far, min_depth, max_depth = params(grid, min_weight, step, far_step, min_depth, max_depth)
    if not (torch.is_tensor(rays_o) and torch.is_tensor(rays_d) and rays_o.shape == rays_d.shape and rays_o.shape[-1:] == (3,)
            and rays_o.dtype == torch.float32 and rays_d.dtype == torch.float32):
        raise RaycastError("raycast: rays_o and rays_d must be float32 (..., 3) tensors of one shape")
    lead = tuple(rays_o.shape[:-1])
    ro = rays_o.detach().cpu().numpy().reshape(-1, 3)
    rd = rays_d.detach().cpu().numpy().reshape(-1, 3)
    N = ro.shape[0]
    depth = np.zeros(N, np.float32)
    hit = np.zeros(N, bool)
    inten = np.zeros(N, np.float32)
    ns = np.zeros(N, np.int32)
    X, Y, Z = grid.dims
    n = np.array([X, Y, Z], np.int64)
    has_int = grid.intensity is not None
    out = lambda: Raycast(depth=torch.from_numpy(depth.reshape(lead)), hit=torch.from_numpy(hit.reshape(lead)),
                          intensity=torch.from_numpy(inten.reshape(lead)) if has_int else None,
                          samples=torch.from_numpy(ns.reshape(lead)) if samples else None)
    if min(X, Y, Z) < 2 or N == 0:
        return out()
    voxel = float(grid.voxel)
    ts = grid.tsdf.detach().cpu().numpy().reshape(-1)
    wt = grid.weight.detach().cpu().numpy().reshape(-1)
    it = grid.intensity.detach().cpu().numpy().reshape(-1) if has_int else None
    cen = [mesh.centres(voxel, int(m)).astype(np.float64) for m in (X, Y, Z)]
    stride = np.array([Y * Z, Z, 1], np.int64)
    coff = CORNER @ stride                                                     # (8,) the corners' offsets from the cell's first voxel
    with np.errstate(invalid="ignore", over="ignore"):
        fin = np.isfinite(ro).all(1) & np.isfinite(rd).all(1)
        o = ro.astype(np.float64) - np.asarray(grid.origin, np.float64)[None]
        d = rd.astype(np.float64)
        nrm = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    live = fin & (nrm > 0.0)
    idx = np.nonzero(live)[0]
    o, d, nrm = o[idx], d[idx], nrm[idx]
    u = d / nrm[:, None]
    tin = np.full(idx.size, min_depth)
    tout = np.full(idx.size, max_depth)
    inside = np.ones(idx.size, bool)
    for a in range(3):
        c0, c1 = cen[a][0], cen[a][-1]
        z = u[:, a] == 0.0
        inside &= ~z | ((c0 <= o[:, a]) & (o[:, a] <= c1))
        with np.errstate(divide="ignore", invalid="ignore"):
            t1, t2 = (c0 - o[:, a]) / u[:, a], (c1 - o[:, a]) / u[:, a]
        lo, hi = np.where(t1 < t2, t1, t2), np.where(t1 < t2, t2, t1)
        tin = np.where(z, tin, np.where(lo > tin, lo, tin))
        tout = np.where(z, tout, np.where(hi < tout, hi, tout))
    keep = inside
    idx, o, u, t, tout = idx[keep], o[keep], u[keep], tin[keep], tout[keep]
    M = idx.size
    kp = np.zeros(M, bool)
    tp, Dp = np.zeros(M), np.zeros(M)
    cp, fp = np.zeros((M, 3), np.int64), np.zeros((M, 3))
    cnt = np.zeros(M, np.int32)
    act = np.arange(M)
    while True:
        act = act[t[act] <= tout[act]]
        if act.size == 0:
            break
        p = o[act] + t[act, None] * u[act]
        fi = np.floor(p / voxel - 0.5)
        hi = (n - 2)[None].astype(np.float64)
        c = np.where(fi > 0.0, np.where(fi > hi, hi, fi), 0.0).astype(np.int64)
        ca = np.stack([cen[a][c[:, a]] for a in range(3)], 1)
        cb = np.stack([cen[a][c[:, a] + 1] for a in range(3)], 1)
        f = (p - ca) / (cb - ca)
        f = np.where(f < 0.0, 0.0, np.where(f > 1.0, 1.0, f))
        cnt[act] += 1
        base = c @ stride
        vi = base[:, None] + coff[None]
        v = ts[vi]
        known = (wt[vi] >= mw).all(1)
        ones = (v == np.float32(1.0)).all(1)
        D = np.zeros(act.size)
        D[known] = _tri(v[known].astype(np.float64), f[known])
        crossing = known & kp[act] & (Dp[act] > 0.0) & (D <= 0.0)
        if crossing.any():
            k = act[crossing]
            w = Dp[k] / (Dp[k] - D[crossing])
            r = idx[k]
            depth[r] = (tp[k] + (t[k] - tp[k]) * w).astype(np.float32)
            hit[r] = True
            if has_int:
                ia = it[(cp[k] @ stride)[:, None] + coff[None]].astype(np.float64)
                ib = it[base[crossing][:, None] + coff[None]].astype(np.float64)
                Ip, Ik = _tri(ia, fp[k]), _tri(ib, f[crossing])
                inten[r] = (Ip + (Ik - Ip) * w).astype(np.float32)
            ns[r] = cnt[k]
        s = np.where(known & ones, far, step)
        kp[act] = known
        upd = known & ~crossing
        tp[act[upd]], Dp[act[upd]] = t[act[upd]], D[upd]
        cp[act[upd]], fp[act[upd]] = c[upd], f[upd]
        t[act] = t[act] + s
        t[act[crossing]] = math.inf                                            # a hit ends the ray
    done = ~hit[idx]
    ns[idx[done]] = cnt[done]
    return out()


# ---- the device ---------------------------------------------------------------------------------------------------------------------------------------------

def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


@torch.no_grad()
def raycast(grid, rays_o, rays_d, *, min_weight=1, step=None, far_step=None, min_depth=0.0, max_depth=80.0, samples=False):
    """Cast the rays ``(..., 3)`` float32 (world frame, on the grid's device) through ``grid`` (see the module text).  One launch on a HIP device
    (none without rays); a CPU grid goes to ``raycast_reference``."""
    mw, step, far, min_depth, max_depth = params(grid, min_weight, step, far_step, min_depth, max_depth)
    o, d, lead = _rays(grid, rays_o, rays_d)
    if grid.device.type != "cuda":
        return raycast_reference(grid, rays_o, rays_d, min_weight=mw, step=step, far_step=far, min_depth=min_depth, max_depth=max_depth,
                                 samples=samples)
    lib = load()
    dev = grid.device
    for name in ("tsdf", "weight") + (("intensity",) if grid.intensity is not None else ()):
        a = getattr(grid, name)
        if not a.is_contiguous() or tuple(a.shape) != tuple(grid.dims):
            raise RaycastError(f"raycast: the grid's {name} must be a contiguous {tuple(grid.dims)} tensor")
    N = o.shape[0]
    depth = torch.empty(N, dtype=torch.float32, device=dev)
    hit = torch.empty(N, dtype=torch.uint8, device=dev)
    inten = torch.empty(N, dtype=torch.float32, device=dev) if grid.intensity is not None else None
    ns = torch.empty(N, dtype=torch.int32, device=dev) if samples else None
    X, Y, Z = grid.dims
    og = np.asarray(grid.origin, np.float64)
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
    with torch.cuda.device(dev):
        rc = lib.lrt_raycast(dev.index, X, Y, Z, float(grid.voxel), float(grid.trunc), float(og[0]), float(og[1]), float(og[2]), grid.tsdf.data_ptr(),
                             grid.weight.data_ptr(), None if grid.intensity is None else grid.intensity.data_ptr(), mw, N, ptr(o), ptr(d), step, far,
                             min_depth, max_depth, ptr(depth), ptr(hit), ptr(inten), ptr(ns), _stream(dev))
    if rc != 0:
        raise RaycastError(f"lrt_raycast failed ({rc}): {lib.lrt_raycast_last_error().decode()}")
    return Raycast(depth=depth.reshape(lead), hit=hit.view(torch.bool).reshape(lead), intensity=None if inten is None else inten.reshape(lead),
                   samples=None if ns is None else ns.reshape(lead))


# ---- frames -------------------------------------------------------------------------------------------------------------------------------------------------

def render_frame(grid, sensor, frame, **kw):
    """(render {"depth", "intensity", "raydrop"} each (H, W, 1), the Raycast) of one frame's own rays ``sensor.rays[frame]``, which are moved to
    the grid's device when they lie elsewhere."""
    o, d = sensor.rays[frame]
    r = raycast(grid, o.to(grid.device), d.to(grid.device), **kw)
    inten = r.intensity if r.intensity is not None else torch.zeros_like(r.depth)
    return {"depth": r.depth[..., None], "intensity": inten[..., None], "raydrop": (1.0 - r.hit.float())[..., None]}, r


def render_frames(grid, sensor, frame_ids, **kw):
    """``{frame: {"depth", "intensity", "raydrop"}}`` in ``evaluation.render_frames``' layout (each (H, W, 1)); raydrop = 1 - hit, intensity 0
    for a grid without one.  ``kw``: ``raycast``'s options."""
    return {f: render_frame(grid, sensor, f, **kw)[0] for f in frame_ids}


# ---- the command line ---------------------------------------------------------------------------------------------------------------------------------------

def main(argv=None):
    from . import beams as beams_mod
    from . import metrics
    from . import sequence as sequence_mod
    ap = argparse.ArgumentParser(prog="python -m lidar_rt_amd.raycast", description=(
        "A map baseline: fuse a sequence's frames into a TSDF grid (lidar_rt_amd.mesh), cast the chosen frames' own rays through it and score the "
        "range images with evaluate's metric set.  The output's \"mean\" and \"per_frame\" have exactly evaluate's keys."))
    ap.add_argument("--data", required=True, help="a sequence directory (lidar_rt_amd.sequence)")
    ap.add_argument("--fuse", choices=("train", "all"), default="train", help="the frames fused into the grid")
    ap.add_argument("--frames", choices=("test", "train", "all"), default="test", help="the frames cast (test falls back to train without test frames)")
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--trunc", type=float, default=None, help="metres (default: 3 voxels)")
    ap.add_argument("--min-weight", type=int, default=1)
    ap.add_argument("--step", type=float, default=None, help="metres (default: half a voxel)")
    ap.add_argument("--far-step", type=float, default=None, help="metres, below trunc (default: trunc - step)")
    ap.add_argument("--max-depth", type=float, default=80.0)
    ap.add_argument("--bounds", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("--max-voxels", type=int, default=mesh.DEFAULT_MAX_VOXELS, help="a larger grid is refused, never coarsened")
    ap.add_argument("--batch", type=int, default=16, help="frames per integrate call")
    ap.add_argument("--static-only", action="store_true", help="fuse without the returns inside a tracking box present in their frame")
    ap.add_argument("--sweep", choices=("off", "stored"), default="off", help="cast with one pose per column (each frame's stored twist), as evaluate --sweep")
    ap.add_argument("--fuse-sweep", choices=("off", "stored"), default="off",
                    help="stored: fuse under the sweep model with each fused frame's stored twist (sweep_fuse.integrate_sweep); --sweep does not imply it")
    ap.add_argument("--sweep-ref", type=float, default=0.5, help="the part of the sweep at which a frame's pose holds, for frames that store no column times")
    ap.add_argument("--sweep-direction", choices=("cw", "ccw"), default="cw", help="cw = time rises with the column index, for frames that store no column times")
    ap.add_argument("--beams", default=None, metavar="FILE", help="cast through a beam table (lidar_rt_amd.beams), as evaluate --beams")
    ap.add_argument("--raydrop-ratio", type=float, default=0.4)
    ap.add_argument("--use-gt-mask", action="store_true", help="mask the renders with the ground-truth ray-hit mask instead of the hit mask")
    ap.add_argument("--sequence", default=None, metavar="OUT", help="also write the renders as a sequence directory (mask = hit)")
    ap.add_argument("--out", default="raycast.json")
    ap.add_argument("--device", default="cuda", help="cuda (the libraries) or cpu (the numpy twins and frame_metrics_reference)")
    a = ap.parse_args(argv)
    t0 = time.perf_counter()
    voxel = float(a.voxel)
    trunc = 3.0 * voxel if a.trunc is None else float(a.trunc)
    if a.batch < 1:
        raise SystemExit("--batch must be at least 1")
    dev = torch.device(a.device)
    try:
        meta, frames, inc = mesh.load_frames(a.data, a.fuse, a.static_only, a.fuse_sweep, a.sweep_ref, a.sweep_direction)
    except mesh.MeshError as e:
        if a.fuse_sweep == "off":
            raise
        raise SystemExit(str(e)) from None
    origin, dims = mesh.grid_bounds(frames, voxel, trunc, a.bounds)
    nvox = math.prod(dims)
    if nvox > a.max_voxels:
        raise SystemExit(f"the grid needs {dims[0]} x {dims[1]} x {dims[2]} = {nvox} voxels at --voxel {voxel}, more than --max-voxels {a.max_voxels}: "
                         "raise --max-voxels, give --bounds or a coarser --voxel")
    grid = mesh.TsdfGrid(origin, voxel, dims, trunc, dev, intensity=True)
    kw = dict(min_weight=a.min_weight, step=a.step, far_step=a.far_step, max_depth=a.max_depth)
    try:
        p = params(grid, **kw)
    except RaycastError as e:
        raise SystemExit(str(e)) from None
    s2e = meta.get("sensor2ego")
    fuse_counts = mesh.fuse_frames(grid, frames, inc, meta, a.batch, a.max_depth, a.fuse_sweep)
    # the rays are formed on the host whatever the device: a device's sin and cos may differ from the host's in the last bit, and with the same
    # rays and the same grid the cast writes the same bytes on both
    host = torch.device("cpu")
    seq = sequence_mod.load_sequence(a.data, host, sweep=a.sweep, sweep_ref=a.sweep_ref, sweep_direction=a.sweep_direction)
    if a.beams:
        beam_rows = int(next(iter(seq.frames.depth.values())).shape[0])
        beams_mod.apply_table(seq.frames, beams_mod.load_table(a.beams, beam_rows, host))
    sensor = seq.frames
    ids = {"test": seq.test_frames or seq.train_frames, "train": seq.train_frames, "all": sorted(set(seq.train_frames) | set(seq.test_frames))}[a.frames]
    ids = [int(f) for f in ids]
    renders, hits, spr, smax, nrays = {}, 0, 0, 0, 0
    rows = []
    for f in ids:
        renders[f], r = render_frame(grid, sensor, f, samples=True, **kw)
        hits += int(r.hit.sum())
        spr += int(r.samples.sum(dtype=torch.int64))
        smax = max(smax, int(r.samples.max()) if r.samples.numel() else 0)
        nrays += r.hit.numel()
        args = (renders[f], sensor.get_depth(f).to(dev), sensor.get_intensity(f).to(dev), sensor.get_mask(f).to(dev))
        mk = dict(rays=tuple(x.to(dev) for x in sensor.get_range_rays(f)), raydrop_ratio=a.raydrop_ratio, use_gt_mask=a.use_gt_mask, max_depth=a.max_depth)
        rows.append(metrics.frame_metrics(*args, **mk) if dev.type == "cuda" else metrics.frame_metrics_reference(*args, **mk))
    per_frame = {}
    if ids:
        table = torch.stack([r.double() for r in rows]).cpu().tolist()          # one transfer
        for f, row in zip(ids, table):
            for (g, m), v in zip(metrics.ROW, row):
                if (g, m) not in metrics.EXTRAS:
                    per_frame.setdefault(str(f), {}).setdefault(g, {})[m] = float(v)
    mean = {}
    for g, m in ([gm for gm in metrics.ROW if gm not in metrics.EXTRAS] if ids else []):
        xs = [per_frame[str(f)][g][m] for f in ids if per_frame[str(f)][g][m] == per_frame[str(f)][g][m]]
        mean.setdefault(g, {})[m] = sum(xs) / len(xs) if xs else float("nan")
    if a.sequence:
        out_rows = []
        for f in ids:
            hit = renders[f]["raydrop"].squeeze(-1) == 0
            zero = lambda x: torch.where(hit, x, torch.zeros_like(x))
            inc_f, s2w, _, _ = sensor.pose_meta[f]
            sw = sensor.sweep_meta.get(f)
            out_rows.append({"id": f, "depth": zero(renders[f]["depth"].squeeze(-1)), "intensity": zero(renders[f]["intensity"].squeeze(-1)), "mask": hit,
                             "inclination": np.asarray(inc_f, np.float32), "sensor2world": s2w.detach().cpu().numpy().astype(np.float64),
                             **({"twist": sw[0], "tau": sw[1]} if sw is not None else {})})
        sequence_mod.write_sequence(a.sequence, out_rows, data_type=meta["data_type"], extent=float(meta.get("extent", 1.0)), sensor2ego=s2e)
    report = {"frames": ids, "mean": mean, "per_frame": per_frame,
              "grid": {"origin": [float(x) for x in origin], "voxel": voxel, "dims": list(dims), "trunc": trunc, "observed_voxels": int((grid.weight > 0).sum())},
              "fused_frames": [f["id"] for f in frames], "fuse_sweep": {"mode": a.fuse_sweep, **(fuse_counts or {})},
              "cast": {"min_weight": p[0], "step": p[1], "far_step": p[2], "max_depth": p[4], "rays": nrays, "hit_fraction": hits / nrays if nrays else 0.0,
                       "samples_per_ray": {"mean": spr / nrays if nrays else 0.0, "max": smax}},
              "seconds": round(time.perf_counter() - t0, 3), "args": vars(a)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps({"mean": mean, "hit_fraction": report["cast"]["hit_fraction"], "seconds": report["seconds"]}))
    return report


if __name__ == "__main__":
    main(sys.argv[1:])
