"""``python -m lidar_rt_amd.simulate --data DIR --ckpt CKPT --out OUT``: scans of a trained scene -- what a LiDAR re-simulator is for.

Loads the sequence and the checkpoint exactly as ``python -m lidar_rt_amd.evaluate`` does (``--boxes``, ``--unet*``, ``--sweep*``, ``--frames``,
``--max-frames``, ``--raydrop-ratio`` included), renders the chosen frames through ``evaluation.render_frames``, turns every render into a point
cloud with ``unproject.points_from_range_images`` and writes

    OUT/<id:06d>.bin     KITTI float32 quadruples [x, y, z, intensity] (``--format npy``: ``.npy``; ``--fields xyzirt``: (N, 6) with the ring and the
                         column's firing time in sweeps)
    OUT/poses.txt        id and the 12 numbers of the sensor-to-world pose, readable by ``python -m lidar_rt_amd.ingest --poses``
    OUT/simulate.json    the arguments, the edits, the five counts of every frame (``unproject.COUNT_NAMES``), twists and column times when sweeping

``--sequence DIR`` also writes the renders themselves as a sequence directory (``sequence.write_sequence``; mask = the kept pixels).

A sensor the data never had -- the rays come from ``RangeFrames.range_rays`` / ``sweep.sweep_rays``: ``--height H --width W``; ``--inclination A B``
or ``--inclination-table FILE`` (text, one angle per row [rad]); ``--mount x y z roll pitch yaw`` (``sensor2world' = sensor2world @ M``, metres and
radians); ``--poses FILE`` (``ingest``'s pose-file format) replaces the poses of the ids it lists -- the ids stay, the actors' boxes are keyed by them.

Edits -- host-side changes of the asset list and of the ``TrackingBox.frame`` tables before rendering, the checkpoint file is not written to:
``--remove-actor A ...``; ``--move-actor A dx dy dz yaw_deg`` (repeatable): a world-frame offset of the box centre and a rotation about world z in
every frame, composed on the left of the stored pose; ``--only {background,actors}``: the reference renderer's ``decomp``.  Actor ``A`` is the
sequence's ``actor_<A>``: asset ``A + 1``.

The frame of the points, ``--frame``: ``world`` (no transform); ``sensor`` (the inverse of the frame's pose -- with ``--sweep`` this is the motion
COMPENSATED cloud, what KITTI, nuScenes and Waymo publish); ``raw`` (every point in the pose of its own column, ``(P Exp(tau[w] xi))^-1``: what a
spinning sensor's driver emits; needs ``--sweep``).  The tables are formed on the host in float64 from the same pose, twist and ``tau`` that made
the rays, and applied in float64 by the operator (``include/lrt_unproject.h``).  The rays of a moving sensor start at their columns' origins
rounded to float32 (up to 0.06 mm off, 1.6 km from the world's origin); the tables move every column's points onto its exact origin first
(``column_transforms(origins=)``), so a point lies at its rendered range from where the pose file says its column was.  Under ``--sweep`` the
``sensor`` and ``raw`` clouds therefore describe world points up to that rounding away from the ``world`` cloud's; ``--no-origin-shift`` gives the
plain inverses of pose, twist and ``tau`` instead (the same world points as ``world``; the ranges recomputed from them are then off by the
rounding).  A static sensor's clouds are not touched by any of this.

The output closes the loop: ``python -m lidar_rt_amd.ingest --points OUT --poses OUT/poses.txt`` with ``--frame sensor`` clouds, the same height,
width, inclination and data type (and ``--sweep --compensated`` for a moving sensor) rebuilds the range images that were rendered.

Everything after the render -- ``clouds_from_renders``, ``apply_edits``, ``column_transforms``, ``write_clouds`` -- runs on CPU tensors too.
"""
from __future__ import annotations

import argparse
import copy
import json
import math
import os
import sys
from types import SimpleNamespace
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import unproject

SIMULATE_FORMAT = "lidar-rt-amd-simulate/1"
FRAMES = ("world", "sensor", "raw")
# the boolean-mask expression or the HIP operator for world-frame clouds on a HIP device: the faster one at 64 x 2048 (profiles/unproject.md);
# the float64 frames (sensor, raw) have no torch equivalent and always take the operator
DEFAULT_WORLD_BACKEND = "hip"


class SimulateError(ValueError):
    pass


# ---- edits ---------------------------------------------------------------------------------------------------------------------------------------------------

class _MovedBox:
    """A tracking box with another per-frame table; what the loops read of one (``sequence.TrackingBox``)."""

    def __init__(self, box, frame: dict):
        self.min_xyz, self.max_xyz = box.min_xyz, box.max_xyz
        self.frame = frame
        self.twist = getattr(box, "twist", {})       # the body twists are the box's own: a move multiplies on the world side, A' Exp(s eta) = M A Exp(s eta)


def _quat_mul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Hamilton product of (w, x, y, z) quaternions (..., 4)."""
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def apply_edits(assets: Sequence, remove_actor: Sequence[int] = (), move_actor: Sequence[Sequence[float]] = (), only: Optional[str] = None):
    """(assets', decomp, report): the asset list with the removed actors left out and the moved actors' boxes replaced (shallow copies: the
    parameters are shared, the given assets and their tables are not changed); ``decomp`` is ``renderer.raytracing``'s for ``only``.  Actor ``A``
    is ``assets[A + 1]``; ``move_actor`` rows are ``(A, dx, dy, dz, yaw_deg)``: in every frame ``t' = t + (dx, dy, dz)``, ``q' = q_z(yaw) q``."""
    assets = list(assets)
    n = len(assets) - 1
    if only not in (None, "background", "actors"):
        raise SimulateError(f"simulate: only {only!r} (background or actors)")

    def actor(a, what):
        if not (float(a) == int(a) and 0 <= int(a) < n):
            raise SimulateError(f"simulate: {what} {a}: " + (f"the scene's actors are 0 .. {n - 1}" if n else "the scene has no actors"))
        return int(a)

    removed = sorted({actor(a, "--remove-actor") for a in remove_actor})
    moves = []
    for row in move_actor:
        if len(row) != 5:
            raise SimulateError(f"simulate: --move-actor takes A dx dy dz yaw_deg ({len(row)} values given)")
        a = actor(row[0], "--move-actor")
        if a in removed:
            raise SimulateError(f"simulate: actor {a} is both removed and moved")
        dx, dy, dz, yaw = (float(x) for x in row[1:])
        if not all(math.isfinite(x) for x in (dx, dy, dz, yaw)):
            raise SimulateError(f"simulate: --move-actor {a}: a non-finite offset or angle")
        moves.append((a, dx, dy, dz, yaw))
    for a, dx, dy, dz, yaw in moves:                                     # in the order given: a second move of one actor composes on the first
        asset = copy.copy(assets[a + 1])
        box = asset.bounding_box
        if box is None:
            raise SimulateError(f"simulate: actor {a} has no tracking box to move")
        half = 0.5 * math.radians(yaw)
        table = {}
        for ts in box.frame.keys():
            t, q = box.frame[ts][0], box.frame[ts][1]
            d = torch.tensor([dx, dy, dz], dtype=t.dtype, device=t.device)
            qz = torch.tensor([math.cos(half), 0.0, 0.0, math.sin(half)], dtype=q.dtype, device=q.device)
            table[ts] = (t + d, _quat_mul(qz.expand_as(q), q)) + tuple(box.frame[ts][2:])
        asset.bounding_box = _MovedBox(box, table)
        assets[a + 1] = asset
    out = [g for i, g in enumerate(assets) if i == 0 or (i - 1) not in removed]
    decomp = {None: False, "background": "background", "actors": "object"}[only]
    if only == "actors" and len(out) < 2:
        raise SimulateError("simulate: --only actors, and no actor is left")
    report = {"removed": removed, "moved": [{"actor": a, "offset": [dx, dy, dz], "yaw_deg": yaw} for a, dx, dy, dz, yaw in moves], "only": only}
    return out, decomp, report


# ---- the frame of the points -----------------------------------------------------------------------------------------------------------------------------------

def _pose64(pose) -> np.ndarray:
    p = pose.detach().cpu().numpy() if torch.is_tensor(pose) else np.asarray(pose)
    p = np.asarray(p, np.float64)
    if p.shape not in ((3, 4), (4, 4)):
        raise SimulateError(f"simulate: a (3, 4) or (4, 4) pose (it is {p.shape})")
    return p[:3]


def column_transforms(frame: str, pose, twist=None, tau=None, origins=None) -> Optional[np.ndarray]:
    """``world2out`` of one frame for ``unproject.points_from_range_images``, host float64: ``world``: None; ``sensor``: ``pose^-1`` (3, 4);
    ``raw``: ``(pose Exp(tau[w] twist))^-1`` per column (W, 3, 4), with ``sweep.column_poses_reference``'s exponential.  Give the pose, the twist
    and the column times that made the rays (their float32 values).

    ``origins`` (W, 3): the origins the rays of a MOVING sensor were actually cast from -- the columns' origins rounded to float32, 0.1 mm off
    a kilometre from the world's origin.  The range of a render is measured from there, so with them every column's points are moved by
    (exact origin - ray origin) first: the point lies at its rendered range from its column's exact origin, and ``sensor`` becomes a table per
    column too.  A static sensor's ray origin is its pose's translation; nothing is to correct."""
    if frame not in FRAMES:
        raise SimulateError(f"simulate: frame {frame!r} ({', '.join(FRAMES)})")
    if frame == "world":
        return None
    P = _pose64(pose)
    moving = twist is not None and tau is not None
    if frame == "raw" and not moving:
        raise SimulateError("simulate: --frame raw needs a moving sensor (--sweep): every point in the pose of its own column")

    def inv(R, t):
        """The inverse of x -> R x + t as (..., 3, 4).  A true inverse, not the transpose: a pose held in float32 is orthonormal to 1e-7 only,
        and the table has to undo what made the rays."""
        Ri = np.linalg.inv(R)
        return np.concatenate([Ri, -(Ri @ t[..., None])], -1)

    if not moving or (frame == "sensor" and origins is None):
        return inv(P[:, :3], P[:, 3])
    from . import sweep
    host = lambda x: np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, np.float64)
    Rc, tc = sweep.column_poses_reference(torch.as_tensor(P)[None], torch.as_tensor(host(twist).reshape(1, 6)), torch.as_tensor(host(tau).reshape(-1)))
    Rc, tc = Rc[0].numpy(), tc[0].numpy()
    W = tc.shape[0]
    A = inv(Rc, tc) if frame == "raw" else np.broadcast_to(inv(P[:, :3], P[:, 3]), (W, 3, 4)).copy()
    if origins is not None:
        o = host(origins).reshape(-1, 3)
        if o.shape[0] != W:
            raise SimulateError(f"simulate: {o.shape[0]} ray origins for {W} columns")
        A[:, :, 3] += (A[:, :, :3] @ (tc - o)[..., None])[..., 0]
    return np.ascontiguousarray(A)


# ---- renders into clouds -----------------------------------------------------------------------------------------------------------------------------------------

def clouds_from_renders(renders: Dict, sensor, frame_ids: Sequence, raydrop_ratio: float = 0.4, world2out=None, min_depth: float = 0.0,
                        max_depth: float = unproject.FLT_MAX, backend: Optional[str] = None) -> unproject.PointClouds:
    """The clouds of ``evaluation.render_frames``'s renders, all frames in one ``PointClouds``.  ``world2out``: None, or one table per frame in the
    order of ``frame_ids`` ((3, 4) each, or (W, 3, 4) each).  ``backend``: "hip" -- ``unproject.points_from_range_images`` (on CPU tensors its
    twin); "torch" -- the boolean-mask expression per frame, world frame only: the same bits, a host wait per frame; None: "hip" wherever a
    transform is given or the tensors are on the CPU, else ``DEFAULT_WORLD_BACKEND``."""
    frame_ids = list(frame_ids)
    if not frame_ids:
        raise SimulateError("simulate: no frame to turn into a cloud")
    st = lambda k: torch.stack([renders[f][k].squeeze(-1) for f in frame_ids]).float().contiguous()
    depth, intensity, raydrop = st("depth"), st("intensity"), st("raydrop")
    o = torch.stack([sensor.get_range_rays(f)[0] for f in frame_ids]).contiguous()
    d = torch.stack([sensor.get_range_rays(f)[1] for f in frame_ids]).contiguous()
    T = None if world2out is None else np.stack([np.asarray(t, np.float64) for t in world2out])
    if backend is None:
        backend = "hip" if (T is not None or depth.device.type != "cuda") else DEFAULT_WORLD_BACKEND
    if backend not in ("hip", "torch"):
        raise SimulateError(f"simulate: backend {backend!r} (hip or torch)")
    if backend == "hip":
        return unproject.points_from_range_images(depth, o, d, intensity=intensity, raydrop=raydrop, raydrop_ratio=raydrop_ratio, world2out=T,
                                                  min_depth=min_depth, max_depth=max_depth)
    if T is not None:
        raise SimulateError("simulate: the torch backend forms world-frame clouds only (the float64 transform is the operator's)")
    F, H, W = depth.shape
    pts, pix, counts = [], [], []
    ratio = float(np.float32(raydrop_ratio))
    for k in range(F):
        r = depth[k]
        finite = torch.isfinite(r) & torch.isfinite(o[k]).all(-1) & torch.isfinite(d[k]).all(-1)
        masked = finite & ~(raydrop[k] < ratio)
        keep = finite & ~masked & (r.double() > min_depth) & (r.double() <= max_depth)
        flat = keep.reshape(-1)
        p = (o[k] + d[k] * r.reshape(H, W, 1)).reshape(-1, 3)[flat]          # RangeFrames.inverse_projection_with_range
        pts.append(torch.cat([p, intensity[k].reshape(-1)[flat][:, None]], 1))
        pix.append(torch.nonzero(flat).squeeze(1).to(torch.int32))
        n_inv, n_msk, n_pts = int((~finite).sum()), int(masked.sum()), int(flat.sum())
        counts.append([H * W, n_inv, n_msk, H * W - n_inv - n_msk - n_pts, n_pts])
    counts = torch.tensor(counts, dtype=torch.int64, device=depth.device)
    offsets = torch.cat([counts.new_zeros(1), counts[:, 4].cumsum(0)])
    return unproject.PointClouds(points=torch.cat(pts), pixel=torch.cat(pix), offsets=offsets, counts=counts)


# ---- files -----------------------------------------------------------------------------------------------------------------------------------------------------

def write_poses(path: str, poses: Dict[int, np.ndarray]) -> None:
    """Text rows of an id and the 12 numbers of a 3 x 4 sensor-to-world matrix: ``ingest.read_poses`` reads them back exactly."""
    with open(path, "w") as f:
        for fid in sorted(poses):
            f.write(f"{int(fid)} " + " ".join(repr(float(x)) for x in _pose64(poses[fid]).reshape(-1)) + "\n")


def write_clouds(out_dir: str, frame_ids: Sequence[int], clouds: unproject.PointClouds, W: int, poses: Optional[Dict[int, np.ndarray]] = None,
                 fmt: str = "bin", fields: str = "xyzi", tau: Optional[Dict[int, np.ndarray]] = None) -> list:
    """One file per frame, ``OUT/<id:06d>.bin`` (float32 rows) or ``.npy``; ``fields``: "xyzi" (N, 4) or "xyzirt" (N, 6): ring = pixel // W and
    t = tau[id][pixel % W], the column's firing time in sweeps (0 without ``tau``).  ``poses``: also ``OUT/poses.txt``.  Returns the paths."""
    if fmt not in ("bin", "npy"):
        raise SimulateError(f"simulate: format {fmt!r} (bin or npy)")
    if fields not in ("xyzi", "xyzirt"):
        raise SimulateError(f"simulate: fields {fields!r} (xyzi or xyzirt)")
    frame_ids = [int(f) for f in frame_ids]
    off = clouds.offsets.cpu().tolist()                                      # the one host wait
    if len(off) != len(frame_ids) + 1:
        raise SimulateError(f"simulate: {len(frame_ids)} frame ids for the clouds of {len(off) - 1} frames")
    pts, pix = clouds.points[:off[-1]].cpu().numpy(), clouds.pixel[:off[-1]].cpu().numpy()
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for k, fid in enumerate(frame_ids):
        a = pts[off[k]:off[k + 1]]
        if fields == "xyzirt":
            px = pix[off[k]:off[k + 1]]
            t = np.zeros(px.shape, np.float32) if tau is None else np.asarray(tau[fid], np.float32).reshape(-1)[px % W]
            a = np.concatenate([a, (px // W).astype(np.float32)[:, None], t[:, None]], 1)
        a = np.ascontiguousarray(a, np.float32)
        p = os.path.join(out_dir, f"{fid:06d}.{fmt}")
        if fmt == "npy":
            np.save(p, a)
        else:
            a.tofile(p)
        paths.append(p)
    if poses is not None:
        write_poses(os.path.join(out_dir, "poses.txt"), {f: poses[f] for f in frame_ids})
    return paths


# ---- the sensor ------------------------------------------------------------------------------------------------------------------------------------------------

def mount_matrix(mount: Sequence[float]) -> np.ndarray:
    """(4, 4) float64 of ``x y z roll pitch yaw`` [m, rad]: R = Rz(yaw) Ry(pitch) Rx(roll)."""
    if len(mount) != 6 or not all(math.isfinite(float(x)) for x in mount):
        raise SimulateError(f"simulate: --mount takes x y z roll pitch yaw (finite), it is {list(mount)}")
    x, y, z, roll, pitch, yaw = (float(v) for v in mount)
    cr, sr, cp, sp, cy, sy = math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch), math.cos(yaw), math.sin(yaw)
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = Rz @ Ry @ Rx, (x, y, z)
    return M


def read_inclination_table(path: str, H: int) -> list:
    t = np.loadtxt(path, dtype=np.float64).reshape(-1)
    return check_inclination(t.tolist(), H, path)


def check_inclination(inc, H: int, what: str = "--inclination") -> list:
    inc = [float(x) for x in inc]
    if len(inc) != 2 and len(inc) != H:
        raise SimulateError(f"simulate: {what} holds {len(inc)} angles: two bounds, or a beam table of one per row ({H})")
    if len(inc) > 2 and H < 3:
        raise SimulateError(f"simulate: a beam table needs at least 3 rows ({H})")
    d = np.diff(inc)
    if not np.all(np.isfinite(inc)) or not (np.all(d > 0) or np.all(d < 0)):
        raise SimulateError(f"simulate: {what}: the angles must be finite and strictly monotonic")
    return inc


def build_sensor(seq, frame_ids: Sequence[int], height=None, width=None, inclination=None, mount=None, poses: Optional[dict] = None, sweep_ref: float = 0.5,
                 sweep_direction: str = "cw", sweep_fraction: float = 1.0):
    """The ``RangeFrames`` to render: the sequence's own when nothing is asked for, else one ray grid per frame id from the new height, width,
    inclination, mount and poses (``RangeFrames.add_range_image``; images of zeros stand in for the data the new sensor never had).  With a sweep
    the twists follow the sensor: re-derived from the new trajectory for ``sweep="poses"``, carried into the mounted frame
    (``xi' = Log(M^-1 Exp(xi) M)``) under a mount; another width takes ``sweep.column_times(W, sweep_ref, sweep_direction)``."""
    old = seq.frames
    unknown = sorted({int(k) for k in (poses or {})} - {int(f) for f in old.rays})
    if unknown:
        raise SimulateError(f"simulate: --poses lists ids the sequence does not have: {unknown}")
    if height is None and width is None and inclination is None and mount is None and not poses:
        return old
    from . import sweep as sweep_mod
    from .training import RangeFrames
    missing = [f for f in frame_ids if f not in old.pose_meta]
    if missing:
        raise SimulateError(f"simulate: frames {missing} carry no pose (a new sensor needs the sequence's range-image frames)")
    M = None if mount is None else mount_matrix(mount)
    new_pose = {int(k): np.asarray(v, np.float64).reshape(4, 4) for k, v in (poses or {}).items()}
    twists = {}
    if seq.sweep == "poses" and new_pose:
        traj = {int(f): new_pose.get(int(f), old.pose_meta[f][1].detach().cpu().numpy().astype(np.float64)) for f in old.pose_meta}
        twists = sweep_mod.twists_from_poses(traj, sweep_fraction)
    rf = RangeFrames()
    for f in frame_ids:
        inc0, s2w0, data_type, s2e = old.pose_meta[f]
        H0, W0 = old.depth[f].shape
        H, W = int(height or H0), int(width or W0)
        dev = old.depth[f].device
        if inclination is not None:
            inc = check_inclination(inclination, H)
        else:
            inc = [float(x) for x in inc0]
            if len(inc) > 2 and len(inc) != H:
                raise SimulateError(f"simulate: the sequence's beam table holds {len(inc)} angles, --height {H} needs its own (--inclination / --inclination-table)")
        P = new_pose.get(int(f), s2w0.detach().cpu().numpy().astype(np.float64))
        kw = {}
        if f in old.sweep_meta:
            xi, tau = old.sweep_meta[f]
            xi = np.asarray(twists[int(f)] if int(f) in twists else xi.detach().cpu().numpy(), np.float64).reshape(6)
            if M is not None:
                Re, te = sweep_mod._exp64(torch.as_tensor(xi)[None])
                E = np.eye(4)
                E[:3, :3], E[:3, 3] = Re[0].numpy(), te[0].numpy()
                xi = sweep_mod.se3_log(np.linalg.inv(M) @ E @ M)
            kw = {"twist": torch.as_tensor(xi.astype(np.float32)), "tau": tau if W == W0 else sweep_mod.column_times(W, sweep_ref, sweep_direction)}
        if M is not None:
            P = P @ M
        z = torch.zeros((H, W), dtype=torch.float32, device=dev)
        rf.add_range_image(f, z, z, torch.zeros((H, W), dtype=torch.bool, device=dev), inc if len(inc) > 2 else (inc[0], inc[1]),
                           torch.as_tensor(P.astype(np.float32), device=dev), data_type, s2e, **kw)
    return rf


# ---- the run ---------------------------------------------------------------------------------------------------------------------------------------------------

def simulate(data: str, ckpt: str, out: str, frames: str = "test", max_frames: int = 0, raydrop_ratio: float = 0.4, boxes: Optional[str] = None,
             unet: Optional[str] = None, unet_backend: Optional[str] = None, unet_no_spatial: bool = False, sweep: str = "off", sweep_ref: float = 0.5,
             sweep_direction: str = "cw", sweep_fraction: float = 1.0, height: Optional[int] = None, width: Optional[int] = None,
             inclination: Optional[Sequence[float]] = None, inclination_table: Optional[str] = None, mount: Optional[Sequence[float]] = None,
             poses: Optional[str] = None, remove_actor: Sequence[int] = (), move_actor: Sequence[Sequence[float]] = (), only: Optional[str] = None,
             frame: str = "world", fmt: str = "bin", fields: str = "xyzi", sequence_dir: Optional[str] = None, backend: Optional[str] = None,
             min_depth: float = 0.0, max_depth: Optional[float] = None, max_points: int = 2_000_000, seed: int = 0, device: int = 0,
             origin_shift: bool = True, actor_sweep: str = "off", actor_twists: Optional[str] = None, beams: Optional[str] = None) -> dict:
    """The run behind the command (see the module text); returns what ``OUT/simulate.json`` holds.  ``origin_shift=False``: the tables of a moving
    sensor are the plain inverses of pose, twist and ``tau`` (``column_transforms`` without ``origins``)."""
    from . import evaluate as evaluate_mod
    from . import evaluation, ingest
    from . import sequence as sequence_mod
    from . import training
    if frame not in FRAMES:
        raise SimulateError(f"simulate: frame {frame!r} ({', '.join(FRAMES)})")
    if frame == "raw" and sweep in (None, "off"):
        raise SimulateError("simulate: --frame raw needs a moving sensor (--sweep): every point in the pose of its own column")
    if inclination is not None and inclination_table is not None:
        raise SimulateError("simulate: --inclination and --inclination-table exclude each other")
    if (height is not None and height < 1) or (width is not None and width < 1):
        raise SimulateError(f"simulate: a sensor of {height} x {width} pixels")
    if actor_sweep not in ("off", "stored", "boxes"):
        raise SimulateError(f"simulate: actor_sweep {actor_sweep!r} (off, stored or boxes)")
    if actor_sweep != "off" and sweep in (None, "off"):
        raise SimulateError("simulate: --actor-sweep needs a moving sensor (--sweep): the instants are those of its columns")
    if actor_twists and actor_sweep == "off":
        raise SimulateError("simulate: --actor-twists needs --actor-sweep")
    if fmt not in ("bin", "npy") or fields not in ("xyzi", "xyzirt"):
        raise SimulateError(f"simulate: format {fmt!r} (bin or npy), fields {fields!r} (xyzi or xyzirt)")
    with open(os.path.join(data, "meta.json")) as fh:                       # the arguments are judged before the device is touched
        H_new = int(height or json.load(fh)["height"])
    if inclination_table is not None:
        inclination = read_inclination_table(inclination_table, H_new)
    elif inclination is not None:
        inclination = check_inclination(inclination, H_new)
    if not torch.cuda.is_available():
        raise SystemExit("lidar_rt_amd.simulate needs a HIP device (there is no CPU path for the render)")
    dev = torch.device("cuda", device)
    torch.cuda.set_device(dev)
    seq = sequence_mod.load_sequence(data, dev, sweep=sweep, sweep_fraction=sweep_fraction, sweep_ref=sweep_ref, sweep_direction=sweep_direction,
                                     actor_sweep=actor_sweep)
    if actor_twists:                                                        # what python -m lidar_rt_amd.train --refine-actor-twist learnt
        for (a_, f_), v in torch.load(actor_twists, map_location=dev, weights_only=False)["eta"].items():
            seq.boxes[a_].twist[f_] = v.to(dev)
    opt = training.default_options()
    scene = sequence_mod.scene_from_sequence(seq, max_points=max_points, seed=seed)
    scene.training_setup(opt)
    model_params, iteration = torch.load(ckpt, map_location=dev, weights_only=False)
    scene.restore(model_params, opt)
    if boxes:
        from .actor_poses import ActorPoses
        if not seq.boxes:
            raise SystemExit(f"--boxes: {data} has no tracking boxes (boxes.npz)")
        ActorPoses.from_state_dict(seq.boxes, torch.load(boxes, map_location=dev, weights_only=False)).install(scene.gaussians_assets)
    refiner = evaluate_mod.load_refiner(unet, dev, spatial=not unet_no_spatial, backend=unet_backend) if unet else None
    ids = {"test": seq.test_frames or seq.train_frames, "train": seq.train_frames, "all": sorted(set(seq.train_frames) | set(seq.test_frames))}[frames]
    if max_frames > 0:
        ids = ids[:max_frames]
    ids = [int(f) for f in ids]
    new_poses = ingest.read_poses(poses, sorted(int(f) for f in seq.frames.rays)) if poses else None
    assets, decomp, edits = apply_edits(scene.gaussians_assets, remove_actor, move_actor, only)
    sensor = build_sensor(seq, ids, height, width, inclination, mount, new_poses, sweep_ref, sweep_direction, sweep_fraction)
    if beams:
        # the sensor's beam table (lidar_rt_amd.beams), one (eps, delta) pair per row of the SIMULATED sensor; the origins stay one per column
        from . import beams as beams_mod
        rows = int(sensor.depth[ids[0]].shape[0])
        try:
            beams_mod.apply_table(sensor, beams_mod.load_table(beams, rows, dev), ids)
        except beams_mod.BeamError as e:
            raise SimulateError(f"simulate: --beams: {e}") from None
    bg = torch.tensor([0.0, 0.0, 1.0], device=dev)
    rargs = SimpleNamespace(dynamic=bool(seq.meta.get("dynamic")), opt=SimpleNamespace(use_rayhit=bool(getattr(opt, "use_rayhit", False))), pipe=SimpleNamespace())
    from . import renderer
    before = renderer.actor_sweep
    renderer.actor_sweep = actor_sweep != "off"                             # every Gaussian of a moving actor at its own instant (lidar_rt_amd.actor_sweep)
    try:
        renders = evaluation.render_frames(assets, sensor, ids, bg, rargs, refiner=refiner, decomp=decomp)
    finally:
        renderer.actor_sweep = before
    H, W = (int(x) for x in sensor.get_range_rays(ids[0])[0].shape[:2])
    pose_of = {f: sensor.pose_meta[f][1].detach().cpu().numpy().astype(np.float64) for f in ids}
    sw = {f: tuple(t.detach().cpu().numpy() for t in sensor.sweep_meta[f]) for f in ids if f in sensor.sweep_meta}
    T = None if frame == "world" else [column_transforms(frame, pose_of[f], *(sw[f] if f in sw else (None, None)),
                                                         origins=sensor.get_range_rays(f)[0][0] if (f in sw and origin_shift) else None) for f in ids]
    clouds = clouds_from_renders(renders, sensor, ids, raydrop_ratio, T, min_depth, unproject.FLT_MAX if max_depth is None else max_depth, backend)
    tau = {f: sw[f][1] for f in sw} or None
    write_clouds(out, ids, clouds, W, pose_of, fmt, fields, tau)
    counts = clouds.counts.cpu().tolist()
    report = {"format": SIMULATE_FORMAT, "iteration": int(iteration), "frames": [{"id": f, **dict(zip(unproject.COUNT_NAMES, (int(c) for c in counts[k])))} for k, f in enumerate(ids)],
              "height": H, "width": W, "frame": frame, "file_format": fmt, "fields": fields, "edits": edits,
              "arguments": {"data": data, "ckpt": ckpt, "frames": frames, "max_frames": max_frames, "raydrop_ratio": raydrop_ratio, "boxes": boxes, "unet": unet,
                            "sweep": sweep, "sweep_ref": sweep_ref, "sweep_direction": sweep_direction, "sweep_fraction": sweep_fraction, "height": height,
                            "width": width, "inclination": inclination, "mount": None if mount is None else [float(x) for x in mount], "poses": poses,
                            "min_depth": min_depth, "max_depth": max_depth, "backend": backend, "origin_shift": bool(origin_shift),
                            "actor_sweep": actor_sweep, "actor_twists": actor_twists, **({"beams": beams} if beams else {})},
              **({"twists": {str(f): [float(x) for x in sw[f][0]] for f in sw}, "tau": {str(f): [float(x) for x in sw[f][1]] for f in sw}} if sw else {})}
    with open(os.path.join(out, "simulate.json"), "w") as fh:
        json.dump(report, fh, indent=1)
    if sequence_dir:
        off = clouds.offsets.cpu().tolist()
        rows = []
        for k, f in enumerate(ids):
            kept = torch.zeros(H * W, dtype=torch.bool, device=dev)
            kept[clouds.pixel[off[k]:off[k + 1]].long()] = True
            kept = kept.reshape(H, W)
            inc = sensor.pose_meta[f][0]
            zero = lambda x: torch.where(kept, x, torch.zeros_like(x))       # not x * kept: an invalid pixel's NaN would stay
            rows.append({"id": f, "depth": zero(renders[f]["depth"].squeeze(-1)), "intensity": zero(renders[f]["intensity"].squeeze(-1)), "mask": kept,
                         "inclination": np.asarray(inc, np.float32), "sensor2world": pose_of[f], **({"twist": sw[f][0], "tau": sw[f][1]} if f in sw else {})})
        s2e = seq.meta.get("sensor2ego")
        sequence_mod.write_sequence(sequence_dir, rows, data_type=seq.meta["data_type"], extent=float(seq.meta.get("extent", 1.0)), sensor2ego=s2e)
    return report


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m lidar_rt_amd.simulate", description=__doc__.split("\n\n")[0])
    ap.add_argument("--data", required=True, help="sequence directory (lidar_rt_amd.sequence layout)")
    ap.add_argument("--ckpt", required=True, help="checkpoint in the reference's (model_params, iteration) layout (python -m lidar_rt_amd.train writes them)")
    ap.add_argument("--out", required=True, help="the directory of the clouds, poses.txt and simulate.json")
    ap.add_argument("--frames", choices=("test", "train", "all"), default="test", help="which frames (test falls back to train when the sequence names no test frames)")
    ap.add_argument("--max-frames", type=int, default=0)
    ap.add_argument("--raydrop-ratio", type=float, default=0.4, help="a pixel whose ray-drop probability is not below it is masked (eval.py:72)")
    ap.add_argument("--min-depth", type=float, default=0.0)
    ap.add_argument("--max-depth", type=float, default=None, help="a pixel is kept for min < depth <= max (default: no upper limit)")
    ap.add_argument("--max-points", type=int, default=2_000_000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--boxes", default=None, help="refined actor boxes (boxes<it>.pth of python -m lidar_rt_amd.train --refine-boxes) to render with")
    ap.add_argument("--unet", default=None, help="state_dict of the ray-drop refinement network, as python -m lidar_rt_amd.evaluate --unet")
    ap.add_argument("--unet-backend", choices=("hip", "torch"), default=None)
    ap.add_argument("--unet-no-spatial", action="store_true")
    ap.add_argument("--sweep", choices=("off", "stored", "poses"), default="off", help="render with one pose per column, as python -m lidar_rt_amd.evaluate --sweep")
    ap.add_argument("--sweep-ref", type=float, default=0.5)
    ap.add_argument("--sweep-direction", choices=("cw", "ccw"), default="cw")
    ap.add_argument("--sweep-fraction", type=float, default=1.0)
    ap.add_argument("--actor-sweep", choices=("off", "stored", "boxes"), default="off", help="the actors move within a sweep too (lidar_rt_amd.actor_sweep), as "
                    "python -m lidar_rt_amd.evaluate --actor-sweep; needs a --sweep.  --move-actor keeps an actor's twist: it is a motion in the actor's own frame")
    ap.add_argument("--actor-twists", default=None, help="--actor-sweep: learnt twists (actor_twists<it>.pth of python -m lidar_rt_amd.train --refine-actor-twist)")
    ap.add_argument("--beams", default=None, metavar="FILE", help="a beam table of the simulated sensor (lidar_rt_amd.beams): a beams<it>.pth of python -m "
                    "lidar_rt_amd.train --refine-beams, or a text table with one `eps delta` pair per image row (rad)")
    ap.add_argument("--height", type=int, default=None, help="rows of the simulated sensor (default: the sequence's)")
    ap.add_argument("--width", type=int, default=None, help="columns of the simulated sensor (default: the sequence's)")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--inclination", type=float, nargs=2, metavar=("A", "B"), help="the two inclination bounds [rad]")
    g.add_argument("--inclination-table", metavar="FILE", help="a per-beam inclination table [rad]: text, one angle per row")
    ap.add_argument("--mount", type=float, nargs=6, metavar=("X", "Y", "Z", "ROLL", "PITCH", "YAW"), help="sensor2world' = sensor2world @ M [m, rad]")
    ap.add_argument("--poses", default=None, metavar="FILE", help="ingest's pose-file format: replaces the poses of the ids it lists")
    ap.add_argument("--remove-actor", type=int, nargs="+", default=[], metavar="A")
    ap.add_argument("--move-actor", type=float, nargs=5, action="append", default=[], metavar=("A", "DX", "DY", "DZ", "YAW_DEG"),
                    help="a world-frame offset of the box centre and a rotation about world z in every frame (repeatable)")
    ap.add_argument("--only", choices=("background", "actors"), default=None, help="render that part of the scene alone (the reference renderer's decomp)")
    ap.add_argument("--frame", choices=FRAMES, default="world", help="the frame of the points: world; sensor (with --sweep: motion compensated); raw (each "
                    "point in the pose of its own column; needs --sweep)")
    ap.add_argument("--format", dest="fmt", choices=("bin", "npy"), default="bin")
    ap.add_argument("--fields", choices=("xyzi", "xyzirt"), default="xyzi", help="xyzirt adds the ring and the column's firing time")
    ap.add_argument("--sequence", dest="sequence_dir", default=None, metavar="DIR", help="also write the renders as a sequence directory (mask = kept pixels)")
    ap.add_argument("--backend", choices=("hip", "torch"), default=None, help="world-frame clouds: the HIP operator or the boolean-mask expression "
                    f"(default: {DEFAULT_WORLD_BACKEND}, profiles/unproject.md); the sensor and raw frames always take the operator")
    ap.add_argument("--no-origin-shift", dest="origin_shift", action="store_false", help="--sweep with --frame sensor / raw: the plain inverses of pose, twist "
                    "and tau, without moving each column's points from its float32 ray origin onto its exact origin")
    a = ap.parse_args(argv)
    try:
        rep = simulate(**vars(a))
    except SimulateError as e:
        print(str(e), file=sys.stderr)
        return 2
    n = sum(f["points"] for f in rep["frames"])
    print(f"simulate: {len(rep['frames'])} frames of {rep['height']} x {rep['width']} -> {n} points ({rep['frame']} frame); wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
