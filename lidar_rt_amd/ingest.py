"""Point clouds into a sequence directory: the converter that ``lidar_rt_amd/sequence.py`` promises, for any source of LiDAR scans.

    ingest_point_clouds(out_dir, clouds, H, W, inclination, data_type="KITTI", sensor2ego=None, max_depth=80.0, test_frames=(),
                        boxes=None, init=None, device=None, batch=16, twists=None, compensated=False, odometry=None, discover_actors=None)

``clouds`` yields ``(frame_id, points (N, 4) [x, y, z, intensity] in the SENSOR frame, sensor2world (4, 4))``.  ``batch`` frames go through
``range_image.project_points`` per call (``device="cuda"``: the HIP operator; ``"cpu"``: its float64 twin; ``None``: the HIP device when there
is one); the frames are written with ``sequence.write_sequence`` and ``out_dir/ingest.json`` records the arguments and the six counts of
every frame (points, invalid, out_of_range, out_of_view, hidden, pixels).  The sequence's ``extent`` is the largest range that became a pixel.

``twists`` ({id: (6,)}, ``sweep.twists_from_poses``) stores every frame's motion over its sweep for ``load_sequence(..., sweep="stored")``.  That
alone is right for RAW scans, whose points are each still expressed in the sensor frame of the instant they were fired at.  Most published
clouds (KITTI odometry, KITTI-360, nuScenes, Waymo) are motion COMPENSATED: every point has been moved into the sensor frame of one reference
instant.  ``compensated=True`` projects such frames with ``sweep_project.project_points_sweep`` under their twists -- every return lands in
the column that fired at it, with the range from that column's origin -- and stores the column times ``tau`` with each frame; ``ingest.json``
then records ``compensated``, ``sweep_ref``, ``sweep_direction`` and seven counts (``unseen``: points in the gaps between the columns' bins).

``odometry`` (a dict, possibly empty) is for scans that come WITHOUT poses: the ``sensor2world`` of ``clouds`` is ignored (it may be ``None``), the
frames are projected first -- the projection never needed the pose -- and ``registration.odometry`` aligns every frame to the one before it
(``registration.frame_geometry`` of the two range images, projective point-to-plane ICP).  Its keys: ``first_pose`` (4, 4) for the lowest id (the
identity otherwise), ``sweep_fraction`` to also derive and store the twists from the poses found, and the keyword arguments of
``registration.odometry`` (``schedule``, ``huber``, ``lam``, ``min_pairs``, ``tol_t``, ``tol_r``).  ``ingest.json`` gains ``"odometry"``: the
schedule, every pair's status and final number of partners, and the pairs that kept the constant-velocity guess.  It does not go with
``compensated``, which needs the twists before the projection.  Its key ``loop_closure`` (a dict with ``sensor_height`` and, optionally, the keyword
arguments of ``pose_graph.close_loops``: ``gap``, ``top``, ``max_score``, ``rings``, ``sectors``, ``r_max``, ...) corrects the chain's drift: the
frames that revisit an earlier place are found (``lidar_rt_amd.place``), verified by an alignment and entered as loop edges of a pose graph over
the pairs' hessians (``lidar_rt_amd.pose_graph``); the corrected poses go where the chain's went, and ``"odometry"`` gains ``"loop_closure"``
(the candidates, the accepted and the rejected pairs with the reason, the cost per iteration, and ``closure_error_chain`` / ``closure_error``:
the largest translation residual of a loop edge under the chain's poses and under the corrected ones).  Without the key nothing changes.
Its key ``map_tracking`` (a dict, possibly empty: ``voxel`` [0.2 m], ``trunc`` [4 voxels], ``max_voxels`` and the keyword arguments of
``map_registration.track_and_fuse``: ``iters``, ``huber``, ``lam``, ``min_pairs``, ``tol_t``, ``tol_r``, ``min_weight``) runs the chain first, sizes a
TSDF grid from the chain's poses (``mesh.grid_bounds``) and tracks every frame against everything fused so far
(``lidar_rt_amd.map_registration``), started from the chain's steps; the tracked poses go where the chain's went and ``ingest.json`` gains
``"map_tracking"``.  It does not go with ``loop_closure``.  The range image must be fine enough for the map (``map_registration``'s module text).

``discover_actors`` (a dict with ``sensor_height`` and, optionally, the keyword arguments of ``actors.discover``) runs ``lidar_rt_amd.actors.discover`` on
the projected frames once their poses are known -- given, or found by ``odometry`` -- and writes the moving actors' tracking boxes as ``boxes.npz``
and the report as ``actors.json``: what ``python -m lidar_rt_amd.actors`` adds to a finished sequence.  It does not go with ``boxes``.

    python -m lidar_rt_amd.ingest --points DIR --poses FILE --out DIR --height 66 --width 1030 --inclination -0.4346 0.0349
    python -m lidar_rt_amd.ingest --points DIR --odometry --out DIR --height 66 --width 1030 --inclination -0.4346 0.0349
    python -m lidar_rt_amd.ingest --points DIR --odometry --map-tracking [--map-voxel 0.2] [--map-trunc 0.8] --out DIR --height 66 --width 1030 ...
    python -m lidar_rt_amd.ingest --points DIR --odometry --discover-actors --sensor-height 1.8 --out DIR --height 66 --width 1030 --inclination ...

``--points DIR`` holds ``<id>.npy`` ``(N, 4)`` or KITTI-style ``<id>.bin`` (float32 quadruples), ids being integers.  ``--poses FILE`` is a ``.npy``
``(F, 4, 4)`` in the order of the sorted ids, or text rows of an id and 12 or 16 numbers (a 3 x 4 or 4 x 4 sensor-to-world matrix, row-major).
A frame without a row takes the last earlier pose, as the reference's KITTI loader does (lib/dataloader/kitti_loader/__init__.py:199-242);
``ingest.json`` records which frames did.  ``--missing-pose error`` refuses instead.  Exactly one of ``--poses`` and ``--odometry`` is given;
``--first-pose FILE`` is the pose of the first frame under ``--odometry``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Iterable, Optional, Sequence

import numpy as np
import torch

from . import range_image, sequence

INGEST_FORMAT = "lidar-rt-amd-ingest/1"


def ingest_point_clouds(out_dir: str, clouds: Iterable, H: int, W: int, inclination, data_type: str = "KITTI", sensor2ego=None, max_depth: float = 80.0,
                        test_frames: Sequence[int] = (), boxes: Optional[dict] = None, init: Optional[dict] = None, device=None, batch: int = 16,
                        wrap: bool = True, notes: Optional[dict] = None, twists: Optional[dict] = None, compensated: bool = False, tau=None,
                        sweep_ref: float = 0.5, sweep_direction: str = "cw", odometry: Optional[dict] = None,
                        discover_actors: Optional[dict] = None) -> dict:
    """See the module text.  ``wrap``: ``range_image.project_points``'s; ``notes``: further entries for ``ingest.json``; ``twists``: {id: (6,)} the
    sensor's motion over each frame's sweep (``sweep.twists_from_poses``), stored with the frame for ``load_sequence(..., sweep="stored")`` -- without
    ``compensated`` the projection itself is not changed by it.  ``compensated``: the clouds are motion compensated (``twists`` is required): they
    are projected under the sweep model with the column times ``tau`` ((W,), else ``sweep.column_times(W, sweep_ref, sweep_direction)``), which are
    stored with every frame.  ``odometry``: see the module text.  Returns what ``ingest.json`` holds."""
    if batch < 1:
        raise ValueError(f"ingest_point_clouds: batch {batch}")
    if odometry is not None and (compensated or twists is not None):
        raise ValueError("ingest_point_clouds: odometry finds the poses after the projection; compensated clouds and given twists need them before it")
    if discover_actors is not None and boxes is not None:
        raise ValueError("ingest_point_clouds: discover_actors finds the boxes; it does not go with given boxes")
    if discover_actors is not None and "sensor_height" not in discover_actors:
        raise ValueError("ingest_point_clouds: discover_actors needs sensor_height (the height of the sensor above the ground, metres)")
    names = range_image.COUNT_NAMES
    if compensated:
        from . import sweep, sweep_project
        if twists is None:
            raise ValueError("ingest_point_clouds: compensated clouds need the twists of their frames")
        names = sweep_project.COUNT_NAMES
        tau = np.asarray(sweep.column_times(int(W), sweep_ref, sweep_direction) if tau is None else (tau.detach().cpu() if torch.is_tensor(tau) else tau), np.float64).reshape(-1)
    elif tau is not None:
        raise ValueError("ingest_point_clouds: column times without compensated=True")
    dev = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
    inc = [float(x) for x in np.asarray(inclination, np.float64).reshape(-1)]
    per_frame, extent = [], [0.0]

    def twist_of(fid):
        if int(fid) not in twists:
            raise ValueError(f"ingest_point_clouds: frame {fid} has no twist")
        return np.asarray(twists[int(fid)], np.float64).reshape(6)

    def flush(group):
        sizes = [g[1].shape[0] for g in group]
        offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        pts = np.concatenate([g[1] for g in group]) if group else np.zeros((0, 4), np.float32)
        pts = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).to(dev)
        if compensated:
            img = sweep_project.project_points_sweep(pts, H, W, inc, np.stack([twist_of(g[0]) for g in group]), offsets=offsets, data_type=data_type,
                                                     sensor2ego=sensor2ego, tau=tau, max_depth=max_depth, wrap=wrap)
        else:
            img = range_image.project_points(pts, H, W, inc, offsets=offsets, data_type=data_type, sensor2ego=sensor2ego, max_depth=max_depth, wrap=wrap)
        depth, intensity, mask, counts = (t.cpu().numpy() for t in (img.depth, img.intensity, img.mask, img.counts))
        for k, (fid, _, s2w) in enumerate(group):
            per_frame.append({"id": int(fid), **{n: int(v) for n, v in zip(names, counts[k])}})
            if mask[k].any():
                extent[0] = max(extent[0], float(depth[k].max()))
            fr = {"id": int(fid), "depth": depth[k], "intensity": intensity[k], "mask": mask[k], "inclination": inc, "sensor2world": s2w}
            if twists is not None:
                fr["twist"] = twist_of(fid)
            if compensated:
                fr["tau"] = tau
            yield fr

    def frames():
        group = []
        for fid, pts, s2w in clouds:
            pts = np.asarray(pts.detach().cpu() if torch.is_tensor(pts) else pts)
            if pts.ndim != 2 or pts.shape[1] not in (3, 4):
                raise ValueError(f"ingest_point_clouds: frame {fid}: points must be (N, 4) or (N, 3), they are {pts.shape}")
            if pts.shape[1] == 3:
                pts = np.concatenate([pts, np.zeros((pts.shape[0], 1), pts.dtype)], 1)
            s2w = None if odometry is not None else np.asarray(s2w.detach().cpu() if torch.is_tensor(s2w) else s2w, np.float64).reshape(4, 4)
            group.append((fid, pts.astype(np.float32, copy=False), s2w))
            if len(group) == batch:
                yield from flush(group)
                group = []
        if group:
            yield from flush(group)

    done = list(frames())                                                    # every image first: the extent is known after the last one
    if odometry is not None:
        entry, tracking = _odometry(done, dict(odometry), H, W, inc, data_type, sensor2ego, dev, max_depth)
        notes = {**(notes or {}), "odometry": entry, **({"map_tracking": tracking} if tracking is not None else {})}
    actors_report = None
    if discover_actors is not None:
        from . import actors
        opts = dict(discover_actors)
        found, actors_report = actors.discover_images({int(fr["id"]): (fr["depth"], fr["mask"]) for fr in done}, {int(fr["id"]): np.asarray(fr["sensor2world"], np.float32).astype(np.float64) for fr in done},      # the poses as the frames store them
                                                     
                                                      opts.pop("sensor_height"), inc, data_type, sensor2ego, dev, **opts)
        boxes = found if actors_report["n_actors"] else None
        notes = {**(notes or {}), "actors": {"n_actors": actors_report["n_actors"], "tracks": len(actors_report["tracks"])}}
    meta = sequence.write_sequence(out_dir, done, data_type=data_type, extent=extent[0] if extent[0] > 0.0 else 1.0, sensor2ego=sensor2ego, boxes=boxes, init=init,
                                   test_frames=test_frames)
    total = {n: int(sum(f[n] for f in per_frame)) for n in names}
    report = {"format": INGEST_FORMAT, "height": int(H), "width": int(W), "inclination": inc, "data_type": data_type,
              "sensor2ego": None if sensor2ego is None else np.asarray(sensor2ego, np.float64).reshape(4, 4).tolist(), "max_depth": float(max_depth),
              "wrap": bool(wrap), "batch": int(batch), "device": dev.type, "extent": meta["extent"], "frames": per_frame, "total": total,
              **({"compensated": True, "sweep_ref": float(sweep_ref), "sweep_direction": sweep_direction} if compensated else {}), **(notes or {})}
    with open(os.path.join(out_dir, "ingest.json"), "w") as f:
        json.dump(report, f, indent=1)
    if actors_report is not None:
        actors.write_report(out_dir, actors_report)
    return report


class _Geometries:
    """{id: registration.frame_geometry of the frame} made on access, the last two kept: odometry reads consecutive pairs in id order."""

    def __init__(self, done, make):
        self.by_id, self.make, self.kept = {int(fr["id"]): fr for fr in done}, make, {}

    def __iter__(self):
        return iter(self.by_id)

    def __getitem__(self, i):
        if i not in self.kept:
            self.kept = {k: v for k, v in list(self.kept.items())[-1:]}
            self.kept[i] = self.make(self.by_id[i])
        return self.kept[i]


def _map_tracking(done, opts, frames, poses, steps, inc, data_type, sensor2ego, dev, max_depth):
    """The chain's poses replaced by poses tracked against the grid of everything fused so far: ({id: (4, 4)}, the report's entry)."""
    from . import map_registration, mesh
    voxel = float(opts.pop("voxel", 0.2))
    trunc = opts.pop("trunc", None)
    trunc = 4.0 * voxel if trunc is None else float(trunc)
    max_voxels = int(opts.pop("max_voxels", mesh.DEFAULT_MAX_VOXELS))
    if not (voxel > 0.0 and trunc > 0.0):
        raise ValueError(f"ingest_point_clouds: map_tracking voxel {voxel}, trunc {trunc} (both positive)")
    corners = []
    for i in sorted(poses):                                                 # the extent of every frame's returns under the chain's poses
        pts, _, mask = frames[i]
        p = pts[mask].detach().cpu().numpy().astype(np.float64) @ poses[i][:3, :3].T + poses[i][:3, 3]
        if len(p):
            corners.append(dict(world=np.stack([p.min(0), p.max(0)]), mask=np.ones(2, bool)))
    try:
        origin, dims = mesh.grid_bounds(corners, voxel, trunc)
    except mesh.MeshError as e:
        raise ValueError(f"ingest_point_clouds: map_tracking: {e}") from None
    if int(np.prod(dims)) > max_voxels:
        raise ValueError(f"ingest_point_clouds: map_tracking needs a grid of {dims[0]} x {dims[1]} x {dims[2]} voxels at voxel {voxel}, more than "
                         f"max_voxels {max_voxels}: a coarser voxel, or fewer frames")
    grid = mesh.TsdfGrid(origin, voxel, dims, trunc, dev, intensity=False)
    by_id = {int(fr["id"]): fr for fr in done}
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    images = {i: (up(fr["depth"], np.float32), up(fr["mask"], np.bool_)) for i, fr in by_id.items()}
    rel = {int(s["source"]): np.vstack([s["X"], [0.0, 0.0, 0.0, 1.0]]) for s in steps}
    tracked, rep = map_registration.track_and_fuse(grid, frames, images, first_pose=poses[min(poses)], steps=rel, inclination=inc, data_type=data_type,
                                                   sensor2ego=sensor2ego, max_depth=max_depth, **opts)
    moved = {i: float(np.linalg.norm(tracked[i][:3, 3] - poses[i][:3, 3])) for i in tracked}
    return tracked, {"voxel": voxel, "trunc": trunc, "origin": [float(x) for x in origin], "dims": [int(x) for x in dims],
                     "iterations": rep["iterations"], "huber": rep["huber"], "frames": rep["frames"], "failed": rep["failed"],
                     "observed_voxels": int((grid.weight > 0).sum()), "largest_correction": max(moved.values())}


def _odometry(done, opts, H, W, inc, data_type, sensor2ego, dev, max_depth=80.0):
    """Poses (and, with ``sweep_fraction``, twists) for the projected frames ``done``, in place; returns the report's ``"odometry"`` entry and its
    ``"map_tracking"`` entry (None without ``map_tracking``)."""
    from . import registration, sweep
    fraction = opts.pop("sweep_fraction", None)
    tracking = opts.pop("map_tracking", None)
    make = lambda fr: registration.frame_geometry(torch.from_numpy(np.ascontiguousarray(fr["depth"], np.float32)).to(dev),
                                                  torch.from_numpy(np.ascontiguousarray(fr["mask"])).to(dev), inc, int(H), int(W), data_type, sensor2ego)
    loop = opts.pop("loop_closure", None)
    if loop is not None and "sensor_height" not in loop:
        raise ValueError("ingest_point_clouds: loop_closure needs sensor_height (the height of the sensor above the ground, metres)")
    if loop is not None and tracking is not None:
        raise ValueError("ingest_point_clouds: map_tracking does not go with loop_closure")
    frames = {int(fr["id"]): make(fr) for fr in done} if loop is not None else _Geometries(done, make)     # the matcher describes all frames in one call
    poses, rep = registration.odometry(frames, inclination=inc, data_type=data_type, sensor2ego=sensor2ego, **opts, **({"return_steps": True} if loop is not None or tracking is not None else {}))
    closed = None
    if loop is not None:
        from . import pose_graph
        loops, found = pose_graph.close_loops(frames, poses, rep["steps"], inclination=inc, data_type=data_type, sensor2ego=sensor2ego, **loop)
        poses, solved = pose_graph.optimize(poses, pose_graph.odometry_edges(rep["steps"]) + loops)
        closed = {**found, "cost": solved["cost"], "iterations": solved["iterations"], "converged": solved["converged"], "loops": solved["loops"],
                  "closure_error_chain": max((e["before"][0] for e in solved["loops"] if e["kind"] == "loop"), default=None),
                  "closure_error": max((e["after"][0] for e in solved["loops"] if e["kind"] == "loop"), default=None)}
    tracked = None
    if tracking is not None:
        poses, tracked = _map_tracking(done, dict(tracking), frames, poses, rep["steps"], inc, data_type, sensor2ego, dev, max_depth)
    twists = sweep.twists_from_poses(poses, fraction) if fraction is not None else None
    for fr in done:
        fr["sensor2world"] = poses[int(fr["id"])]
        if twists is not None:
            fr["twist"] = twists[int(fr["id"])]
    return {"schedule": rep["schedule"], "pairs": rep["pairs"], "failed": rep["failed"], "first_pose": poses[min(poses)].tolist(),
            **({"loop_closure": closed} if closed is not None else {})}, tracked


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------------

def read_points(path: str) -> np.ndarray:
    if path.endswith(".npy"):
        a = np.load(path)
        if a.ndim != 2 or a.shape[1] not in (3, 4):
            raise ValueError(f"{path}: (N, 4) or (N, 3) expected, the array is {a.shape}")
        return a
    raw = np.fromfile(path, dtype=np.float32)
    if raw.size % 4:
        raise ValueError(f"{path}: {raw.size} float32 values are not quadruples")
    return raw.reshape(-1, 4)


def list_points(folder: str):
    """[(id, path)] sorted by id; ``<id>.npy`` wins over ``<id>.bin``."""
    found = {}
    for fn in sorted(os.listdir(folder)):
        stem, ext = os.path.splitext(fn)
        if ext in (".npy", ".bin") and stem.lstrip("-").isdigit():
            if int(stem) not in found or ext == ".npy":
                found[int(stem)] = os.path.join(folder, fn)
    if not found:
        raise ValueError(f"{folder}: no <id>.npy or <id>.bin file")
    return sorted(found.items())


def read_poses(path: str, ids: Sequence[int]) -> dict:
    """{id: (4, 4) float64} for the ids that have a pose."""
    if path.endswith(".npy"):
        a = np.load(path).astype(np.float64)
        if a.ndim != 3 or a.shape != (len(ids), 4, 4):
            raise ValueError(f"{path}: ({len(ids)}, 4, 4) expected for {len(ids)} frames, the array is {a.shape}")
        return {i: a[k] for k, i in enumerate(ids)}
    poses = {}
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            t = line.split()
            if not t or t[0].startswith("#"):
                continue
            if len(t) not in (13, 17):
                raise ValueError(f"{path}:{ln}: an id and 12 or 16 numbers expected, {len(t)} fields found")
            m = np.eye(4)
            m.reshape(-1)[:len(t) - 1] = [float(x) for x in t[1:]]
            poses[int(float(t[0]))] = m
    return poses


def matrix_file(path: str) -> np.ndarray:
    a = np.load(path) if path.endswith(".npy") else np.loadtxt(path)
    a = np.asarray(a, np.float64).reshape(-1)
    if a.size == 12:
        a = np.concatenate([a, [0, 0, 0, 1]])
    if a.size != 16:
        raise ValueError(f"{path}: a 3 x 4 or 4 x 4 matrix expected")
    return a.reshape(4, 4)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m lidar_rt_amd.ingest", description="Project point clouds into range images and write a sequence directory.")
    ap.add_argument("--points", required=True, help="directory of <id>.npy (N, 4) or KITTI-style <id>.bin float32 quadruples, points in the sensor frame")
    ap.add_argument("--poses", help=".npy (F, 4, 4) in the order of the sorted ids, or text rows: id and 12 or 16 numbers (sensor to world); this or --odometry")
    ap.add_argument("--odometry", action="store_true", help="the scans come without poses: align every frame to the one before it (lidar_rt_amd.registration) "
                    "and write the trajectory found; this or --poses")
    ap.add_argument("--first-pose", help="--odometry: the pose of the first frame, a 4 x 4 (or 3 x 4) matrix, .npy or text (the identity otherwise)")
    ap.add_argument("--out", required=True, help="the sequence directory to write")
    ap.add_argument("--sensor2ego", help="a 4 x 4 (or 3 x 4) matrix, .npy or text: the yaw of Waymo data")
    ap.add_argument("--height", type=int, required=True)
    ap.add_argument("--width", type=int, required=True)
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--inclination", type=float, nargs=2, metavar=("LO", "HI"), help="the two inclination bounds [rad]")
    g.add_argument("--beams", help="a per-beam inclination table [rad], one value per row: .npy or text")
    ap.add_argument("--data-type", choices=("KITTI", "Waymo"), default="KITTI")
    ap.add_argument("--max-depth", type=float, default=80.0)
    ap.add_argument("--no-wrap", action="store_true", help="drop a column index outside [0, W) as the reference's loader does, instead of wrapping it")
    ap.add_argument("--test-frames", type=int, nargs="*", default=[])
    ap.add_argument("--missing-pose", choices=("previous", "error"), default="previous", help="a frame without a pose row: the last earlier pose, or refuse")
    ap.add_argument("--sweep", action="store_true", help="also store every frame's twist -- the sensor's motion over one sweep, derived from consecutive poses "
                    "(lidar_rt_amd.sweep.twists_from_poses) -- for train / evaluate --sweep stored")
    ap.add_argument("--sweep-fraction", type=float, default=1.0, help="--sweep: the part of the time between two consecutive frame ids that one sweep takes")
    ap.add_argument("--compensated", action="store_true", help="--sweep: the clouds are motion compensated (every point in the sensor frame of the frame's reference "
                    "instant, as KITTI, nuScenes and Waymo publish them): project them under the sweep model (lidar_rt_amd.sweep_project)")
    ap.add_argument("--sweep-ref", type=float, default=0.5, help="--compensated: the part of the sweep at which a frame's pose holds (0 = its first column, 0.5 = its middle)")
    ap.add_argument("--sweep-direction", choices=("cw", "ccw"), default="cw", help="--compensated: cw = time rises with the column index (a clockwise-spinning sensor)")
    ap.add_argument("--discover-actors", action="store_true", help="once the poses are known (--poses or --odometry), find the moving actors "
                    "(lidar_rt_amd.actors) and write their tracking boxes as boxes.npz, the report as actors.json; needs --sensor-height")
    ap.add_argument("--sensor-height", type=float, help="--discover-actors: the height of the sensor above the ground [m]")
    ap.add_argument("--loop-closure", action="store_true", help="--odometry: find the frames that revisit an earlier place (lidar_rt_amd.place), verify them with an "
                    "alignment and correct the chain with a pose graph (lidar_rt_amd.pose_graph); needs --sensor-height")
    ap.add_argument("--loop-gap", type=int, default=20, help="--loop-closure: a frame is compared with the frames at least this many before it")
    ap.add_argument("--loop-top", type=int, default=2, help="--loop-closure: the candidates per frame that are verified")
    ap.add_argument("--loop-max-score", type=float, default=None, help="--loop-closure: the largest descriptor score (0 identical, 1 disjoint) of a candidate")
    ap.add_argument("--place-rings", type=int, default=None, help="--loop-closure: the rings of the descriptor (at most 32)")
    ap.add_argument("--place-sectors", type=int, default=None, help="--loop-closure: the sectors of the descriptor (at most 128 and --width)")
    ap.add_argument("--place-range", type=float, default=None, help="--loop-closure: the outer ground range of the descriptor [m]")
    ap.add_argument("--map-tracking", action="store_true", help="--odometry: after the chain, fuse the frames into a TSDF grid sized from the chain's poses and "
                    "align every frame to everything fused before it (lidar_rt_amd.map_registration); the tracked poses are written")
    ap.add_argument("--map-voxel", type=float, default=0.2, help="--map-tracking: the voxel of the grid [m]")
    ap.add_argument("--map-trunc", type=float, default=None, help="--map-tracking: the truncation distance [m] (default: 4 voxels)")
    ap.add_argument("--device", choices=("cpu", "cuda"), default=None)
    ap.add_argument("--batch", type=int, default=16)
    a = ap.parse_args(argv)
    if a.map_tracking and not a.odometry:
        print("ingest: --map-tracking goes with --odometry (it starts from the chain's steps)", file=sys.stderr)
        return 2
    if a.map_tracking and a.loop_closure:
        print("ingest: --map-tracking does not go with --loop-closure: tracking against a map that a pose graph moves afterwards is not built yet", file=sys.stderr)
        return 2
    if a.loop_closure and not a.odometry:
        print("ingest: --loop-closure goes with --odometry", file=sys.stderr)
        return 2
    if a.loop_closure and a.sensor_height is None:
        print("ingest: --loop-closure and --sensor-height Z go together", file=sys.stderr)
        return 2
    if a.discover_actors != (a.sensor_height is not None) and not (a.loop_closure and not a.discover_actors):
        print("ingest: --discover-actors and --sensor-height Z go together", file=sys.stderr)
        return 2
    if bool(a.poses) == bool(a.odometry):
        print("ingest: give exactly one of --poses FILE and --odometry" + (" (both were given)" if a.poses else " (neither was given)"), file=sys.stderr)
        return 2
    if a.odometry and a.compensated:
        print("ingest: --odometry does not go with --compensated: compensated clouds are projected under their twists, which would need a second "
              "projection pass after the poses are found", file=sys.stderr)
        return 2
    if a.first_pose and not a.odometry:
        print("ingest: --first-pose goes with --odometry", file=sys.stderr)
        return 2
    if a.compensated and not a.sweep:
        print("ingest: --compensated needs --sweep (the twists the clouds were compensated with)", file=sys.stderr)
        return 2
    files = list_points(a.points)
    ids = [i for i, _ in files]
    if a.odometry and a.sweep and len(ids) < 2:
        print("ingest: --sweep: twists from poses need at least two frames", file=sys.stderr)
        return 2
    poses = {i: None for i in ids} if a.odometry else read_poses(a.poses, ids)
    inc = list(a.inclination) if a.inclination else (np.load(a.beams) if a.beams.endswith(".npy") else np.loadtxt(a.beams)).reshape(-1).tolist()
    borrowed, use, last = {}, {}, None
    for i in ids:
        if i in poses:
            last = i
        elif a.missing_pose == "error" or last is None:
            print(f"ingest: frame {i} has no pose" + ("" if a.missing_pose == "error" else " and no earlier frame has one"), file=sys.stderr)
            return 2
        else:
            borrowed[str(i)] = last
        use[i] = poses[last]
    twists = None
    if a.sweep and not a.odometry:
        from . import sweep
        try:
            twists = sweep.twists_from_poses(use, a.sweep_fraction)
        except sweep.SweepError as e:
            print(f"ingest: --sweep: {e}", file=sys.stderr)
            return 2
    clouds = ((i, read_points(p), use[i]) for i, p in files)
    rep = ingest_point_clouds(a.out, clouds, a.height, a.width, inc, data_type=a.data_type, sensor2ego=matrix_file(a.sensor2ego) if a.sensor2ego else None,
                              max_depth=a.max_depth, test_frames=a.test_frames, device=a.device, batch=a.batch, wrap=not a.no_wrap,
                              notes={"pose_taken_from": borrowed, **({"sweep_fraction": float(a.sweep_fraction)} if a.sweep else {})}, twists=twists,
                              **({"odometry": {**({"first_pose": matrix_file(a.first_pose)} if a.first_pose else {}),
                                               **({"sweep_fraction": a.sweep_fraction} if a.sweep else {}),
                                               **({"map_tracking": {"voxel": a.map_voxel, "trunc": a.map_trunc}} if a.map_tracking else {}),
                                               **({"loop_closure": {"sensor_height": a.sensor_height, "gap": a.loop_gap, "top": a.loop_top,
                                                                    **({"max_score": a.loop_max_score} if a.loop_max_score is not None else {}),
                                                                    **({"rings": a.place_rings} if a.place_rings is not None else {}),
                                                                    **({"sectors": a.place_sectors} if a.place_sectors is not None else {}),
                                                                    **({"r_max": a.place_range} if a.place_range is not None else {})}} if a.loop_closure else {})}}
                                 if a.odometry else {}),
                              **(dict(compensated=True, sweep_ref=a.sweep_ref, sweep_direction=a.sweep_direction) if a.compensated else {}),
                              **({"discover_actors": {"sensor_height": a.sensor_height}} if a.discover_actors else {}))
    t = rep["total"]
    unseen = f"{t['unseen']} unseen, " if a.compensated else ""
    print(f"ingest: {len(ids)} frames, {t['points']} points -> {t['pixels']} pixels ({t['hidden']} hidden, {t['out_of_view']} out of view, {unseen}"
          f"{t['out_of_range']} out of range, {t['invalid']} invalid); " + (f"{len(rep['odometry']['failed'])} of {len(rep['odometry']['pairs'])} pairs kept the constant-velocity guess"
                                                                           if a.odometry else f"{len(borrowed)} frames took an earlier pose")
          + (f"; {len(rep['odometry']['loop_closure']['accepted'])} loops closed" if a.loop_closure else "")
          + (f"; map tracking moved the chain by up to {rep['map_tracking']['largest_correction']:.3f} m, {len(rep['map_tracking']['failed'])} frames kept their start"
             if a.map_tracking else "")
          + (f"; {rep['actors']['n_actors']} moving actors" if a.discover_actors else "") + f"; wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
