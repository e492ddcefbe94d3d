"""Moving actors from scans: the tracking boxes of a dynamic scene without a dataset's labels.

    boxes, report = discover(frames, poses, sensor_height, inclination=..., data_type="KITTI", sensor2ego=None)
    python -m lidar_rt_amd.actors --data DIR --sensor-height Z [--force]

``frames`` is ``{id: (points (H, W, 3) float32, depth (H, W) float32, mask (H, W))}`` in the SENSOR frame (``frames_from_depth`` makes them from
range images), ``poses`` ``{id: (4, 4) sensor2world}``.  On a HIP device the five operators of ``lidar_rt_amd.segmentation`` run in
``liblrt_segment.so``; on the CPU their exact numpy twins do.  Everything after the integer tables is host float64 and is the same code on both
paths, so both return the same bits.

What ``discover`` does:

1. ``ground``, ``label`` (the ground excluded), ``freespace`` against frame k - 1 and against frame k + 1, and ``stats`` for all frames in one call
   each; then ONE host read (the tables and their counts).
2. Candidate segments: at least ``min_points`` pixels, a horizontal bound diagonal in ``[0.5, 12]`` m and a height in ``[0.3, 4]`` m (sensor frame).
3. World centroids from the integer sums and the poses.
4. A greedy tracker in frame order: the prediction is a track's last centroid plus its last per-frame displacement; the (track, segment) pairs
   within ``gate`` metres are sorted by (distance, track id, segment id) and assigned greedily; unmatched segments open tracks; a track unmatched
   for more than ``max_gap`` frames closes.  There is no randomness.
5. A track is a MOVING ACTOR if and only if it has at least ``min_track`` frames, ``sum free / sum known >= min_free`` over both evidence images,
   and its first and last centroid are at least ``min_disp`` apart.  The free-space fraction is the test proper -- a parked car's centroid also
   wanders as its visible side changes; the displacement is there only so that a heading exists.
6. Yaw per frame from the world-xy direction of the centroid's central difference (one-sided at the ends).  ROLL AND PITCH ARE ZERO AND THE WORLD
   Z AXIS IS UP, as in every sequence this project writes.
7. ``track_bounds`` in those frames: ``size = extent + 2 pad``, and every frame's translation is the centroid moved by the bounds' centre.
8. The dictionary ``sequence.write_sequence(boxes=...)`` takes -- ``frames``, ``translation``, ``quaternion`` (w, x, y, z), ``valid``, ``size`` -- and a
   report with every track's length, free fraction, displacement and why it was dropped.

LIMITATION: one box per track is the union of partial views around a drifting centroid, so it is looser than a labelled box;
``train --refine-boxes`` is the tool that tightens the poses afterwards.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np
import torch

from . import segmentation as sg

ACTORS_FORMAT = "lidar-rt-amd-actors/1"
DEFAULTS = dict(min_points=30, gate=2.0, max_gap=1, min_track=4, min_free=0.04, min_disp=1.0, pad=0.1, s_max=4096)


class ActorsError(RuntimeError):
    pass


@torch.no_grad()
def frames_from_depth(images, inclination, data_type="KITTI", sensor2ego=None, device=None):
    """{id: (points, depth, mask)} from {id: (depth (H, W), mask (H, W))} numpy arrays or tensors, on ``device``."""
    out = {}
    for fid, (depth, mask) in images.items():
        depth = torch.as_tensor(np.ascontiguousarray(depth, np.float32) if isinstance(depth, np.ndarray) else depth)
        mask = torch.as_tensor(np.ascontiguousarray(mask) if isinstance(mask, np.ndarray) else mask)
        if device is not None:
            depth, mask = depth.to(device), mask.to(device)
        pts, m = sg.frame_points(depth, mask, inclination, data_type=data_type, sensor2ego=sensor2ego)
        out[int(fid)] = (pts, torch.where(m, depth.to(torch.float32), torch.zeros_like(depth, dtype=torch.float32)).contiguous(), m)
    return out


def _pose(T):
    T = np.asarray(T.detach().cpu() if torch.is_tensor(T) else T, np.float64).reshape(-1)
    if T.size == 12:
        T = np.concatenate([T, [0.0, 0.0, 0.0, 1.0]])
    if T.size != 16:
        raise ActorsError("discover: a pose must be a (4, 4) or (3, 4) matrix")
    return T.reshape(4, 4)


def _inverse(T):
    R, t = T[:3, :3], T[:3, 3]
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = R.T, -(R.T @ t)
    return out


@torch.no_grad()
def tables(frames, poses, sensor_height, inclination, data_type="KITTI", sensor2ego=None, s_max=4096, ground_kw=None, label_kw=None, freespace_kw=None):
    """Step 1: (ids, points (F, H, W, 3), stats on the frames' device).  No host read."""
    ids = sorted(int(i) for i in frames)
    if not ids:
        raise ActorsError("discover: no frames")
    pts, depth, mask = (torch.stack([frames[i][k] for i in ids]) for k in range(3))
    pts, depth = pts.to(torch.float32).contiguous(), depth.to(torch.float32).contiguous()
    mask = (mask != 0).contiguous()
    dev = pts.device
    T = [_pose(poses[i]) for i in ids]
    F = len(ids)
    g = sg.ground(pts, mask, sensor_height, inclination, **(ground_kw or {}))
    lab = sg.label(pts, mask, exclude=g, inclination=inclination, **(label_kw or {}))
    ev = []
    for step in (-1, 1):                                                      # against the frame before, against the frame after
        other = [min(max(k + step, 0), F - 1) for k in range(F)]
        has = torch.tensor([0 <= k + step < F for k in range(F)], device=dev)
        X = torch.from_numpy(np.stack([(_inverse(T[o]) @ T[k])[:3] for k, o in enumerate(other)])).to(dev)
        idx = torch.tensor(other, device=dev)
        t_mask = mask.index_select(0, idx) & has[:, None, None]               # no neighbour: an empty target, every verdict -1
        ev.append(sg.freespace((pts, mask), (depth.index_select(0, idx), t_mask), X, inclination=inclination, data_type=data_type, sensor2ego=sensor2ego,
                               **(freespace_kw or {})))
    return ids, T, pts, sg.stats(pts, lab, ev, s_max)


def _track(cands, F, gate, max_gap):
    """cands[k]: [(segment id, world centroid)] of frame k.  Returns tracks: lists of (k, segment id, centroid)."""
    tracks, live = [], []
    for k in range(F):
        pairs = []
        for t in live:
            tr = tracks[t]
            last = tr[-1]
            vel = (last[2] - tr[-2][2]) / (last[0] - tr[-2][0]) if len(tr) > 1 else np.zeros(3)
            pred = last[2] + vel * (k - last[0])
            for s, c in cands[k]:
                d = float(np.linalg.norm(c - pred))
                if d <= gate:
                    pairs.append((d, t, s))
        pairs.sort()
        used_t, used_s = set(), set()
        by_id = dict(cands[k])
        for d, t, s in pairs:
            if t in used_t or s in used_s:
                continue
            used_t.add(t); used_s.add(s)
            tracks[t].append((k, s, by_id[s]))
        for s, c in cands[k]:
            if s not in used_s:
                tracks.append([(k, s, c)])
                live.append(len(tracks) - 1)
        live = [t for t in live if k - tracks[t][-1][0] <= max_gap]
    return tracks


@torch.no_grad()
def discover(frames, poses, sensor_height, inclination, data_type="KITTI", sensor2ego=None, min_points=DEFAULTS["min_points"], gate=DEFAULTS["gate"],
             max_gap=DEFAULTS["max_gap"], min_track=DEFAULTS["min_track"], min_free=DEFAULTS["min_free"], min_disp=DEFAULTS["min_disp"], pad=DEFAULTS["pad"],
             s_max=DEFAULTS["s_max"], ground_kw=None, label_kw=None, freespace_kw=None):
    """(boxes, report): see the module text.  The boxes are float64 numpy arrays; ``boxes["translation"].shape[0]`` is the number of actors (it may
    be 0).  Roll and pitch of every box are zero and the world z axis is up.  One box per track is the union of partial views around a drifting
    centroid: looser than a labelled box (``train --refine-boxes`` tightens the poses)."""
    ids, T, pts, st = tables(frames, poses, sensor_height, inclination, data_type, sensor2ego, s_max, ground_kw, label_kw, freespace_kw)
    F = len(ids)
    packed = torch.cat([st.table.reshape(F, -1), st.n_seg[:, None].to(torch.int64), st.overflow[:, None].to(torch.int64)], 1).cpu().numpy()   # the one host read
    table, n_seg, overflow = packed[:, :-2].reshape(F, int(s_max), sg.NCOL), packed[:, -2], packed[:, -1]
    Q = sg.QUANT
    cands = []
    for k in range(F):
        rows = table[k, :n_seg[k]]
        cnt = rows[:, sg.COL_COUNT]
        ext = (rows[:, sg.COL_MAX:sg.COL_MAX + 3] - rows[:, sg.COL_MIN:sg.COL_MIN + 3]).astype(np.float64) / Q
        diag = np.hypot(ext[:, 0], ext[:, 1])
        ok = (cnt >= min_points) & (diag >= 0.5) & (diag <= 12.0) & (ext[:, 2] >= 0.3) & (ext[:, 2] <= 4.0)
        frame = []
        for s in np.nonzero(ok)[0]:
            c = rows[s, sg.COL_SUM:sg.COL_SUM + 3].astype(np.float64) / float(cnt[s]) / Q
            frame.append((int(s), T[k][:3, :3] @ c + T[k][:3, 3]))
        cands.append(frame)
    tracks = _track(cands, F, float(gate), int(max_gap))
    kept, rep = [], []
    for n, tr in enumerate(tracks):
        ev = np.stack([table[k, s, sg.COL_EV:sg.COL_EV + 4] for k, s, _ in tr]).sum(0)
        free, known = int(ev[0] + ev[2]), int(ev[1] + ev[3])
        frac = free / known if known else 0.0
        disp = float(np.linalg.norm(tr[-1][2] - tr[0][2]))
        why = None
        if len(tr) < min_track:
            why = "short"
        elif frac < min_free:
            why = "static"
        elif disp < min_disp:
            why = "no displacement"
        rep.append({"track": n, "first_frame": ids[tr[0][0]], "length": len(tr), "free": free, "known": known, "free_fraction": frac, "displacement": disp,
                    "dropped": why, "first_centroid": tr[0][2].tolist(), "last_centroid": tr[-1][2].tolist()})
        if why is None:
            kept.append(n)
    A = len(kept)
    translation, quaternion = np.zeros((A, F, 3)), np.zeros((A, F, 4))
    quaternion[..., 0] = 1.0
    valid, size = np.zeros((A, F), bool), np.zeros((A, 3))
    if A:
        track_of = np.full((F, int(s_max)), -1, np.int32)
        pose = np.tile(np.eye(4)[:3], (A, F, 1, 1))
        yaw, cen = np.zeros((A, F)), np.zeros((A, F, 3))
        for a, n in enumerate(kept):
            tr = tracks[n]
            for j, (k, s, c) in enumerate(tr):
                lo, hi = tr[max(j - 1, 0)], tr[min(j + 1, len(tr) - 1)]
                d = hi[2] - lo[2]
                yaw[a, k] = math.atan2(d[1], d[0])
                cen[a, k] = c
                valid[a, k] = True
                track_of[k, s] = a
                A2W = np.eye(4)
                cy, sy = math.cos(yaw[a, k]), math.sin(yaw[a, k])
                A2W[:3, :3] = [[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]]
                A2W[:3, 3] = c
                pose[a, k] = (_inverse(T[k]) @ A2W)[:3]
        dev = pts.device
        bounds, count = sg.track_bounds(pts, st.seg, torch.from_numpy(track_of).to(dev), torch.from_numpy(pose).to(dev))
        bounds, count = bounds.cpu().numpy(), count.cpu().numpy()
        for a, n in enumerate(kept):
            lo, hi = bounds[a, :3].astype(np.float64) / Q, bounds[a, 3:].astype(np.float64) / Q
            size[a] = (hi - lo) + 2.0 * float(pad)
            mid = 0.5 * (lo + hi)
            for k in np.nonzero(valid[a])[0]:
                cy, sy = math.cos(yaw[a, k]), math.sin(yaw[a, k])
                translation[a, k] = cen[a, k] + np.array([cy * mid[0] - sy * mid[1], sy * mid[0] + cy * mid[1], mid[2]])
                quaternion[a, k] = (math.cos(0.5 * yaw[a, k]), 0.0, 0.0, math.sin(0.5 * yaw[a, k]))
            rep[n]["actor"] = a
            rep[n]["pixels"] = int(count[a])
    boxes = {"frames": np.asarray(ids, np.int64), "translation": translation, "quaternion": quaternion, "valid": valid, "size": size}
    report = {"format": ACTORS_FORMAT, "frames": ids, "n_actors": A, "segments": [int(v) for v in n_seg], "overflow": [int(v) for v in overflow],
              "parameters": dict(sensor_height=float(sensor_height), min_points=int(min_points), gate=float(gate), max_gap=int(max_gap), min_track=int(min_track),
                                 min_free=float(min_free), min_disp=float(min_disp), pad=float(pad), s_max=int(s_max)),
              "tracks": [r for r in rep if r["length"] >= 2 or r["dropped"] is None]}
    return boxes, report


def discover_sequence(root, sensor_height, device=None, **kw):
    """``discover`` on the frames of a sequence directory: (boxes, report)."""
    with open(os.path.join(root, "meta.json")) as f:
        meta = json.load(f)
    dev = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
    images, poses, inc = {}, {}, None
    from .sequence import _frame_path
    for fid in meta["frames"]:
        z = np.load(_frame_path(root, fid))
        images[int(fid)] = (z["depth"], z["mask"])
        poses[int(fid)] = z["sensor2world"].astype(np.float64)
        inc = [float(x) for x in z["inclination"].reshape(-1)]
    return discover_images(images, poses, sensor_height, inc, meta["data_type"], meta.get("sensor2ego"), dev, **kw)


def discover_images(images, poses, sensor_height, inclination, data_type, sensor2ego, device, **kw):
    frames = frames_from_depth(images, inclination, data_type, sensor2ego, device)
    return discover(frames, poses, sensor_height, inclination, data_type, sensor2ego, **kw)


def write_report(root, report):
    with open(os.path.join(root, "actors.json"), "w") as f:
        json.dump(report, f, indent=1)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m lidar_rt_amd.actors", description="Find the moving actors of a sequence and write their tracking boxes.")
    ap.add_argument("--data", required=True, help="a sequence directory (meta.json, frames/)")
    ap.add_argument("--sensor-height", type=float, required=True, help="the height of the sensor above the ground [m]")
    ap.add_argument("--force", action="store_true", help="overwrite an existing boxes.npz")
    ap.add_argument("--device", choices=("cpu", "cuda"), default=None)
    for name, val in DEFAULTS.items():
        ap.add_argument("--" + name.replace("_", "-"), type=type(val), default=val)
    a = ap.parse_args(argv)
    from . import sequence
    if os.path.exists(os.path.join(a.data, "boxes.npz")) and not a.force:
        print(f"actors: {a.data} already has a boxes.npz (--force overwrites it)", file=sys.stderr)
        return 2
    boxes, report = discover_sequence(a.data, a.sensor_height, a.device, **{n: getattr(a, n) for n in DEFAULTS})
    write_report(a.data, report)
    if report["n_actors"]:
        sequence.write_boxes(a.data, boxes, force=a.force)
    print(f"actors: {len(report['frames'])} frames, {sum(report['segments'])} segments, {len(report['tracks'])} tracks, {report['n_actors']} moving actors; "
          + (f"wrote {os.path.join(a.data, 'boxes.npz')}" if report["n_actors"] else "no boxes.npz written"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
