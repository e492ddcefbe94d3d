#!/usr/bin/env python3
"""Time the scene initialisation from range images (lidar_rt_amd.scene_init) on an analytic sequence: a ground plane and box-shaped actors
seen through a spinning-LiDAR grid, written in the on-disk layout of lidar_rt_amd/sequence.py (no tracer needed: the ranges are ray / plane
and ray / box intersections in numpy).

    python tools/bench_scene_init.py [--height 64 --width 2048 --frames 50 --actors 8] [--reference-frames 1] [--json OUT]

Reports, per stage, the GPU time over all frames (HIP events around the operators alone), the launches per call, the time of the
``*_reference`` twins on CPU tensors (``--reference-frames`` frames only: the brute-force neighbour search is quadratic), and the library's
VGPR / LDS table.  ``write_analytic_sequence`` is also what the tests of the feature train on.  Reported, not gated.
"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

GROUND_Z = -1.73
BODY = np.array([4.6, 2.1, 1.8], np.float32)


def _yaw_quat(yaw):
    return np.array([math.cos(yaw / 2), 0.0, 0.0, math.sin(yaw / 2)], np.float32)


def _yaw_matrix(yaw):
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)


def actor_pose(a: int, f: int):
    """Actor a at frame f: on a circle of 7 + 3 a metres around the origin, heading along it."""
    r, ph = 7.0 + 3.0 * a, 0.9 * a + 0.02 * f * (1 if a % 2 == 0 else -1)
    return np.array([r * math.cos(ph), r * math.sin(ph), GROUND_Z + 0.5 * BODY[2]], np.float32), ph + math.pi / 2


def write_analytic_sequence(out: str, H: int = 16, W: int = 256, n_frames: int = 4, n_actors: int = 2, with_extent: bool = True, init=None,
                            noise: float = 0.0, seed: int = 0) -> dict:
    """Frames of a ground plane (z = GROUND_Z, intensity 0.3) and ``n_actors`` boxes (intensity 0.8) under a KITTI-style grid; tracking boxes
    0.4 m larger than the bodies.  Returns the meta dictionary; ``with_extent=False`` drops ``extent`` from meta.json."""
    from lidar_rt_amd import sequence
    from lidar_rt_amd.training import RangeFrames
    rng = np.random.default_rng(seed)
    inc = (math.radians(-24.9), math.radians(2.0))
    frames = []
    for f in range(n_frames):
        s2w = np.eye(4, dtype=np.float32)
        s2w[:3, :3] = _yaw_matrix(0.01 * f).astype(np.float32); s2w[0, 3] = 0.5 * f
        o, d = RangeFrames.range_rays(H, W, inc, torch.as_tensor(s2w), "KITTI")
        o, d = o.numpy().astype(np.float64), d.numpy().astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(d[..., 2] < -1e-6, (GROUND_Z - o[..., 2]) / d[..., 2], np.inf)
        inten = np.full((H, W), 0.3)
        for a in range(n_actors):
            c, yaw = actor_pose(a, f)
            R = _yaw_matrix(yaw)
            lo_, ld = (o - c.astype(np.float64)) @ R, d @ R                      # the ray in the actor's frame
            with np.errstate(divide="ignore", invalid="ignore"):
                t0, t1 = (-0.5 * BODY - lo_) / ld, (0.5 * BODY - lo_) / ld
            tn, tf = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
            hit = (tn < tf) & (tn > 0.1) & (tn < t)
            t = np.where(hit, tn, t); inten = np.where(hit, 0.8, inten)
        mask = np.isfinite(t) & (t < 80.0)
        depth = np.where(mask, t + noise * rng.standard_normal((H, W)), 0.0).astype(np.float32)
        frames.append({"id": f, "depth": depth, "intensity": (inten * mask).astype(np.float32), "mask": mask, "inclination": np.asarray(inc, np.float32),
                       "sensor2world": s2w})
    boxes = None
    if n_actors:
        tr = np.stack([[actor_pose(a, f)[0] for f in range(n_frames)] for a in range(n_actors)])
        qu = np.stack([[_yaw_quat(actor_pose(a, f)[1]) for f in range(n_frames)] for a in range(n_actors)])
        boxes = {"frames": list(range(n_frames)), "translation": tr, "quaternion": qu, "size": np.tile(BODY + 0.4, (n_actors, 1))}
    meta = sequence.write_sequence(out, frames, data_type="KITTI", extent=40.0, boxes=boxes, init=init)
    if not with_extent:
        del meta["extent"]
        with open(os.path.join(out, "meta.json"), "w") as fh:
            json.dump(meta, fh, indent=1)
    return meta


def _gpu_ms(fn, reps=1):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        out = fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--height", type=int, default=64); ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=50); ap.add_argument("--actors", type=int, default=8)
    ap.add_argument("--knn", type=int, default=6); ap.add_argument("--voxel-size", type=float, default=0.15)
    ap.add_argument("--reference-frames", type=int, default=1, help="frames the CPU twins are timed on (0: skip them)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    from lidar_rt_amd import build as lrt_build, grid_chamfer, resources, scene_init as si, sequence
    dev = torch.device("cuda:0")
    res = {"shape": [args.height, args.width], "frames": args.frames, "actors": args.actors, "knn": args.knn, "voxel_size": args.voxel_size,
           "sources": lrt_build.init_source_hash()}
    with tempfile.TemporaryDirectory() as tmp:
        write_analytic_sequence(tmp, args.height, args.width, args.frames, args.actors, noise=0.01)
        seq = sequence.load_sequence(tmp, dev)
        rf = seq.frames
        f0 = seq.train_frames[0]
        o, d = rf.rays[f0]
        si.estimate_normals(o, d, rf.get_depth(f0), rf.get_mask(f0), args.knn)        # loads the library, warms the allocator
        t_n = t_a = 0.0
        bg = []
        for f in seq.train_frames:
            o, d = rf.rays[f]
            depth, mask = rf.get_depth(f), rf.get_mask(f)
            ms, (nrm, _) = _gpu_ms(lambda: si.estimate_normals(o, d, depth, mask, args.knn)); t_n += ms
            pts = o + d * depth[..., None]
            tab = si.frame_pose_table(seq.boxes, f, dev)
            ms, (lab, lp, ln) = _gpu_ms(lambda: si.assign_to_boxes(pts, nrm, mask, *tab)); t_a += ms
            sel = torch.nonzero(lab.reshape(-1) == 0).squeeze(1)
            bg.append((lp.reshape(-1, 3)[sel], rf.get_intensity(f).reshape(-1)[sel], ln.reshape(-1, 3)[sel]))
        P, I, N = (torch.cat([b[i] for b in bg]) for i in range(3))
        t_v, vox = _gpu_ms(lambda: si.voxel_downsample(P, I, N, args.voxel_size))
        # the grid Chamfer search on the same frame (prediction = ground truth + 3 cm): the kernel the self-k-NN is judged against
        depth, mask = rf.get_depth(f0), rf.get_mask(f0)
        o, d = rf.rays[f0]
        ra = depth + 0.03 * torch.randn_like(depth)
        grid_chamfer.grid_chamfer_nearest(o, d, ra, depth, mask)
        t_gc, _ = _gpu_ms(lambda: grid_chamfer.grid_chamfer_nearest(o, d, ra, depth, mask), reps=5)
        t_n1, _ = _gpu_ms(lambda: si.estimate_normals(o, d, depth, mask, args.knn), reps=5)
        t0 = time.perf_counter(); clouds = si.init_clouds(seq, k=args.knn, voxel_size=args.voxel_size); torch.cuda.synchronize()
        res.update({"gpu_ms": {"normals_all_frames": round(t_n, 3), "normals_per_frame": round(t_n1, 3), "assign_all_frames": round(t_a, 3),
                               "voxel_mean_incl_sort": round(t_v, 3), "grid_chamfer_forward_same_frame": round(t_gc, 3)},
                    "launches": {"normals": 3, "assign": 1, "voxel_keys": 3, "voxel_mean": 5, "torch_sort": "torch.sort(stable=True) + one cast"},
                    "init_clouds_wall_s": round(time.perf_counter() - t0, 3), "returns": int(P.shape[0]), "voxels": int(vox[0].shape[0]),
                    "actor_real_returns": [int(clouds[f"actor_{a:02d}"]["real"]) for a in range(args.actors)]})
        if args.reference_frames > 0:
            cpu = sequence.load_sequence(tmp, "cpu", frames=seq.train_frames[:args.reference_frames])
            crf = cpu.frames
            tn = ta = 0.0
            cb = []
            for f in cpu.train_frames:
                o, d = crf.rays[f]
                pts = o + d * crf.get_depth(f)[..., None]
                vi = torch.nonzero(crf.get_mask(f).reshape(-1)).squeeze(1)
                q = vi[torch.randperm(vi.shape[0], generator=torch.Generator().manual_seed(0))[:4096]]
                # the brute-force search is quadratic: timed on 4096 queries against all candidates and scaled to the frame's valid pixels
                t0 = time.perf_counter(); nb = si.neighbours_reference(pts, crf.get_mask(f), args.knn, queries=q); dt = time.perf_counter() - t0
                t0 = time.perf_counter(); si.normals_from_lists_reference(pts.reshape(-1, 3)[q], o.reshape(-1, 3)[q], torch.ones(q.shape[0]), nb * 0); dt2 = time.perf_counter() - t0
                tn += (dt + dt2) * vi.shape[0] / max(1, q.shape[0])
                nrm = torch.zeros_like(pts)
                tab = si.frame_pose_table(cpu.boxes, f, "cpu")
                t0 = time.perf_counter(); lab, lp, ln = si.assign_to_boxes_reference(pts, nrm, crf.get_mask(f), *tab); ta += time.perf_counter() - t0
            t0 = time.perf_counter(); si.voxel_downsample_reference(P.cpu(), I.cpu(), N.cpu(), args.voxel_size); tv = time.perf_counter() - t0
            res["cpu_reference_s"] = {"frames": args.reference_frames, "normals_per_frame_scaled_from_4096_queries": round(tn / args.reference_frames, 3),
                                      "assign_per_frame": round(ta / args.reference_frames, 4), "voxel_mean_all_returns": round(tv, 3)}
    print(json.dumps(res))
    print(resources.table_md(resources.kernel_resources(lrt_build.INIT_LIB)))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
