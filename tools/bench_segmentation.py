#!/usr/bin/env python3
"""Time the range-image segmentation (`lidar_rt_amd/segmentation.py`, `liblrt_segment.so`) operator by operator, the labelling against iterative
minimum-label propagation in torch expressions, and `actors.discover` next to `registration.odometry` on the same frames.

  operators   ``ground``, ``label``, ``freespace``, ``stats``, ``track_bounds`` on F frames of H x W: time per call and launches per call
  torch       for the labelling only: the join flags as float32 torch expressions, then ``label <- min(label, joined neighbours' labels)`` over the
              whole image until nothing changes (one host read per sweep).  That is what one writes without a kernel; it says what the loop costs
              without one, not more.

64 x 2048, F = 1 and F = 16 frames of the analytic world of tests/segment_cases.py (the room, two moving boxes and a parked one, the scenario's
trajectory).  A round times ``reps`` calls of one side between two device synchronisations with the host clock; the two sides of the labelling
alternate round by round in one process after a warm-up of both; the median and the 10th / 90th percentile of the rounds are reported.  A
separate, untimed pass under the torch profiler counts the launches of one call.  One JSON object on stdout, the same into ``--out``.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np
import torch

from lidar_rt_amd import actors, build, registration as rg, segmentation as sg
from tests import segment_cases as sc

BIG = 2 ** 31 - 1


def torch_label(pts, kept, d_abs, c_h, c_v):
    """Minimum-label propagation to convergence on (F, H, W, .) tensors: (labels int32, sweeps)."""
    F, H, W = kept.shape
    r2 = (pts * pts).sum(-1)
    da2 = torch.tensor(d_abs * d_abs, dtype=torch.float32, device=pts.device)

    def join(a, b, ra, rb, c):
        return ((a - b) ** 2).sum(-1) <= torch.maximum(da2, (c * c) * torch.minimum(ra, rb))
    jr = kept & kept.roll(-1, 2) & join(pts, pts.roll(-1, 2), r2, r2.roll(-1, 2), c_h)            # with the pixel to the right, seam included
    jd = torch.zeros_like(kept)
    jd[:, :-1] = kept[:, :-1] & kept[:, 1:] & join(pts[:, :-1], pts[:, 1:], r2[:, :-1], r2[:, 1:], c_v)
    jl, ju = jr.roll(1, 2), jd.roll(1, 1)
    big = torch.full((F, H, W), BIG, dtype=torch.int32, device=pts.device)
    lab = torch.where(kept, torch.arange(H * W, dtype=torch.int32, device=pts.device).reshape(1, H, W).expand(F, H, W), big)
    sweeps = 0
    while True:
        new = torch.minimum(lab, torch.where(jr, lab.roll(-1, 2), big))
        new = torch.minimum(new, torch.where(jl, lab.roll(1, 2), big))
        new = torch.minimum(new, torch.where(jd, lab.roll(-1, 1), big))
        new = torch.minimum(new, torch.where(ju, lab.roll(1, 1), big))
        sweeps += 1
        if torch.equal(new, lab):                                             # the host read that drives the loop
            break
        lab = new
    return torch.where(kept, lab, torch.full_like(lab, -1)), sweeps


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--frames", type=int, nargs="*", default=[1, 16])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "segmentation.json"), help="the file the result is also written into")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_segmentation: needs a HIP device (a timing taken anywhere else says nothing)", file=sys.stderr)
        return 2
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device("cuda", 0)
    H, W, inc = a.height, a.width, list(sc.rc.BOUNDS)
    c_h, c_v = sg.default_thresholds(H, W, inc)
    res = {"bench": "segmentation", "height": H, "width": W, "rounds": a.rounds, "reps": a.reps, "torch_reps": a.torch_reps, "device": torch.cuda.get_device_name(0),
           "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", "").split(":")[0], "sources": build.segment_source_hash(),
           "unit": "milliseconds per call on all F frames", "frames": {}}
    q = lambda v, p: float(np.percentile(v, p))
    side = lambda v: {"median": q(v, 50), "p10": q(v, 10), "p90": q(v, 90)}

    def timed(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    def count(fn):
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.key_averages() if e.device_time_total > 0]
        return {"launches": int(sum(e.count for e in ev)), "k_seg": int(sum(e.count for e in ev if "k_seg_" in e.key)),
                "kernel_ms": sum(e.device_time_total for e in ev) / 1e3}

    for F in a.frames:
        poses = [sc.scenario_pose(k % 8 if F > 8 else k) for k in range(F)]
        made = [sc.world_frame(H, W, inc, "KITTI", None, poses[k], sc.scenario_boxes(k % 8)) for k in range(F)]
        pts, depth, mask = (torch.stack([m[k] for m in made]).to(dev) for k in range(3))
        X = torch.eye(4, dtype=torch.float64, device=dev)[:3].expand(F, 3, 4).contiguous()
        g = sg.ground(pts, mask, sc.SENSOR_HEIGHT, inc)
        lab = sg.label(pts, mask, exclude=g, inclination=inc)
        ev = sg.freespace((pts, mask), (depth, mask), X, inclination=inc)
        st = sg.stats(pts, lab, (ev, ev), 4096)
        track_of = torch.zeros((F, 4096), dtype=torch.int32, device=dev)
        pose = X[None].contiguous()
        kept = mask & (g == 0)
        ws = torch.empty(sg.work_bytes(F, H, W), dtype=torch.uint8, device=dev)
        ops = {"ground": lambda: sg.ground(pts, mask, sc.SENSOR_HEIGHT, inc), "label": lambda: sg.label(pts, mask, exclude=g, inclination=inc),
               "freespace": lambda: sg.freespace((pts, mask), (depth, mask), X, inclination=inc), "stats": lambda: sg.stats(pts, lab, (ev, ev), 4096, workspace=ws),
               "track_bounds": lambda: sg.track_bounds(pts, st.seg, track_of, pose)}
        th = lambda: torch_label(pts, kept, sg.DEFAULT_D_ABS, c_h, c_v)
        for _ in range(a.warmup):
            for fn in ops.values():
                fn()
        t_lab, sweeps = th()
        out = {"operators": {}, "segments": st.n_seg.cpu().tolist(), "overflow": st.overflow.cpu().tolist(),
               "torch_labels_equal": bool(torch.equal(t_lab, lab)), "torch_sweeps": sweeps}
        for name, fn in ops.items():
            if name != "label":
                out["operators"][name] = {**side([timed(fn, a.reps) for _ in range(a.rounds)]), **count(fn)}
        t_op, t_th = [], []
        for _ in range(a.rounds):
            t_op.append(timed(ops["label"], a.reps))
            t_th.append(timed(th, a.torch_reps))
        out["operators"]["label"] = {**side(t_op), **count(ops["label"])}
        out["torch_label"] = {**side(t_th), **count(th)}
        out["ratio_torch_to_label"] = q(t_th, 50) / q(t_op, 50)
        res["frames"][str(F)] = out
    if 16 in a.frames:                                                 # what --discover-actors adds to an ingest: 16 frames, the trajectory twice over
        F = 16
        poses = {100 + k: sc.scenario_pose(k * 0.5) for k in range(F)}
        world = [sc.world_frame(H, W, inc, "KITTI", None, poses[100 + k], sc.scenario_boxes(k * 0.5)) for k in range(F)]
        fr = {100 + k: tuple(t.to(dev) for t in world[k][:3]) for k in range(F)}
        geo = {i: rg.frame_geometry(f[1], f[2], inc, H, W) for i, f in fr.items()}
        disc = lambda: actors.discover(fr, poses, sc.SENSOR_HEIGHT, inc)
        odo = lambda: rg.odometry(geo, inclination=inc)
        disc(); odo()
        t_d, t_o = [], []
        for _ in range(max(a.rounds // 2, 2)):
            t_d.append(timed(disc, 1))
            t_o.append(timed(odo, 1))
        boxes, rep = disc()
        res["discover_16_frames"] = {"discover_ms": side(t_d), "odometry_ms": side(t_o), "ratio_discover_to_odometry": q(t_d, 50) / q(t_o, 50),
                                     "n_actors": rep["n_actors"], "segments": rep["segments"]}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
