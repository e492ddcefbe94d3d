#!/usr/bin/env python3
"""Time the range-image projection (`lidar_rt_amd.range_image.project_points`, `liblrt_project.so`) and its float64 numpy twin.

    python tools/bench_project.py [--runs 200] [--out FILE.json]

Two shapes: 16 frames of 130,000 points at 66 x 1030 (KITTI-360's grid, two inclination bounds) and 16 frames of 180,000 points at 64 x 2650
(Waymo's top LiDAR, a per-beam table and a sensor yaw).  The points are seeded `randn * (20, 20, 2)` metres.  The operator is timed between
device events around one call (the median, minimum and maximum of `--runs` calls after a warm-up), the twin once on the CPU with
`time.perf_counter`.  The operator's result is compared with the twin's before anything is timed.  Prints the library's source hash."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lidar_rt_amd import build as lrt_build, range_image as ri      # noqa: E402

SHAPES = [dict(name="16 x 130 k points, 66 x 1030, KITTI bounds", F=16, n=130_000, H=66, W=1030, data_type="KITTI",
               inclination=[math.radians(-24.9), math.radians(2.0)], sensor2ego=None),
          dict(name="16 x 180 k points, 64 x 2650, Waymo table and yaw", F=16, n=180_000, H=64, W=2650, data_type="Waymo",
               inclination=np.linspace(-0.305, 0.04, 64).tolist(),
               sensor2ego=[[math.cos(0.3), -math.sin(0.3), 0, 1.4], [math.sin(0.3), math.cos(0.3), 0, 0], [0, 0, 1, 2.1], [0, 0, 0, 1]])]


def one(shape, runs, dev):
    rng = np.random.default_rng(7)
    F, n, H, W = shape["F"], shape["n"], shape["H"], shape["W"]
    pts = np.concatenate([rng.standard_normal((F * n, 3)) * (20.0, 20.0, 2.0), rng.uniform(0, 1, (F * n, 1))], 1).astype(np.float32)
    offsets = np.arange(F + 1, dtype=np.int64) * n
    kw = dict(H=H, W=W, inclination=shape["inclination"], offsets=offsets, data_type=shape["data_type"], sensor2ego=shape["sensor2ego"])
    t0 = time.perf_counter()
    tw = ri.project_points_reference(pts, **kw)
    twin_s = time.perf_counter() - t0
    d = torch.tensor(pts, device=dev)
    ws = torch.empty(ri.work_bytes(F, H, W), dtype=torch.uint8, device=dev)
    op = ri.project_points(d, **kw, workspace=ws)
    torch.cuda.synchronize()
    equal = all(torch.equal(a.cpu(), b) for a, b in zip(op, tw))
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ri.project_points(d, **kw, workspace=ws)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    c = tw.counts.sum(0).tolist()
    # bytes: the points read once by the scatter (16 B), one key word written by the fill, read by the resolve (8 + 8 B per pixel), 13 B of
    # outputs per pixel, the atomics' words not counted
    model = F * n * 16 + F * H * W * (8 + 8 + 13)
    return dict(shape=shape["name"], points=F * n, pixels=F * H * W, counts=dict(zip(ri.COUNT_NAMES, c)), margin=tw.margin, equal_to_twin=equal,
                operator_ms=dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1], runs=runs), twin_cpu_s=twin_s, model_bytes=model,
                model_gb_per_s=model / (ms[len(ms) // 2] * 1e-3) / 1e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_project: no HIP device", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    res = dict(source_hash=lrt_build.project_source_hash(), device=torch.cuda.get_device_name(dev), shapes=[one(s, a.runs, dev) for s in SHAPES])
    print(f"liblrt_project.so sources {res['source_hash']} on {res['device']}")
    for r in res["shapes"]:
        m = r["operator_ms"]
        print(f"{r['shape']}: operator {m['median']:.3f} ms (min {m['min']:.3f}, max {m['max']:.3f}, {m['runs']} calls), twin on the CPU {r['twin_cpu_s']:.2f} s; "
              f"{r['counts']['pixels']} pixels, {r['counts']['hidden']} hidden; equal to the twin: {r['equal_to_twin']}; margin {r['margin']:.2e}; "
              f"byte model {r['model_bytes'] / 1e6:.1f} MB -> {r['model_gb_per_s']:.0f} GB/s")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if all(r["equal_to_twin"] for r in res["shapes"]) else 1


if __name__ == "__main__":
    sys.exit(main())
