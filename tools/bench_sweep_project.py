#!/usr/bin/env python3
"""Time the range-image projection under the sweep model (`lidar_rt_amd.sweep_project.project_points_sweep`, `liblrt_sweepproj.so`).

    python tools/bench_sweep_project.py [--rounds 7] [--calls 50] [--out FILE.json]

One 64 x 2048 frame of 131,072 points, and a batch of 16 such frames, seeded `randn * (20, 20, 2)` metres, KITTI bounds, the twist MODERATE =
(1.5, 0.2, 0, 0, 0, 0.05).  Three variants on the same points, alternated round by round, `--calls` calls per round between two device events,
the median over the rounds of the time per call:

    sweep      project_points_sweep with the twist: the column table, up to eight evaluations per point
    no_twist   project_points_sweep(twist=None): the same kernels without the table, one evaluation per point
    static     range_image.project_points: what there was before -- a lower bound, one evaluation and no table

Before anything is timed the operator's result is compared with the float64 twin's bit for bit; the twin is timed once on the CPU.  Prints one JSON object."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lidar_rt_amd import build as lrt_build, range_image as ri, sweep_project as sp      # noqa: E402

MODERATE = (1.5, 0.2, 0.0, 0.0, 0.0, 0.05)
H, W, POINTS = 64, 2048, 131_072
INC = [math.radians(-24.9), math.radians(2.0)]


def one(F, rounds, calls, dev):
    rng = np.random.default_rng([7, F])
    pts = np.concatenate([rng.standard_normal((F * POINTS, 3)) * (20.0, 20.0, 2.0), rng.uniform(0, 1, (F * POINTS, 1))], 1).astype(np.float32)
    offsets = np.arange(F + 1, dtype=np.int64) * POINTS
    kw = dict(H=H, W=W, inclination=INC, offsets=offsets)
    twist = np.array(MODERATE)
    t0 = time.perf_counter()
    tw = sp.project_points_sweep_reference(pts, twist=twist, **kw)
    twin_s = time.perf_counter() - t0
    d = torch.tensor(pts, device=dev)
    ws = torch.empty(sp.work_bytes(F, H, W), dtype=torch.uint8, device=dev)
    variants = {"sweep": lambda: sp.project_points_sweep(d, twist=twist, **kw, workspace=ws),
                "no_twist": lambda: sp.project_points_sweep(d, twist=None, **kw, workspace=ws),
                "static": lambda: ri.project_points(d, **kw, workspace=ws)}
    op = variants["sweep"]()
    torch.cuda.synchronize()
    equal = all(torch.equal(a.cpu(), b) for a, b in zip(op, tw))
    st, nt = variants["static"](), variants["no_twist"]()
    torch.cuda.synchronize()
    zero_motion_equal = all(torch.equal(getattr(st, k), getattr(nt, k)) for k in ("depth", "intensity", "mask", "index"))
    for fn in variants.values():                                              # warm every shape the timed window uses
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():                                        # alternating: the variants share whatever else the machine does
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / calls)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return dict(frames=F, points=F * POINTS, pixels=F * H * W, counts=dict(zip(sp.COUNT_NAMES, tw.counts.sum(0).tolist())), mean_evaluations=float(tw.evals.double().mean()),
                margin=tw.margin, range_margin=tw.range_margin, equal_to_twin=equal, zero_motion_equal_to_static=zero_motion_equal,
                ms_per_call={k: dict(median=med[k], min=min(v), max=max(v)) for k, v in ms.items()}, sweep_over_static=med["sweep"] / med["static"],
                no_twist_over_static=med["no_twist"] / med["static"], twin_cpu_s=twin_s, points_per_s=F * POINTS / (med["sweep"] * 1e-3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_sweep_project: no HIP device", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    res = dict(source_hash=lrt_build.sweepproj_source_hash(), device=torch.cuda.get_device_name(dev), twist=list(MODERATE), height=H, width=W, rounds=a.rounds,
               calls_per_round=a.calls, shapes=[one(F, a.rounds, a.calls, dev) for F in (1, 16)])
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if all(r["equal_to_twin"] and r["zero_motion_equal_to_static"] for r in res["shapes"]) else 1


if __name__ == "__main__":
    sys.exit(main())
