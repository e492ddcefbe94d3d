#!/usr/bin/env python3
"""Time the TSDF fusion under the sweep model (`lidar_rt_amd/sweep_fuse.py`, `liblrt_sweepfuse.so`) against the static fusion (`mesh.integrate`,
`liblrt_mesh.so`) on the same inputs: the analytic room of tests/registration_cases.py, as tools/bench_mesh.py sets it up.

  sweep_moving   integrate_sweep, 16 frames of H x W into a grid of X x Y x Z, every frame with the MODERATE twist of tests/sweep_project_cases.py
  sweep_zero     integrate_sweep on the same inputs with zero twists: the column table is the identity, every search takes one evaluation
  static         mesh.integrate on the same inputs: the yardstick

A round times ``reps`` calls of one side between two device synchronisations with the host clock; the three sides alternate round by round in
one process after a warm-up of all; the median and the 10th / 90th percentile of the rounds are reported, and the ratios of the medians to the
static side's.  A separate, untimed pass under the torch profiler counts the launches of one call and sums the kernels' device time.  As context
the numpy twin's mean number of evaluations per searched voxel-frame on a small grid (the same frames and twists) is reported: the expectation
for sweep_moving is the static time times roughly that mean plus one.  The kernels' registers and scratch come from the build's resource gate.
One JSON object on stdout, the same into ``--out``.
"""
import argparse
import json
import math
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np
import torch

from lidar_rt_amd import build, mesh, resources, sweep_fuse
from tests import registration_cases as rc
from tests import sweep_project_cases as spc


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--grids", default="256x256x32,512x512x64")
    ap.add_argument("--small", default="32x32x8", help="the grid of the twin's evaluation count")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sweep_fuse.json"), help="the file the result is also written into")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_sweepfuse: needs a HIP device (a timing taken anywhere else says nothing)", file=sys.stderr)
        return 2
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device("cuda", 0)
    H, W, F, inc = a.height, a.width, a.frames, list(rc.BOUNDS)
    lib, lib_mesh = build.build_sweepfuse(), build.build_mesh()
    kres = {**resources.kernel_resources(lib), **resources.kernel_resources(lib_mesh)}
    res = {"bench": "sweep_fuse", "height": H, "width": W, "frames": F, "rounds": a.rounds, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "sources": build.sweepfuse_source_hash(), "mesh_sources": build.mesh_source_hash(), "twist": list(spc.MODERATE), "unit": "milliseconds per call",
           "grids": {}, "kernels": {n: {k: kres[n][k] for k in ("vgpr", "sgpr", "vgpr_spill", "scratch_bytes", "lds_bytes", "waves_per_simd")}
                                    for n in ("k_sf_table", "k_sf_fuse", "k_mesh_integrate")}}
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
        own = lambda e: "k_sf_" in e.key or "k_mesh_" in e.key
        return {"launches": int(sum(e.count for e in ev if "memcpy" not in e.key.lower())), "kernels": int(sum(e.count for e in ev if own(e))),
                "kernel_ms": sum(e.device_time_total for e in ev if own(e)) / 1e3}

    d_local = rc.local_directions(H, W, inc, "KITTI", None)
    rng = np.random.default_rng(5)
    depth, mask, fint, poses = [], [], [], []
    for f in range(F):
        P = rc.exp4(np.concatenate([rng.uniform(-2.0, 2.0, size=2), [0.0, 0.0, 0.0], [rng.uniform(-math.pi, math.pi)]]))
        d = rc.room_depth(d_local, P)
        m = torch.isfinite(d) & (d > 0)
        depth.append(torch.where(m, d, torch.zeros_like(d))); mask.append(m); poses.append(P)
        fint.append(torch.from_numpy(rng.uniform(0, 1, (H, W)).astype(np.float32)))
    depth, mask, fint = torch.stack(depth), torch.stack(mask), torch.stack(fint)
    poses = np.stack(poses)
    moving, zero = np.tile(np.array(spc.MODERATE, np.float64), (F, 1)), np.zeros((F, 6))
    origin = (-6.5013, -11.4027, -2.0031)

    # the twin's evaluation count on a small grid: context for the ratio
    X, Y, Z = (int(v) for v in a.small.split("x"))
    small = mesh.TsdfGrid(origin, 20.0 / X, (X, Y, Z))
    tw = sweep_fuse.integrate_sweep_reference(small, depth, mask, poses, inc, moving, intensity=fint)
    searched = int(tw.evals[1:].sum())
    res["twin"] = {"grid": a.small, "voxel_frames": X * Y * Z * F, "searched": searched, "fused": tw.fused, "unseen": tw.unseen,
                   "evals": [int(x) for x in tw.evals], "mean_evals": float((np.arange(tw.evals.size) * tw.evals).sum() / max(searched, 1))}

    depth, mask, fint = depth.to(dev), mask.to(dev), fint.to(dev)
    for spec in a.grids.split(","):
        X, Y, Z = (int(v) for v in spec.split("x"))
        voxel = 20.0 / X                                                  # 20 m across: the room's 15 x 18 m floor plan and 2.5 m above the floor
        fresh = lambda: mesh.TsdfGrid(origin, voxel, (X, Y, Z), device=dev)
        kw = dict(depth=depth, mask=mask, sensor2world=poses, inclination=inc, intensity=fint)
        ws = torch.empty(sweep_fuse.work_bytes(F, W), dtype=torch.uint8, device=dev)
        gs, gz, gm = fresh(), fresh(), fresh()
        mesh.integrate(gs, **kw)
        sweep_fuse.integrate_sweep(gz, twist=zero, workspace=ws, **kw)
        sweep_fuse.integrate_sweep(gm, twist=moving, workspace=ws, **kw)
        zero_differs = int(((gz.tsdf.view(torch.int32) != gs.tsdf.view(torch.int32)) | (gz.weight != gs.weight)
                            | (gz.intensity.view(torch.int32) != gs.intensity.view(torch.int32))).sum())
        out = {"voxel": voxel, "voxels": X * Y * Z, "observed_static": int((gs.weight > 0).sum()), "observed_moving": int((gm.weight > 0).sum()),
               "fused_static": int(gs.weight.sum(dtype=torch.int64)), "fused_moving": int(gm.weight.sum(dtype=torch.int64)),
               "zero_twist_voxels_differing_from_static": zero_differs, "operators": {}}
        work = fresh()
        ops = {"sweep_moving": lambda: sweep_fuse.integrate_sweep(work, twist=moving, workspace=ws, **kw),
               "sweep_zero": lambda: sweep_fuse.integrate_sweep(work, twist=zero, workspace=ws, **kw),
               "static": lambda: mesh.integrate(work, **kw)}
        for _ in range(a.warmup):
            for fn in ops.values():
                fn()
        times = {k: [] for k in ops}
        for _ in range(a.rounds):
            for k, fn in ops.items():
                times[k].append(timed(fn, a.reps))
        for k in ops:
            out["operators"][k] = {**side(times[k]), **count(ops[k])}
        base = q(times["static"], 50)
        out["ratio_to_static"] = {k: q(times[k], 50) / base for k in ("sweep_moving", "sweep_zero")}
        kbase = out["operators"]["static"]["kernel_ms"]
        out["kernel_ratio_to_static"] = {k: out["operators"][k]["kernel_ms"] / kbase for k in ("sweep_moving", "sweep_zero")}
        res["grids"][spec] = out
        del gs, gz, gm, work
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
