#!/usr/bin/env python3
"""Time the scan-to-map registration (`lidar_rt_amd/map_registration.py`, `liblrt_mapreg.so`) next to the scan-to-scan registration
(`registration.align`, `liblrt_reg.so`) on the same frames: the analytic room of tests/registration_cases.py, as tools/bench_sweepfuse.py sets it up.

  map    align_to_grid, F frames of H x W against a grid of X x Y x Z fused (mesh.integrate) from the frames of the start poses, DEFAULT_ITERS iterations
  scan   registration.align, the same F frames against the frames of their start poses, the default schedule (14 iterations)

Every source frame stands 0.25 m and 1.5 degrees from its start pose.  A round times ``reps`` calls of one side between two device
synchronisations with the host clock; the sides alternate round by round in one process after a warm-up of both; the median and the 10th / 90th
percentile of the rounds are reported, per call and per iteration.  A separate, untimed pass under the torch profiler counts the launches of one
call and sums the kernels' device time.  The result is reported, not gated.  One JSON object on stdout, the same into ``--out``.
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

from lidar_rt_amd import build, map_registration as mr, mesh, registration as rg, resources
from tests import registration_cases as rc


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--frames", default="1,16")
    ap.add_argument("--grids", default="256x256x32,512x512x64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "map_registration.json"), help="the file the result is also written into")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_mapreg: needs a HIP device (a timing taken anywhere else says nothing)", file=sys.stderr)
        return 2
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device("cuda", 0)
    H, W, inc = a.height, a.width, list(rc.BOUNDS)
    counts = [int(x) for x in a.frames.split(",")]
    Fmax = max(counts)
    kres = {**resources.kernel_resources(build.build_mapreg()), **resources.kernel_resources(build.build_reg())}
    res = {"bench": "map_registration", "height": H, "width": W, "rounds": a.rounds, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "sources": build.mapreg_source_hash(), "reg_sources": build.reg_source_hash(), "unit": "milliseconds per call", "iterations": {"map": mr.DEFAULT_ITERS,
           "scan": len(rg.DEFAULT_SCHEDULE)}, "grids": {},
           "kernels": {n: {k: kres[n][k] for k in ("vgpr", "sgpr", "vgpr_spill", "scratch_bytes", "lds_bytes", "waves_per_simd")}
                       for n in ("k_mapreg_linearize", "k_mapreg_solve", "k_reg_linearize", "k_reg_solve")}}
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
        own = lambda e: "k_mapreg_" in e.key or "k_reg_" in e.key
        return {"launches": int(sum(e.count for e in ev if "memcpy" not in e.key.lower())), "kernels": int(sum(e.count for e in ev if own(e))),
                "kernel_ms": sum(e.device_time_total for e in ev if own(e)) / 1e3}

    d_local = rc.local_directions(H, W, inc, "KITTI", None)
    rng = np.random.default_rng(5)
    depth, mask, start, truth, src, tgt = [], [], [], [], [], []
    for f in range(Fmax):
        P = rc.exp4(np.concatenate([rng.uniform(-2.0, 2.0, size=2), [0.0, 0.0, 0.0], [rng.uniform(-np.pi, np.pi)]]))
        T = P @ rc.exp4(rc.twist(60 + f, 0.25, 1.5))
        for pose, geo in ((P, tgt), (T, src)):
            d = rc.room_depth(d_local, pose)
            m = torch.isfinite(d) & (d > 0)
            d = torch.where(m, d, torch.zeros_like(d)).to(dev)
            geo.append(rg.frame_geometry(d, m.to(dev), inc, H, W))
            if geo is tgt:
                depth.append(d); mask.append(m.to(dev))
        start.append(P); truth.append(T)
    depth, mask = torch.stack(depth), torch.stack(mask)
    sp, sm = torch.stack([g[0] for g in src]), torch.stack([g[2] for g in src])
    tp, tn, tm = (torch.stack([g[k] for g in tgt]) for k in range(3))
    origin = (-6.5013, -11.4027, -2.0031)
    for spec in a.grids.split(","):
        X, Y, Z = (int(v) for v in spec.split("x"))
        voxel = 20.0 / X                                                  # 20 m across: the room's 15 x 18 m floor plan and 2.5 m above the floor
        grid = mesh.TsdfGrid(origin, voxel, (X, Y, Z), 4.0 * voxel, device=dev, intensity=False)
        mesh.integrate(grid, depth, mask, np.stack(start), inc)
        X0 = torch.from_numpy(np.ascontiguousarray(mr.grid_pose(grid, np.stack(start))[:, :3])).to(dev)
        Xt = mr.grid_pose(grid, np.stack(truth))[:, :3]
        out = {"voxel": voxel, "trunc": 4.0 * voxel, "voxels": X * Y * Z, "observed": int((grid.weight > 0).sum()), "frames": {}}
        for F in counts:
            ws_m = torch.empty(mr.work_bytes(F, H, W), dtype=torch.uint8, device=dev)
            ws_s = torch.empty(rg.work_bytes(F, H, W), dtype=torch.uint8, device=dev)
            ops = {"map": lambda: mr.align_to_grid(grid, (sp[:F], sm[:F]), X0[:F], workspace=ws_m),
                   "scan": lambda: rg.align((sp[:F], sm[:F]), (tp[:F], tn[:F], tm[:F]), None, inclination=inc, workspace=ws_s)}
            for _ in range(a.warmup):
                for fn in ops.values():
                    fn()
            times = {k: [] for k in ops}
            for _ in range(a.rounds):
                for k, fn in ops.items():
                    times[k].append(timed(fn, a.reps))
            reg = ops["map"]()
            err = [rc.pose_error(reg.X[f].cpu().numpy(), Xt[f]) for f in range(F)]
            row = {k: {**side(times[k]), "per_iteration": q(times[k], 50) / res["iterations"][k], **count(ops[k])} for k in ops}
            row["ratio_map_to_scan"] = q(times["map"], 50) / q(times["scan"], 50)
            row["map_status"] = reg.status.cpu().tolist()
            row["map_terms"] = [int(x) for x in reg.log[:, -1, 0].cpu().tolist()]
            row["map_error"] = {"translation_max": max(e[0] for e in err), "rotation_max": max(e[1] for e in err)}
            out["frames"][str(F)] = row
        res["grids"][spec] = out
        del grid
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
