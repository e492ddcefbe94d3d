#!/usr/bin/env python3
"""Time the surface meshes (`lidar_rt_amd/mesh.py`, `liblrt_mesh.so`): `integrate` and `extract` on the analytic room of
tests/registration_cases.py, and the integration rule written as float64 torch expressions on the device.

  integrate   16 frames of H x W (seeded sensor poses in the room, KITTI bounds) into a grid of X x Y x Z covering the room's floor half, one call
  extract     on the grid that call left (count + scan, one host read of the totals, vertices + faces)
  torch       the same rule without a kernel: per frame the transform, range, azimuth and elevation of every voxel centre as float64 torch
              expressions, a gather of its pixel and the running means -- what one writes without a kernel; it is not the code under test.  The
              number of voxels whose (tsdf, weight, intensity) bits differ from the operator's is reported (atan2 and hypot of torch and of the
              device library may differ in the last bit; the expressions' order is the rule's).

A round times ``reps`` calls of one side between two device synchronisations with the host clock; the two sides alternate round by round in one
process after a warm-up of both; the median and the 10th / 90th percentile of the rounds are reported.  A separate, untimed pass under the torch
profiler counts the launches of one call.  The kernels' registers and scratch come from the build's resource gate.  One JSON object on stdout, the
same into ``--out``.
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

from lidar_rt_amd import build, mesh, range_image as ri, resources
from tests import registration_cases as rc


def torch_integrate(grid, T, depth, mask, fint, inc, off, yaw, min_depth, max_depth):
    """(tsdf, weight, intensity) after one call, as float64 torch expressions in the rule's order."""
    X, Y, Z = grid.dims
    dev = depth.device
    F, H, W = depth.shape
    cen = [torch.from_numpy(mesh.centres(grid.voxel, n).astype(np.float64)).to(dev) for n in (X, Y, Z)]
    x0, y0, z0 = (t.reshape(-1) for t in torch.meshgrid(*cen, indexing="ij"))
    D, Wt, I = grid.tsdf.reshape(-1).double(), grid.weight.reshape(-1).double(), grid.intensity.reshape(-1).double()
    seen = torch.zeros_like(D, dtype=torch.bool)
    trunc = grid.trunc
    for f in range(F):
        t = T[f]
        x = t[0, 0] * x0 + t[0, 1] * y0 + t[0, 2] * z0 + t[0, 3]
        y = t[1, 0] * x0 + t[1, 1] * y0 + t[1, 2] * z0 + t[1, 3]
        z = t[2, 0] * x0 + t[2, 1] * y0 + t[2, 2] * z0 + t[2, 3]
        r = torch.sqrt(x * x + y * y + z * z)
        rd = r.float().double()
        ok = (r != 0) & (rd > min_depth) & (rd <= max_depth)
        az, el = torch.atan2(y, x), torch.atan2(z, torch.hypot(x, y))
        w = torch.round((math.pi - (az + yaw)) * W / (2 * math.pi) - off)
        w = w - torch.floor(w / W) * W
        h = torch.round(H - off - (el - inc[0]) / (inc[1] - inc[0]) * H)
        ok &= (w >= 0) & (w < W) & (h >= 0) & (h < H)
        p = torch.where(ok, h * W + w, torch.zeros_like(h)).long()
        dep = depth[f].reshape(-1)[p]
        ok &= mask[f].reshape(-1)[p] & (dep > 0)
        sdf = dep.double() - rd
        ok &= sdf >= -trunc
        d = torch.clamp(sdf / trunc, max=1.0)
        D = torch.where(ok, (Wt * D + d) / (Wt + 1.0), D)
        I = torch.where(ok, (Wt * I + fint[f].reshape(-1)[p].double()) / (Wt + 1.0), I)
        Wt = torch.where(ok, Wt + 1.0, Wt)
        seen |= ok
    return (torch.where(seen, D.float(), grid.tsdf.reshape(-1)), torch.where(seen, Wt.int(), grid.weight.reshape(-1)),
            torch.where(seen, I.float(), grid.intensity.reshape(-1)))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--grids", default="256x256x32,512x512x64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh.json"), help="the file the result is also written into")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_mesh: needs a HIP device (a timing taken anywhere else says nothing)", file=sys.stderr)
        return 2
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device("cuda", 0)
    H, W, F, inc = a.height, a.width, a.frames, list(rc.BOUNDS)
    lib = build.build_mesh()
    kres = resources.kernel_resources(lib)
    res = {"bench": "mesh", "height": H, "width": W, "frames": F, "rounds": a.rounds, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "sources": build.mesh_source_hash(), "unit": "milliseconds per call", "grids": {},
           "kernels": {n: {k: kres[n][k] for k in ("vgpr", "sgpr", "vgpr_spill", "scratch_bytes", "lds_bytes", "waves_per_simd")}
                       for n in sorted(kres) if resources.is_own_kernel(n)}}
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
        return {"launches": int(sum(e.count for e in ev if "memcpy" not in e.key.lower())), "k_mesh": int(sum(e.count for e in ev if "k_mesh_" in e.key)),
                "kernel_ms": sum(e.device_time_total for e in ev if "k_mesh_" in e.key) / 1e3}

    d_local = rc.local_directions(H, W, inc, "KITTI", None)
    rng = np.random.default_rng(5)
    depth, mask, fint, poses = [], [], [], []
    for f in range(F):
        P = rc.exp4(np.concatenate([rng.uniform(-2.0, 2.0, size=2), [0.0, 0.0, 0.0], [rng.uniform(-math.pi, math.pi)]]))
        d = rc.room_depth(d_local, P)
        m = torch.isfinite(d) & (d > 0)
        depth.append(torch.where(m, d, torch.zeros_like(d))); mask.append(m); poses.append(P)
        fint.append(torch.from_numpy(rng.uniform(0, 1, (H, W)).astype(np.float32)))
    depth, mask, fint = torch.stack(depth).to(dev), torch.stack(mask).to(dev), torch.stack(fint).to(dev)
    poses = np.stack(poses)
    off, yaw = ri.convention("KITTI", None)
    for spec in a.grids.split(","):
        X, Y, Z = (int(v) for v in spec.split("x"))
        voxel = 20.0 / X                                                  # 20 m across: the room's 15 x 18 m floor plan and 2.5 m above the floor
        origin = (-6.5013, -11.4027, -2.0031)
        fresh = lambda: mesh.TsdfGrid(origin, voxel, (X, Y, Z), device=dev)
        g = fresh()
        kw = dict(depth=depth, mask=mask, sensor2world=poses, inclination=inc, intensity=fint)
        mesh.integrate(g, **kw)
        T = torch.from_numpy(mesh.grid2sensor(origin, poses)).to(dev)
        th = torch_integrate(fresh(), T, depth, mask, fint, inc, off, yaw, 0.0, 80.0)
        diff = ((th[0].view(torch.int32) != g.tsdf.reshape(-1).view(torch.int32)) | (th[1] != g.weight.reshape(-1))
                | (th[2].view(torch.int32) != g.intensity.reshape(-1).view(torch.int32)))
        work = fresh()
        ops = {"integrate": lambda: mesh.integrate(work, **kw), "extract": lambda: mesh.extract(g),
               "torch_integrate": lambda: torch_integrate(work, T, depth, mask, fint, inc, off, yaw, 0.0, 80.0)}
        for _ in range(a.warmup):
            for fn in ops.values():
                fn()
        m = mesh.extract(g)
        times = {k: [] for k in ops}
        for _ in range(a.rounds):
            for k, fn in ops.items():
                times[k].append(timed(fn, a.reps if k != "torch_integrate" else 1))
        out = {"voxel": voxel, "voxels": X * Y * Z, "observed": int((g.weight > 0).sum()), "vertices": int(m.vertices.shape[0]),
               "faces": int(m.faces.shape[0]), "torch_voxels_differing": int(diff.sum()), "operators": {}}
        for k in ops:
            out["operators"][k] = {**side(times[k]), **count(ops[k])}
        out["ratio_torch_to_integrate"] = q(times["torch_integrate"], 50) / q(times["integrate"], 50)
        res["grids"][spec] = out
        del g, work, th, diff
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
