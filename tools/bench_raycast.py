#!/usr/bin/env python3
"""Time the ray casting of a TSDF grid (`lidar_rt_amd/raycast.py`, `liblrt_raycast.so`) on the analytic room of tests/registration_cases.py, and
the same rule written as float64 torch expressions on the device.

  grid      16 frames of H x W (seeded sensor poses in the room, KITTI bounds) fused by ``mesh.integrate`` into a grid of X x Y x Z (20 m across)
  raycast   1 and 16 frames of H x W range rays from poses offset from the fused ones, one call each, in the rays' memory order (consecutive
            columns of a row in consecutive lanes)
  torch     the same rule without a kernel: a loop over samples on the rays that still march, each sample's cell, fractions, eight gathers,
            trilinear value and crossing test as float64 torch expressions -- what one writes without a kernel; it is not the code under test.  The
            number of rays whose (depth bits, hit, intensity bits, samples) differ from the operator's is reported; it is expected to be 0.

A round times ``reps`` calls of one side between two device synchronisations with the host clock; the two sides alternate round by round in one
process after a warm-up of both; the median and the 10th / 90th percentile of the rounds are reported.  A separate, untimed pass under the torch
profiler counts the launches of one call.  The kernel's registers and scratch come from the build's resource gate.  One JSON object on stdout, the
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

from lidar_rt_amd import build, mesh, raycast, resources
from lidar_rt_amd.training import RangeFrames
from tests import registration_cases as rc


def torch_raycast(grid, rays_o, rays_d, mw, step, far, min_depth, max_depth):
    """(depth, hit, intensity, samples) of the rule as float64 torch expressions in the rule's order, on the rays' device."""
    dev = rays_o.device
    X, Y, Z = grid.dims
    ro, rd = rays_o.reshape(-1, 3), rays_d.reshape(-1, 3)
    N = ro.shape[0]
    depth = torch.zeros(N, dtype=torch.float32, device=dev)
    hit = torch.zeros(N, dtype=torch.bool, device=dev)
    inten = torch.zeros(N, dtype=torch.float32, device=dev)
    ns = torch.zeros(N, dtype=torch.int32, device=dev)
    voxel = float(grid.voxel)
    ts, wt, it = grid.tsdf.reshape(-1), grid.weight.reshape(-1), grid.intensity.reshape(-1)
    cen = [torch.from_numpy(mesh.centres(voxel, m).astype(np.float64)).to(dev) for m in (X, Y, Z)]
    stride = torch.tensor([Y * Z, Z, 1], dtype=torch.int64, device=dev)
    dot = lambda c: (c * stride).sum(-1)                                   # an int64 product: no matmul for it on the device
    coff = dot(torch.from_numpy(raycast.CORNER).to(dev))
    hi_cell = torch.tensor([X - 2, Y - 2, Z - 2], dtype=torch.float64, device=dev)
    lerp = lambda a, b, f: a + f * (b - a)

    def tri(v, f):
        c00, c10 = lerp(v[:, 0], v[:, 1], f[:, 0]), lerp(v[:, 2], v[:, 3], f[:, 0])
        c01, c11 = lerp(v[:, 4], v[:, 5], f[:, 0]), lerp(v[:, 6], v[:, 7], f[:, 0])
        return lerp(lerp(c00, c10, f[:, 1]), lerp(c01, c11, f[:, 1]), f[:, 2])

    o = ro.double() - torch.tensor([float(x) for x in grid.origin], dtype=torch.float64, device=dev)
    d = rd.double()
    nrm = torch.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    live = torch.isfinite(ro).all(1) & torch.isfinite(rd).all(1) & (nrm > 0)
    u = d / nrm[:, None]
    tin = torch.full((N,), min_depth, dtype=torch.float64, device=dev)
    tout = torch.full((N,), max_depth, dtype=torch.float64, device=dev)
    for a in range(3):
        c0, c1 = cen[a][0], cen[a][-1]
        z = u[:, a] == 0
        live &= ~z | ((c0 <= o[:, a]) & (o[:, a] <= c1))
        t1, t2 = (c0 - o[:, a]) / u[:, a], (c1 - o[:, a]) / u[:, a]
        lo, hi = torch.where(t1 < t2, t1, t2), torch.where(t1 < t2, t2, t1)
        tin = torch.where(z, tin, torch.where(lo > tin, lo, tin))
        tout = torch.where(z, tout, torch.where(hi < tout, hi, tout))
    idx = torch.nonzero(live)[:, 0]
    o, u, t, tout = o[idx], u[idx], tin[idx], tout[idx]
    M = idx.numel()
    kp = torch.zeros(M, dtype=torch.bool, device=dev)
    tp, Dp = torch.zeros(M, dtype=torch.float64, device=dev), torch.zeros(M, dtype=torch.float64, device=dev)
    cp, fp = torch.zeros((M, 3), dtype=torch.int64, device=dev), torch.zeros((M, 3), dtype=torch.float64, device=dev)
    cnt = torch.zeros(M, dtype=torch.int32, device=dev)
    act = torch.arange(M, device=dev)
    while True:
        act = act[t[act] <= tout[act]]
        if act.numel() == 0:
            break
        ta = t[act]
        p = o[act] + ta[:, None] * u[act]
        fi = torch.floor(p / voxel - 0.5)
        c = torch.where(fi > 0, torch.where(fi > hi_cell, hi_cell.expand_as(fi), fi), torch.zeros_like(fi)).long()
        ca = torch.stack([cen[a][c[:, a]] for a in range(3)], 1)
        cb = torch.stack([cen[a][c[:, a] + 1] for a in range(3)], 1)
        f = ((p - ca) / (cb - ca)).clamp(0.0, 1.0)
        cnt[act] += 1
        base = dot(c)
        vi = base[:, None] + coff[None]
        v = ts[vi]
        known = (wt[vi] >= mw).all(1)
        ones = (v == 1.0).all(1)
        D = torch.where(known, tri(v.double(), f), torch.zeros_like(ta))
        crossing = known & kp[act] & (Dp[act] > 0) & (D <= 0)
        k = act[crossing]
        w = Dp[k] / (Dp[k] - D[crossing])
        r = idx[k]
        depth[r] = (tp[k] + (ta[crossing] - tp[k]) * w).float()
        hit[r] = True
        Ip = tri(it[dot(cp[k])[:, None] + coff[None]].double(), fp[k])
        Ik = tri(it[base[crossing][:, None] + coff[None]].double(), f[crossing])
        inten[r] = (Ip + (Ik - Ip) * w).float()
        ns[r] = cnt[k]
        kp[act] = known
        upd = known & ~crossing
        au = act[upd]
        tp[au], Dp[au], cp[au], fp[au] = ta[upd], D[upd], c[upd], f[upd]
        t[act] = torch.where(crossing, torch.full_like(ta, math.inf), ta + torch.where(known & ones, torch.full_like(ta, far), torch.full_like(ta, step)))
    done = ~hit[idx]
    ns[idx[done]] = cnt[done]
    return depth, hit, inten, ns


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=16, help="frames fused into the grid")
    ap.add_argument("--casts", default="1,16", help="frames per cast call")
    ap.add_argument("--grids", default="256x256x32,512x512x64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "raycast.json"), help="the file the result is also written into")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_raycast: needs a HIP device (a timing taken anywhere else says nothing)", file=sys.stderr)
        return 2
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device("cuda", 0)
    H, W, F, inc = a.height, a.width, a.frames, list(rc.BOUNDS)
    casts = [int(v) for v in a.casts.split(",")]
    lib = build.build_raycast()
    kres = resources.kernel_resources(lib)
    res = {"bench": "raycast", "height": H, "width": W, "fused_frames": F, "rounds": a.rounds, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "sources": build.raycast_source_hash(), "unit": "milliseconds per call", "ray_order": "memory order: consecutive columns of a row",
           "grids": {}, "kernels": {n: {k: kres[n][k] for k in ("vgpr", "sgpr", "vgpr_spill", "scratch_bytes", "lds_bytes", "waves_per_simd")}
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
        return {"launches": int(sum(e.count for e in ev if "memcpy" not in e.key.lower())), "k_raycast": int(sum(e.count for e in ev if "k_raycast" in e.key)),
                "kernel_ms": sum(e.device_time_total for e in ev if "k_raycast" in e.key) / 1e3}

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
    ro, rd = [], []
    for f in range(max(casts)):                                           # the cast poses: the fused ones moved by up to 0.5 m and turned by up to 0.3 rad
        P = poses[f % F] @ rc.exp4(np.concatenate([rng.uniform(-0.5, 0.5, size=2), [0.0, 0.0, 0.0], [rng.uniform(-0.3, 0.3)]]))
        o, d = RangeFrames.range_rays(H, W, inc, torch.as_tensor(P, dtype=torch.float32), "KITTI", None)
        ro.append(o); rd.append(d)
    ro, rd = torch.stack(ro).contiguous().to(dev), torch.stack(rd).contiguous().to(dev)
    for spec in a.grids.split(","):
        X, Y, Z = (int(v) for v in spec.split("x"))
        voxel = 20.0 / X                                                  # 20 m across: the room's 15 x 18 m floor plan and 2.5 m above the floor
        origin = (-6.5013, -11.4027, -2.0031)
        g = mesh.TsdfGrid(origin, voxel, (X, Y, Z), device=dev)
        mesh.integrate(g, depth=depth, mask=mask, sensor2world=poses, inclination=inc, intensity=fint)
        p = raycast.params(g)
        out = {"voxel": voxel, "voxels": X * Y * Z, "observed": int((g.weight > 0).sum()), "trunc": g.trunc, "step": p[1], "far_step": p[2], "casts": {}}
        for nf in casts:
            o, d = ro[:nf], rd[:nf]
            ops = {"raycast": lambda: raycast.raycast(g, o, d, samples=True), "torch_raycast": lambda: torch_raycast(g, o, d, *p)}
            for _ in range(a.warmup):
                for fn in ops.values():
                    fn()
            r, th = ops["raycast"](), ops["torch_raycast"]()
            diff = ((r.depth.reshape(-1).view(torch.int32) != th[0].view(torch.int32)) | (r.hit.reshape(-1) != th[1])
                    | (r.intensity.reshape(-1).view(torch.int32) != th[2].view(torch.int32)) | (r.samples.reshape(-1) != th[3]))
            s = r.samples.reshape(-1).double()
            times = {k: [] for k in ops}
            for _ in range(a.rounds):
                for k, fn in ops.items():
                    times[k].append(timed(fn, a.reps if k == "raycast" else 1))
            c = {"rays": int(o.numel() // 3), "hit_fraction": float(r.hit.float().mean()),
                 "samples_per_ray": {"mean": float(s.mean()), "p99": float(torch.quantile(s[:: max(1, s.numel() // (1 << 20))], 0.99)), "max": float(s.max())},
                 "torch_rays_differing": int(diff.sum()), "operators": {k: {**side(times[k]), **count(ops[k])} for k in ops}}
            c["rays_per_second"] = c["rays"] / (q(times["raycast"], 50) * 1e-3)
            c["ratio_torch_to_raycast"] = q(times["torch_raycast"], 50) / q(times["raycast"], 50)
            out["casts"][str(nf)] = c
            del r, th, diff
        res["grids"][spec] = out
        del g
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
