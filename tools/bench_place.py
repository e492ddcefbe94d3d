#!/usr/bin/env python3
"""Time the place matcher (`lidar_rt_amd/place.py`, `liblrt_place.so`): `describe` and `match` against the same rule as torch expressions, and
`pose_graph.close_loops` and `optimize` next to `registration.odometry` on the same frames.

  describe, match   F frames of H x W in the analytic room of tests/registration_cases.py (32 seeded sensor poses, repeated to F: the matcher's
                    work does not depend on what the descriptors hold), 20 rings x 60 sectors: time per call and launches per call
  torch             the same rule without a kernel.  describe: the cell index and value of every pixel as float64 torch expressions and one
                    ``scatter_reduce(amax)``.  match: per shift a ``roll``, an ``abs`` of the difference and a ``sum``, a block of queries at a time
                    (the (queries, F, sectors, rings) difference of all queries at once does not fit), then the minimum over the shifts.  That is
                    what one writes without a kernel; it is not the code under test, and its results are compared with the operators'.

A round times ``reps`` calls of one side between two device synchronisations with the host clock; the two sides alternate round by round in one
process after a warm-up of both; the median and the 10th / 90th percentile of the rounds are reported.  A separate, untimed pass under the torch
profiler counts the launches of one call.  One JSON object on stdout, the same into ``--out``.
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

from lidar_rt_amd import build, place, pose_graph as pg, registration as rg
from tests import place_cases as pc, registration_cases as rc


def torch_describe(pts, mask, z_lo, NR, NS, r_min, r_max, z_step):
    F, H, W, _ = pts.shape
    p = pts.double()
    h = p[..., 2]
    rho = torch.sqrt(p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1])
    kept = mask & (rho >= r_min) & (rho < r_max) & (h >= z_lo)
    ring = torch.clamp(torch.floor((rho - r_min) * NR / (r_max - r_min)), max=NR - 1).long()
    value = torch.clamp(1 + torch.floor((h - z_lo) / z_step), max=255).long()
    sector = (torch.arange(W, device=pts.device) * NS // W).expand(F, H, W)
    cell = torch.where(kept, sector * place.padded(NR) + ring, torch.zeros_like(ring)).reshape(F, -1)
    out = torch.zeros((F, NS * place.padded(NR)), dtype=torch.long, device=pts.device)
    out.scatter_reduce_(1, cell, torch.where(kept, value, torch.zeros_like(value)).reshape(F, -1), "amax")
    return out.to(torch.uint8).reshape(F, NS, place.padded(NR)), out.sum(1).int()


def torch_match(desc, gap, block=32):
    F, NS, _ = desc.shape
    a = desc.to(torch.int16)
    best_d = torch.full((F, F), 2 ** 30, dtype=torch.int32, device=desc.device)
    best_s = torch.zeros((F, F), dtype=torch.int32, device=desc.device)
    for i0 in range(0, F, block):
        q = a[i0:i0 + block]
        for s in range(NS):
            D = (q.roll(-s, 1)[:, None] - a[None]).abs().sum((2, 3), dtype=torch.int32)
            better = D < best_d[i0:i0 + block]
            best_s[i0:i0 + block] = torch.where(better, torch.full_like(D, s), best_s[i0:i0 + block])
            best_d[i0:i0 + block] = torch.where(better, D, best_d[i0:i0 + block])
    i = torch.arange(F, device=desc.device)
    inside = i[None, :] + gap <= i[:, None]
    return torch.where(inside, best_d, torch.full_like(best_d, -1)), torch.where(inside, best_s, torch.full_like(best_s, -1))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--frames", type=int, nargs="*", default=[256, 1024])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-tour", action="store_true", help="leave out close_loops and optimize next to odometry")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "place.json"), help="the file the result is also written into")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_place: needs a HIP device (a timing taken anywhere else says nothing)", file=sys.stderr)
        return 2
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device("cuda", 0)
    H, W, inc = a.height, a.width, list(rc.BOUNDS)
    NR, NS, z_lo = place.DEFAULT_RINGS, place.DEFAULT_SECTORS, -1.8
    rule = dict(r_min=place.DEFAULT_R_MIN, r_max=20.0, z_step=place.DEFAULT_Z_STEP)
    res = {"bench": "place", "height": H, "width": W, "rings": NR, "sectors": NS, "rounds": a.rounds, "reps": a.reps, "torch_reps": a.torch_reps,
           "device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", "").split(":")[0],
           "sources": build.place_source_hash(), "unit": "milliseconds per call on all F frames", "frames": {}}
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
        return {"launches": int(sum(e.count for e in ev)), "k_place": int(sum(e.count for e in ev if "k_place_" in e.key)),
                "kernel_ms": sum(e.device_time_total for e in ev) / 1e3}

    d_local = rc.local_directions(H, W, inc, "KITTI", None)
    rng = np.random.default_rng(11)
    base = []
    for k in range(32):
        T = rc.exp4(np.concatenate([rng.uniform(-2.0, 2.0, size=2), [0.0, 0.0, 0.0], [rng.uniform(-math.pi, math.pi)]]))
        depth = rc.room_depth(d_local, T)
        base.append((d_local * depth[..., None], torch.isfinite(depth) & (depth > 0)))
    for F in a.frames:
        idx = [k % 32 for k in range(F)]
        pts = torch.stack([base[k][0] for k in idx]).to(dev).contiguous()
        mask = torch.stack([base[k][1] for k in idx]).to(dev).contiguous()
        gap = place.DEFAULT_GAP
        desc, sums = place.describe(pts, mask, z_lo, NR, NS, **rule)
        ops = {"describe": lambda: place.describe(pts, mask, z_lo, NR, NS, **rule), "match": lambda: place.match(desc, gap)}
        th = {"describe": lambda: torch_describe(pts, mask, z_lo, NR, NS, **rule), "match": lambda: torch_match(desc, gap)}
        for _ in range(a.warmup):
            for fn in ops.values():
                fn()
        t_desc, t_sums = th["describe"]()
        t_bd, t_bs = th["match"]()
        bd, bs = ops["match"]()
        out = {"gap": gap, "pairs": int((bd >= 0).sum()), "torch_describe_equal": bool(torch.equal(t_desc, desc) and torch.equal(t_sums, sums)),
               "torch_match_equal": bool(torch.equal(t_bd, bd) and torch.equal(t_bs, bs)), "operators": {}, "torch": {}}
        for name in ops:
            t_op, t_th = [], []
            for _ in range(a.rounds):
                t_op.append(timed(ops[name], a.reps))
                t_th.append(timed(th[name], a.torch_reps))
            out["operators"][name] = {**side(t_op), **count(ops[name])}
            out["torch"][name] = {**side(t_th), **count(th[name])}
            out[f"ratio_torch_to_{name}"] = q(t_th, 50) / q(t_op, 50)
        res["frames"][str(F)] = out
        del pts, mask
    if not a.no_tour:                                                    # what --loop-closure adds to an ingest: the nine frames of the room tour at H x W
        truth = pc.tour_truth()
        fr = {}
        for i, T in truth.items():
            depth = rc.room_depth(d_local, T)
            m = torch.isfinite(depth) & (depth > 0)
            fr[i] = rg.frame_geometry(torch.where(m, depth, torch.zeros_like(depth)).to(dev), m.to(dev), inc, H, W)
        kw = dict(inclination=inc)
        odo = lambda: rg.odometry(fr, first_pose=truth[0], return_steps=True, **kw)
        chain, rep = odo()
        loops_fn = lambda: pg.close_loops(fr, chain, rep["steps"], sensor_height=1.8, gap=pc.TOUR["gap"], r_max=pc.TOUR["r_max"], **kw)
        loops, lrep = loops_fn()
        edges = pg.odometry_edges(rep["steps"]) + loops
        opt = lambda: pg.optimize(chain, edges)
        solved, srep = opt()
        t_o, t_l, t_s = [], [], []
        for _ in range(max(a.rounds // 2, 2)):
            t_o.append(timed(odo, 1)); t_l.append(timed(loops_fn, 1)); t_s.append(timed(opt, 1))
        Zt = pc.closing_truth()
        res["tour_9_frames"] = {"odometry_ms": side(t_o), "close_loops_ms": side(t_l), "optimize_ms": side(t_s), "accepted": lrep["accepted"],
                                "rejected": len(lrep["rejected"]), "iterations": srep["iterations"],
                                "closure_chain": pg.closure_error(chain, 0, 8, Zt), "closure_solved": pg.closure_error(solved, 0, 8, Zt)}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
