"""Time the actor-sweep operator against its twin's arithmetic in float32 torch, on the GPU, and print one JSON object.

    python tools/bench_actor_sweep.py [--gaussians 80000 --assets 10 --width 2048 --rounds 30 --reps 10]

Both sides advance the Gaussians of ``assets`` moving actors to the instants at which a moving sensor's sweep of ``width`` columns passes over them,
forward and backward (upstream gradients for ``xyz_s`` and ``rot_s``; gradients for ``xyz``, ``rot_raw`` and ``actor_twist``):

  torch     ``actor_sweep_reference(..., dtype=torch.float32, with_margin=False)`` on the device: the column table, eight vectorised search rounds over
            the Gaussians still searching (the compaction between rounds waits for the device, as such code does), the placement, autograd's backward
  operator  ``actor_sweep(...)``: two launches forward, two backward, float64 arithmetic, no host wait

A round times ``reps`` runs of one side between two device synchronisations with the host clock; the sides alternate round by round in one
process, after a warm-up of both.  Reported: the median round of each side per run, the 10th / 90th percentiles as the run-to-run spread, and how
many columns the float32 side places differently from the operator (its arithmetic is not the rule's)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from lidar_rt_amd import actor_sweep as asw, sweep


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=80_000)
    ap.add_argument("--assets", type=int, default=10)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_actor_sweep: needs a HIP device (a timing taken anywhere else says nothing)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    P, A, W = a.gaussians, a.assets, a.width
    rng = np.random.default_rng(0)
    seg = torch.tensor(np.linspace(0, P, A + 1).astype(np.int32), device=dev)
    poses, twists = [], []
    for k in range(A):
        az, r = rng.uniform(-np.pi, np.pi), rng.uniform(5.0, 60.0)
        q = rng.normal(size=4)
        poses.append(np.concatenate([[r * np.cos(az), r * np.sin(az), 0.0], q / np.linalg.norm(q), [1.0]]))
        twists.append(np.array([-3.0, 0.2, 0.0, 0.0, 0.0, 0.15]) * rng.uniform(0.3, 1.0) * rng.choice([-1.0, 1.0]))
    f32 = lambda x: torch.tensor(np.asarray(x), dtype=torch.float32, device=dev)
    xyz = f32(rng.uniform(-1.0, 1.0, (P, 3)) * [2.2, 0.9, 0.8]).requires_grad_(True)
    rot = f32(rng.normal(size=(P, 4))).requires_grad_(True)
    eta = f32(twists).requires_grad_(True)
    pz = f32(poses)
    g_xyz, g_rot = f32(rng.normal(size=(P, 3))), f32(rng.normal(size=(P, 4)))
    s2w = torch.eye(4, dtype=torch.float64, device=dev)
    xi = torch.tensor([4.0, 0.3, 0.0, 0.0, 0.01, 0.05], dtype=torch.float64, device=dev)
    tau = sweep.column_times(W).to(dev)
    ws = torch.empty(asw.work_bytes(P, A, W), dtype=torch.uint8, device=dev)

    def clear():
        xyz.grad = rot.grad = eta.grad = None

    def torch_side():
        clear()
        t = asw.actor_sweep_reference(xyz, rot, seg, pz, eta, s2w, xi, tau, W, dtype=torch.float32, with_margin=False)
        torch.autograd.backward([t.xyz_s, t.rot_s], [g_xyz, g_rot])
        return t.column

    def op_side():
        clear()
        xs, rs, info = asw.actor_sweep(xyz, rot, seg, pz, eta, s2w, xi, tau, W, workspace=ws)
        torch.autograd.backward([xs, rs], [g_xyz, g_rot])
        return info

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.reps * 1e6

    sides = (torch_side, op_side)
    for _ in range(a.warmup):
        for fn in sides:
            fn()
    t = [[] for _ in sides]
    for _ in range(a.rounds):
        for k, fn in enumerate(sides):
            t[k].append(timed(fn))
    info = op_side()
    differ = int((torch_side().to(torch.int32) != info.column).sum())
    q = lambda v, p: float(np.percentile(v, p))
    stat = lambda v: {"median": q(v, 50), "p10": q(v, 10), "p90": q(v, 90)}
    res = {"bench": "actor_sweep", "gaussians": P, "assets": A, "width": W, "rounds": a.rounds, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "unit": "microseconds per forward + backward", "torch_float32": stat(t[0]), "operator": stat(t[1]), "speedup": q(t[0], 50) / q(t[1], 50),
           "counts": dict(zip(asw.COUNT_NAMES, info.counts.tolist())), "columns_the_float32_side_places_differently": differ}
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
