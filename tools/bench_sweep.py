"""Time the sweep-ray operator against the torch expression it replaces under --refine-poses, on the GPU, and print one JSON object.

    python tools/bench_sweep.py [--height 64 --width 2048 --rounds 30 --reps 50]

Both sides rebuild the ray grid of one frame from ``sensor2world @ Exp(xi)`` and run the backward for the same upstream gradients, which is what
a training iteration does:

  torch     ``RangeFrames.range_rays(H, W, inc, s2w @ se3_exp(xi))`` and autograd's backward (what ``SensorPoses.get_range_rays`` did before
            the operator, and still does for a frame without a sweep)
  operator  ``sweep.sweep_rays(s2w @ se3_exp(xi), twist, H, W, inc)`` and its backward (two launches each way, plus the same se3_exp)

A round times ``reps`` forward + backward pairs of one side between two device synchronisations with the host clock; the sides alternate round
by round in one process, after a warm-up of both.  Reported: the median round of each side, per pair, and the 10th / 90th percentiles as the
run-to-run spread.  ``grid_only`` is the same comparison from a pose that is a leaf tensor: the grid and its backward without ``se3_exp``,
whose small launches cost both sides the same.  ``max_direction_difference``: with a zero twist the two grids are the same rays (float32 against float64 arithmetic).
"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from lidar_rt_amd import poses, scenes, sweep
from lidar_rt_amd.training import RangeFrames


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_sweep: needs a HIP device (a timing taken anywhere else says nothing)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    H, W = a.height, a.width
    inc = (math.radians(-24.9), math.radians(2.0))
    s2w = torch.as_tensor(scenes.pose_matrix((812.3, -655.1, 1.7), yaw=0.4), dtype=torch.float32, device=dev)
    g = torch.Generator().manual_seed(0)
    g_o, g_d = torch.randn((H, W, 3), generator=g).to(dev), torch.randn((H, W, 3), generator=g).to(dev)
    xi = torch.nn.Parameter(torch.tensor([0.01, -0.02, 0.005, 0.001, -0.002, 0.003], device=dev))
    twist = torch.nn.Parameter(torch.tensor([1.5, 0.1, 0.0, 0.0, 0.0, 0.02], device=dev))
    inc_d = torch.tensor(inc, dtype=torch.float32, device=dev)
    tau_d = sweep.column_times(W).to(device=dev, dtype=torch.float32)

    def torch_pair():
        xi.grad = None
        o, d = RangeFrames.range_rays(H, W, inc, s2w @ poses.se3_exp(xi), "KITTI")
        torch.autograd.backward([o, d], [g_o, g_d])

    def op_pair():
        xi.grad = None; twist.grad = None
        o, d = sweep.sweep_rays(s2w @ poses.se3_exp(xi), twist, H, W, inc_d, "KITTI", tau=tau_d)
        torch.autograd.backward([o, d], [g_o, g_d])

    # the grid alone, from a pose that is a leaf: what the operator itself replaces (se3_exp and the 4 x 4 product cost both sides the same)
    pose_leaf = (s2w @ poses.se3_exp(xi)).detach().requires_grad_(True)

    def torch_grid():
        pose_leaf.grad = None
        o, d = RangeFrames.range_rays(H, W, inc, pose_leaf, "KITTI")
        torch.autograd.backward([o, d], [g_o, g_d])

    def op_grid():
        pose_leaf.grad = None; twist.grad = None
        o, d = sweep.sweep_rays(pose_leaf, twist, H, W, inc_d, "KITTI", tau=tau_d)
        torch.autograd.backward([o, d], [g_o, g_d])

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.reps * 1e6

    for _ in range(a.warmup):
        torch_pair(); op_pair(); torch_grid(); op_grid()
    t_torch, t_op, t_torch_grid, t_op_grid = [], [], [], []
    for _ in range(a.rounds):
        t_torch.append(timed(torch_pair))
        t_op.append(timed(op_pair))
        t_torch_grid.append(timed(torch_grid))
        t_op_grid.append(timed(op_grid))
    with torch.no_grad():
        d_ref = RangeFrames.range_rays(H, W, inc, s2w, "KITTI")[1]
        d_op = sweep.sweep_rays(s2w, torch.zeros(6, device=dev), H, W, inc_d, "KITTI", tau=tau_d)[1]
    q = lambda v, p: float(np.percentile(v, p))
    res = {"bench": "sweep_rays", "height": H, "width": W, "rounds": a.rounds, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "unit": "microseconds per forward + backward",
           "torch": {"median": q(t_torch, 50), "p10": q(t_torch, 10), "p90": q(t_torch, 90)},
           "operator": {"median": q(t_op, 50), "p10": q(t_op, 10), "p90": q(t_op, 90)},
           "speedup": q(t_torch, 50) / q(t_op, 50),
           "grid_only": {"torch": {"median": q(t_torch_grid, 50), "p10": q(t_torch_grid, 10), "p90": q(t_torch_grid, 90)},
                         "operator": {"median": q(t_op_grid, 50), "p10": q(t_op_grid, 10), "p90": q(t_op_grid, 90)},
                         "speedup": q(t_torch_grid, 50) / q(t_op_grid, 50)},
           "max_direction_difference": float((d_ref - d_op).abs().max())}
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
