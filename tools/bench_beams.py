"""Time the beam-ray operator against the sweep-ray operator on the same inputs, on the GPU; print one JSON object and write profiles/beam_rays.md.

    python tools/bench_beams.py [--height 64 --width 2048 --rounds 30 --reps 400] [--out profiles/beam_rays.md]

Both sides make the ray grid of one frame (F = 1) from a leaf pose and a twist and run the backward for the same upstream gradients:

  sweep   ``sweep.sweep_rays(pose, twist, H, W, inc)`` and its backward to pose and twist: the parent operation, two launches each way
  beams   ``beams.beam_rays(pose, twist, H, W, inc, table)`` and its backward to pose, twist AND the (H, 2) table: two launches each way

The beam operator does strictly more work -- a third axis per column, two more numbers per row, a third sum per column, and the table's
gradient: two cross-lane sums per ray -- so what is reported is its RATIO to the sweep operator, not a gain.  ``beams_pose_only`` is the same call
with a table that needs no gradient (the row reduction is skipped): what the forward and the pose chain alone cost over the sweep rays.

A round times ``reps`` forward + backward pairs of one side between two device synchronisations with the host clock; the sides alternate round
by round in one process, after a warm-up of all.  Reported: the median round of each side, per pair, and the 10th / 90th percentiles as the
run-to-run spread.  ``--pairs N``: run N pairs of ``beams`` after one warm-up pair and nothing else (for a kernel trace that counts launches).
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

from lidar_rt_amd import beams, build, resources, scenes, sweep


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--reps", type=int, default=400, help="pairs per timed round: a round of 400 is about a tenth of a second")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=0, help="run that many forward + backward pairs of the beam operator and exit (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "beam_rays.md"), help="the document the result is also written into")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_beams: needs a HIP device (a timing taken anywhere else says nothing)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    H, W = a.height, a.width
    inc_d = torch.tensor((math.radians(-24.9), math.radians(2.0)), dtype=torch.float32, device=dev)
    tau_d = sweep.column_times(W).to(device=dev, dtype=torch.float32)
    g = torch.Generator().manual_seed(0)
    g_o, g_d = torch.randn((H, W, 3), generator=g).to(dev), torch.randn((H, W, 3), generator=g).to(dev)
    pose = torch.as_tensor(scenes.pose_matrix((812.3, -655.1, 1.7), yaw=0.4), dtype=torch.float32, device=dev).requires_grad_(True)
    twist = torch.tensor([1.5, 0.1, 0.0, 0.0, 0.0, 0.02], device=dev).requires_grad_(True)
    table = (2e-3 * torch.randn((H, 2), generator=g)).to(dev).requires_grad_(True)
    table_fixed = table.detach().clone()
    ws_s = torch.empty(sweep.work_bytes(1, H, W), dtype=torch.uint8, device=dev)
    ws_b = torch.empty(beams.work_bytes(1, H, W), dtype=torch.uint8, device=dev)

    def sweep_pair():
        pose.grad = None; twist.grad = None
        o, d = sweep.sweep_rays(pose, twist, H, W, inc_d, "KITTI", tau=tau_d, workspace=ws_s)
        torch.autograd.backward([o, d], [g_o, g_d])

    def beams_pair():
        pose.grad = None; twist.grad = None; table.grad = None
        o, d = beams.beam_rays(pose, twist, H, W, inc_d, table, "KITTI", tau=tau_d, workspace=ws_b)
        torch.autograd.backward([o, d], [g_o, g_d])

    def beams_pose_only():
        pose.grad = None; twist.grad = None
        o, d = beams.beam_rays(pose, twist, H, W, inc_d, table_fixed, "KITTI", tau=tau_d, workspace=ws_b)
        torch.autograd.backward([o, d], [g_o, g_d])

    if a.pairs > 0:
        beams_pair()
        torch.cuda.synchronize()
        for _ in range(a.pairs):
            beams_pair()
        torch.cuda.synchronize()
        print(json.dumps({"bench": "beam_rays", "pairs": a.pairs, "warmup_pairs": 1}), flush=True)
        return 0

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.reps * 1e6

    for _ in range(a.warmup):
        sweep_pair(); beams_pair(); beams_pose_only()
    t_s, t_b, t_p = [], [], []
    for _ in range(a.rounds):
        t_s.append(timed(sweep_pair))
        t_b.append(timed(beams_pair))
        t_p.append(timed(beams_pose_only))
    with torch.no_grad():                                                # what the table moves, and that a zero table moves nothing
        d_s = sweep.sweep_rays(pose, twist, H, W, inc_d, "KITTI", tau=tau_d)[1]
        d_b = beams.beam_rays(pose, twist, H, W, inc_d, table_fixed, "KITTI", tau=tau_d)[1]
        d_0 = beams.beam_rays(pose, twist, H, W, inc_d, torch.zeros_like(table_fixed), "KITTI", tau=tau_d)[1]
    q = lambda v, p: float(np.percentile(v, p))
    side = lambda v: {"median": q(v, 50), "p10": q(v, 10), "p90": q(v, 90)}
    res = {"bench": "beam_rays", "height": H, "width": W, "frames": 1, "rounds": a.rounds, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", "").split(":")[0],
           "sources": build.beams_source_hash(), "unit": "microseconds per forward + backward",
           "sweep": side(t_s), "beams": side(t_b), "beams_pose_only": side(t_p),
           "ratio_to_sweep": q(t_b, 50) / q(t_s, 50), "ratio_to_sweep_pose_only": q(t_p, 50) / q(t_s, 50),
           "zero_table_equals_sweep": bool(torch.equal(d_0, d_s)), "max_direction_change_of_the_table": float((d_b - d_s).abs().max())}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    row = lambda name, s: f"| {name} | {s['median']:.0f} ({s['p10']:.0f} .. {s['p90']:.0f}) |"
    with open(a.out, "w") as fh:
        fh.write(f"# Beam rays (`liblrt_beams.so`, `lidar_rt_amd/beams.py`): `tools/bench_beams.py` on {res['device']} ({res['arch']})\n\n"
                 f"Sources `{res['sources']}` (`build.beams_source_hash()`).  {H} x {W}, one frame.  Microseconds per forward + backward, host clock around\n"
                 f"{a.reps} pairs between two device synchronisations, {a.rounds} rounds per side alternating in one process after a warm-up of all; median\n"
                 "(10th .. 90th percentile).  The beam operator does strictly more work than the sweep operator: the ratio is a cost, not a gain.\n\n"
                 "| side | time |\n|---|---:|\n" + row("`sweep_rays`, backward to pose and twist (the parent operation)", res["sweep"]) + "\n"
                 + row("`beam_rays`, backward to pose, twist and table", res["beams"]) + "\n"
                 + row("`beam_rays`, table without a gradient (no row reduction)", res["beams_pose_only"]) + "\n\n"
                 f"Ratio of medians to `sweep_rays`: {res['ratio_to_sweep']:.3f} with the table's gradient, {res['ratio_to_sweep_pose_only']:.3f} without.\n\n"
                 "```json\n" + line + "\n```\n\n"
                 "## Resources (`resources.table_md`, hipcc `--offload-arch=" + build.ARCH + " " + " ".join(build.CODEGEN_FLAGS) + "`)\n\n"
                 + resources.table_md(resources.kernel_resources(build.BEAMS_LIB)) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
