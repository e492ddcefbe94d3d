"""Time the un-projection operator against the torch expression it replaces, on the GPU, and print one JSON object.

    python tools/bench_unproject.py [--height 64 --width 2048 --frames 16 --rounds 30 --reps 20]

Both sides turn F rendered range images, about half of whose pixels are kept, into world-frame points:

  torch     per frame ``RangeFrames.inverse_projection_with_range(f, depth, mask)`` with a boolean mask -- the indexing waits for the device to
            learn each frame's size (the host wait is part of what is replaced, and of what is timed)
  operator  ``unproject.points_from_range_images(depth, rays_o, rays_d, keep=mask)``: all frames in one call, three launches, no host wait; the
            points, their pixels, the offsets and the counts

A round times ``reps`` runs of one side between two device synchronisations with the host clock; the sides alternate round by round in one
process, after a warm-up of both.  Reported: the median round of each side, per run over all F frames, and the 10th / 90th percentiles as the
run-to-run spread.  ``transformed``: the operator's float64 path with one transform per frame and one per column (no torch counterpart is
timed: it would have to hold the rays in float64).  ``equal_bits``: the two sides' world-frame points are the same bits.
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

from lidar_rt_amd import scenes, unproject
from lidar_rt_amd.training import RangeFrames


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_unproject: needs a HIP device (a timing taken anywhere else says nothing)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    F, H, W = a.frames, a.height, a.width
    inc = (math.radians(-24.9), math.radians(2.0))
    g = torch.Generator().manual_seed(0)
    rf = RangeFrames()
    poses = []
    for f in range(F):
        s2w = torch.as_tensor(scenes.pose_matrix((812.3 + 0.5 * f, -655.1, 1.7), yaw=0.4 + 0.01 * f), dtype=torch.float32, device=dev)
        poses.append(s2w.double().cpu().numpy())
        o, d = RangeFrames.range_rays(H, W, inc, s2w, "KITTI")
        depth = (1.0 + 79.0 * torch.rand((H, W), generator=g)).to(dev)
        rf.add_frame(f, o, d, depth, torch.rand((H, W), generator=g).to(dev), (torch.rand((H, W), generator=g) < 0.5).to(dev))
    depth = torch.stack([rf.depth[f] for f in range(F)]).contiguous()
    inten = torch.stack([rf.intensity[f] for f in range(F)]).contiguous()
    keep = torch.stack([rf.mask[f] for f in range(F)]).contiguous()
    o = torch.stack([rf.rays[f][0] for f in range(F)]).contiguous()
    d = torch.stack([rf.rays[f][1] for f in range(F)]).contiguous()
    ws = torch.empty(unproject.work_bytes(F, H, W), dtype=torch.uint8, device=dev)
    T_frame = np.stack([np.linalg.inv(p)[:3] for p in poses])
    T_col = np.ascontiguousarray(np.broadcast_to(T_frame[:, None], (F, W, 3, 4)))

    def torch_side():
        return [rf.inverse_projection_with_range(f, rf.depth[f], rf.mask[f]) for f in range(F)]

    def op_side():
        return unproject.points_from_range_images(depth, o, d, intensity=inten, keep=keep, workspace=ws)

    def op_frame():
        return unproject.points_from_range_images(depth, o, d, intensity=inten, keep=keep, world2out=T_frame, workspace=ws)

    def op_column():
        return unproject.points_from_range_images(depth, o, d, intensity=inten, keep=keep, world2out=T_col, workspace=ws)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.reps * 1e6

    sides = (torch_side, op_side, op_frame, op_column)
    for _ in range(a.warmup):
        for fn in sides:
            fn()
    t = [[] for _ in sides]
    for _ in range(a.rounds):
        for k, fn in enumerate(sides):
            t[k].append(timed(fn))
    pc = op_side()
    n = int(pc.offsets[-1])
    equal = bool(torch.equal(pc.points[:n, :3].contiguous().view(torch.int32), torch.cat(torch_side()).contiguous().view(torch.int32)))
    q = lambda v, p: float(np.percentile(v, p))
    stat = lambda v: {"median": q(v, 50), "p10": q(v, 10), "p90": q(v, 90)}
    res = {"bench": "unproject", "frames": F, "height": H, "width": W, "kept_fraction": n / float(F * H * W), "rounds": a.rounds, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "unit": f"microseconds per {F} frames",
           "torch": stat(t[0]), "operator": stat(t[1]), "speedup": q(t[0], 50) / q(t[1], 50),
           "transformed": {"per_frame": stat(t[2]), "per_column": stat(t[3])}, "equal_bits": equal}
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
