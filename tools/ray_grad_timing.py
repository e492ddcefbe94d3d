#!/usr/bin/env python3
"""Developer tool: the cost of ray gradients (lrt_backward_rays) on the S1M frame (1 M Gaussians, 64 x 2048 rays, deg 3).

Alternating training steps through `Tracer` with and without ray_o / ray_d requiring grad; per step the library's HIP-event timing of
the backward region (lrt_get_timing 'bwd': the bucketed replay's launches, k_bwd_prep2<1> included) and a torch-event window around
`out.backward()` (the memsets of the two ray-gradient tensors and the autograd plumbing included).  Prints one JSON line with medians.
    python tools/ray_grad_timing.py [--steps 30]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, REPO)
from lidar_rt_amd import scenes                                       # noqa: E402
from lidar_rt_amd.diff_lidar_tracer import Tracer, TracingSettings   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sc, ro_np, rd_np = scenes.s1m()
    t = {k: torch.as_tensor(v, device=dev).requires_grad_(True) for k, v in sc.items()}
    dL = torch.as_tensor(scenes.upstream_grad(*ro_np.shape[:2]), device=dev)
    e = torch.empty(0, device=dev)
    st = TracingSettings(None, None, None, None, torch.as_tensor(scenes.BG_DEFAULT, device=dev), 1.0, e, e, 3, torch.zeros(3, device=dev), False, False)
    tr = Tracer()
    tr.optix_context.enable_timing(True)
    res = {False: {"bwd_region_ms": [], "backward_call_ms": []}, True: {"bwd_region_ms": [], "backward_call_ms": []}}
    for i in range(a.warmup + 2 * a.steps):
        rays = bool(i % 2)
        ro = torch.as_tensor(ro_np, device=dev).requires_grad_(rays); rd = torch.as_tensor(rd_np, device=dev).requires_grad_(rays)
        for v in t.values():
            v.grad = None
        tr.build_from_gaussians(t["means"], t["scales"], t["rotations"], t["opacities"])
        out, _ = tr(ro, rd, None, t["means"], torch.zeros_like(t["means"]), shs=t["shs"], opacities=t["opacities"], scales=t["scales"],
                    rotations=t["rotations"], tracer_settings=st)
        torch.cuda.synchronize()
        tr.optix_context.get_timing(dev)                                 # reset the sums: only this step's backward below
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out.backward(dL); e1.record()
        torch.cuda.synchronize()
        tm = tr.optix_context.get_timing(dev)
        if i >= a.warmup:
            res[rays]["bwd_region_ms"].append(tm["bwd"][0] / max(tm["bwd"][1], 1))
            res[rays]["backward_call_ms"].append(e0.elapsed_time(e1))
    med = {("with_rays" if k else "without"): {n: float(np.median(v)) for n, v in d.items()} for k, d in res.items()}
    med["extra_ms"] = {n: med["with_rays"][n] - med["without"][n] for n in ("bwd_region_ms", "backward_call_ms")}
    med["steps"] = a.steps
    print(json.dumps(med))


if __name__ == "__main__":
    main()
