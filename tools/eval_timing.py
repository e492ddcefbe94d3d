"""What a frame's evaluation costs after its render, with `evaluation.evaluate(..., fused=...)` off and on.

    python tools/eval_timing.py [--gaussians 1000000] [--frames 8] [--height 64] [--width 2048] [--repeats 7] [--parent FILE] [--out FILE.json]

Eight frames of a seeded S1M-scale scene on a 64 x 2048 KITTI-style grid, the ground truth rendered from the scene itself plus noise and a mask
of its own (the way tools/make_sequence.py renders its ground truth; its dataset shapes have no 64 x 2048 grid, so the frames are built in
memory).  The frames are rendered ONCE and `evaluation.render_frames` is replaced by that cached rendering, so that only what follows the render
is measured.  Per configuration, in alternating windows, medians of `--repeats`:

  host_ms_per_frame     wall time of evaluate() (it ends in its one device->host transfer) / frames
  gpu_ms_per_frame      summed kernel time of the profiler's device events / frames          (null if the profiler is not usable)
  launches_per_frame    the number of those events / frames

`--parent FILE`: a copy of the PARENT commit's lidar_rt_amd/evaluation.py; its evaluate() is measured in the same windows against today's
`fused=False`: the two run the same code, so their spread is the noise floor of the comparison.  Prints one JSON object."""
import argparse
import importlib.util
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from lidar_rt_amd import evaluation, renderer, scenes, training


def build(n_gauss, n_frames, H, W, dev):
    sc = scenes.make_scene(n_gauss, seed=scenes.SEED, radius_scale=1.0)
    t = lambda a: torch.as_tensor(a, device=dev)
    asset = training.GaussianAsset.from_tensors(t(sc["means"]), t(sc["shs"][:, :1]).contiguous(), t(sc["shs"][:, 1:]).contiguous(), torch.log(t(sc["scales"])),
                                                t(sc["rotations"]), training.inverse_sigmoid(t(sc["opacities"])), max_sh_degree=3, extent=30.0)
    asset.active_sh_degree = 3
    bg = torch.tensor([0.0, 0.0, 1.0], device=dev)
    blank, rays = training.RangeFrames(), {}
    for f in range(n_frames):
        pose = torch.as_tensor(scenes.pose_matrix((0.5 * f, 0.0, 0.0), yaw=0.01 * f), dtype=torch.float32, device=dev)
        rays[f] = training.RangeFrames.range_rays(H, W, (math.radians(-24.9), math.radians(2.0)), pose, "KITTI")
        z = torch.zeros(H, W, device=dev)
        blank.add_frame(f, rays[f][0], rays[f][1], z, z, torch.ones(H, W, device=dev))
    renderer.tracer_2dgs = None
    torch.cuda.synchronize(); t0 = time.perf_counter()
    renders = evaluation.render_frames([asset], blank, range(n_frames), bg)
    torch.cuda.synchronize(); render_ms = (time.perf_counter() - t0) * 1e3 / n_frames
    thr = float(torch.cat([renders[f]["raydrop"].flatten() for f in range(n_frames)]).median())
    rng = np.random.default_rng(1)
    frames = training.RangeFrames()
    for f in range(n_frames):
        hit = t(rng.uniform(size=(H, W)) < 0.9) & (renders[f]["raydrop"].squeeze(-1) < thr)
        noise = t(rng.normal(0, 0.03, (H, W)).astype(np.float32))
        frames.add_frame(f, rays[f][0], rays[f][1], (renders[f]["depth"].squeeze(-1) + noise).clamp_min(0) * hit,
                         (renders[f]["intensity"].squeeze(-1) + noise).clamp(0, 1) * hit, hit)
    return asset, bg, frames, renders, thr, render_ms


def profiled(fn):
    """(summed device time in ms, number of device events) of one call, or (None, None)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn(); torch.cuda.synchronize()
        ev = [e for e in prof.events() if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower()]
        if not ev:
            return None, None
        dur = lambda e: getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0) or (e.time_range.end - e.time_range.start)
        return sum(dur(e) for e in ev) / 1e3, len(ev)
    except Exception as exc:                                            # the measurement is optional, the reason is reported
        print(f"eval_timing: profiler not usable: {exc!r}", file=sys.stderr)
        return None, None


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--parent", default=None, help="a copy of the parent commit's lidar_rt_amd/evaluation.py")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    asset, bg, frames, renders, thr, render_ms = build(a.gaussians, a.frames, a.height, a.width, dev)
    ids = list(range(a.frames))
    cached = lambda *x, **k: renders
    runs = {"fused_off": lambda: evaluation.evaluate([asset], frames, ids, bg, raydrop_ratio=thr),
            "fused_on": lambda: evaluation.evaluate([asset], frames, ids, bg, raydrop_ratio=thr, fused=True)}
    evaluation.render_frames = cached
    if a.parent:
        spec = importlib.util.spec_from_file_location("lidar_rt_amd._parent_evaluation", a.parent)
        parent = importlib.util.module_from_spec(spec); spec.loader.exec_module(parent)
        parent.render_frames = cached
        runs["parent_commit"] = lambda: parent.evaluate([asset], frames, ids, bg, raydrop_ratio=thr)
    results = {k: fn() for k, fn in runs.items()}                     # warm-up: workspaces, caches, the libraries
    torch.cuda.synchronize()
    host = {k: [] for k in runs}
    for _ in range(a.repeats):                                          # alternating windows
        for k, fn in runs.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); host[k].append((time.perf_counter() - t0) * 1e3 / a.frames)
    out = {"gaussians": a.gaussians, "frames": a.frames, "H": a.height, "W": a.width, "repeats": a.repeats, "render_ms_per_frame": render_ms, "configs": {}}
    for k, fn in runs.items():
        gpu_ms, n_ev = profiled(fn)
        out["configs"][k] = {"host_ms_per_frame": statistics.median(host[k]), "host_ms_min": min(host[k]), "host_ms_max": max(host[k]),
                             "gpu_ms_per_frame": None if gpu_ms is None else gpu_ms / a.frames, "launches_per_frame": None if n_ev is None else n_ev / a.frames}
    out["mean_fused_off"] = results["fused_off"]["mean"]; out["mean_fused_on"] = results["fused_on"]["mean"]
    if a.parent:
        out["parent_equals_fused_off"] = json.dumps(results["parent_commit"], sort_keys=True) == json.dumps(results["fused_off"], sort_keys=True)
    txt = json.dumps(out)
    print(txt, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
