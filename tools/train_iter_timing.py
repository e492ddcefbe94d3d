#!/usr/bin/env python3
"""Developer tool: wall time of whole training iterations (lidar_rt_amd.training.training_step) at S1M scale and the
share of the library's kernels in it (torch profiler, kernel names grouped).
--fused-loss (or FUSED=1): the per-pixel losses through lidar_rt_amd.losses.range_image_loss.  --compare-loss: both settings in one process,
alternating -- ms per iteration (median of RUNS >= 5 windows of 10 iterations each) and, profiled in a pass of its own, the GPU time and the
launch count of the loss part alone (the raw image -> loss -> d_rendered, forward + backward), each as the median of RUNS passes."""
import os, sys, time, types
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, REPO)
from lidar_rt_amd import scenes, training
from lidar_rt_amd.renderer import raytracing

dev = torch.device("cuda:0")
sc, ro, rd = scenes.s1m()
t = lambda a: torch.as_tensor(a, device=dev)
op = sc["opacities"]
def asset(noise):
    r = np.random.default_rng(1)
    a = training.GaussianAsset.from_tensors(t(sc["means"] + noise * r.normal(size=sc["means"].shape).astype(np.float32)),
                                            t(sc["shs"][:, :1]), t(sc["shs"][:, 1:]), t(np.log(sc["scales"])), t(sc["rotations"]),
                                            t(np.log(op / (1 - op))), extent=60.0)
    a.active_sh_degree = 3
    return a
opt = training.default_options()
opt.bvh_refit_interval = int(os.environ.get("REFIT", "0"))
opt.fused_loss = "--fused-loss" in sys.argv or os.environ.get("FUSED", "0") == "1"
bg = torch.tensor([0.0, 0.0, 1.0], device=dev)
frames = training.RangeFrames()
args = types.SimpleNamespace(dynamic=False, opt=opt, pipe=types.SimpleNamespace())
with torch.no_grad():
    pk = raytracing(0, [asset(0.0)], (t(ro), t(rd), torch.zeros(3, device=dev)), bg, args)
frames.add_frame(0, t(ro), t(rd), pk["depth"].squeeze(-1).detach(), pk["intensity"].squeeze(-1).detach(), pk["raydrop"].squeeze(-1) < 0.6)
scene = training.GaussianScene([asset(0.02)])
scene.training_setup(opt)
if "--compare-loss" in sys.argv:
    import statistics
    from torch.profiler import profile, ProfilerActivity
    from lidar_rt_amd import losses
    runs = max(5, int(os.environ.get("RUNS", "7")))
    it = 0
    ms = {False: [], True: []}
    for fused in (False, True):                                   # warm both paths (code objects, workspaces, allocator)
        opt.fused_loss = fused
        for _ in range(3):
            it += 1; training.training_step(scene, frames, 0, it, opt, bg)
    for _ in range(runs):                                         # alternating windows: drift of the machine hits both alike
        for fused in (False, True):
            opt.fused_loss = fused
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(10):
                it += 1; training.training_step(scene, frames, 0, it, opt, bg)
            torch.cuda.synchronize(); ms[fused].append((time.perf_counter() - t0) / 10 * 1e3)
    # the loss part alone on this scene's image: GPU kernel time and launches of forward + backward (profiler on: no wall time taken here)
    with torch.no_grad():
        img = raytracing(0, scene.gaussians_assets, frames, bg, args, return_rendered=True)["rendered"].detach().clone()
    gt = (frames.get_depth(0), frames.get_intensity(0), frames.get_mask(0))
    part = {}
    for fused, fn in ((False, losses.range_image_loss_torch), (True, losses.range_image_loss)):
        us, launches = [], []
        for k in range(runs + 2):
            x = img.clone().requires_grad_(True)
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn(x, *gt, opt)[0].backward()
                torch.cuda.synchronize()
            if k >= 2:
                ev = [e for e in prof.key_averages() if e.device_time_total > 0]
                us.append(sum(e.device_time_total for e in ev)); launches.append(sum(e.count for e in ev))
        part[fused] = (statistics.median(us), statistics.median(launches), min(us), max(us))
    print(f"S1M, {img.shape[0]} x {img.shape[1]} image, {runs} alternating windows of 10 iterations; loss part: {runs} profiled passes")
    print("| | torch expression (default) | fused operator (--fused-loss) |")
    print("|---|---:|---:|")
    f = lambda v: f"{statistics.median(v):.3f} (min {min(v):.3f}, max {max(v):.3f})"
    print(f"| training iteration, ms wall | {f(ms[False])} | {f(ms[True])} |")
    print(f"| loss part, GPU kernel time, us | {part[False][0]:.1f} (min {part[False][2]:.1f}, max {part[False][3]:.1f}) | {part[True][0]:.1f} (min {part[True][2]:.1f}, max {part[True][3]:.1f}) |")
    print(f"| loss part, kernel launches | {part[False][1]:.0f} | {part[True][1]:.0f} |")
    print(f"| loss part, share of the iteration's wall time (GPU time / iteration) | {part[False][0] / 10 / statistics.median(ms[False]):.1f} % | {part[True][0] / 10 / statistics.median(ms[True]):.1f} % |")
    sys.exit(0)
for it in range(1, 4):
    training.training_step(scene, frames, 0, it, opt, bg)
torch.cuda.synchronize()
t0 = time.perf_counter()
n = 10
for it in range(4, 4 + n):
    training.training_step(scene, frames, 0, it, opt, bg)
torch.cuda.synchronize()
print(f"training iteration: {(time.perf_counter() - t0) / n * 1e3:.2f} ms wall (S1M, 1 asset, all losses, Adam step, fused_loss={opt.fused_loss})")
from torch.profiler import profile, ProfilerActivity
with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
    for it in range(20, 23):
        training.training_step(scene, frames, 0, it, opt, bg)
    torch.cuda.synchronize()
rows = [(e.key, e.device_time_total / 3.0, e.count / 3) for e in prof.key_averages() if e.device_time_total > 0]
rows.sort(key=lambda r: -r[1])
tot = sum(r[1] for r in rows)
print(f"GPU kernel time per iteration: {tot / 1e3:.2f} ms")
for k, us, c in rows[:int(os.environ.get('ROWS', '22'))]:
    print(f"  {us:8.1f} us  x{c:4.1f}  {k[:90]}")
