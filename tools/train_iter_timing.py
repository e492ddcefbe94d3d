#!/usr/bin/env python3
"""Developer tool: wall time of whole training iterations (lidar_rt_amd.training.training_step) at S1M scale and the
share of the library's kernels in it (torch profiler, kernel names grouped).
--fused-loss (or FUSED=1): the per-pixel losses through lidar_rt_amd.losses.range_image_loss.  --compare-loss: both settings in one process,
alternating -- ms per iteration (median of RUNS >= 5 windows of 10 iterations each) and, profiled in a pass of its own, the GPU time and the
launch count of the loss part alone (the raw image -> loss -> d_rendered, forward + backward), each as the median of RUNS passes.
--compare-chamfer: the same alternating windows for the Chamfer term, chamfer_3DDist on the masked points against the grid operator
(lidar_rt_amd.grid_chamfer), both with chamfer_points_detached=False; then the operator alone, forward and backward GPU time and launches,
on this scene's coherent frame and on independent random ranges (the degenerate search).
--compare-adam [--actors]: the same alternating windows for the optimizer step under three settings, each on a scene of its own: torch.optim.Adam
(fused=True, the default), lidar_rt_amd.optim.GaussianAdam (--fused-adam) and GaussianAdam on the rows the frame hit (--fused-adam --sparse-adam);
then, profiled in a pass of its own, the GPU kernel time and the launch count of the optimizer part alone (the steps of all assets on the
gradients of one real backward), and the measured share of touched rows.  S1M by default; --actors: the kitti360_dynamic shape (500 k background
Gaussians + 8 actors x 8 k with tracking boxes, 66 x 1030 rays), where sparse mode steps the boxed actors densely (lambda_reg != 0).
--compare-densify: the same alternating windows for the densification statistics of an iteration, the PyTorch ops against the fused operator
(--fused-densify, lidar_rt_amd.densify.densify_stats), on S1M, in iterations without a densification event (tools/bench_densify.py times the event)."""
import os, sys, time, types
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, REPO)
from lidar_rt_amd import scenes, training
from lidar_rt_amd.renderer import raytracing

dev = torch.device("cuda:0")


def compare_adam():
    import statistics
    from torch.profiler import profile, ProfilerActivity
    t = lambda a: torch.as_tensor(a, device=dev)
    runs = max(5, int(os.environ.get("RUNS", "7")))
    with_actors = "--actors" in sys.argv
    bg = torch.tensor([0.0, 0.0, 1.0], device=dev)

    def mk(s, noise, seed, box=None):
        r = np.random.default_rng(seed); op = s["opacities"]
        a = training.GaussianAsset.from_tensors(t(s["means"] + noise * r.normal(size=s["means"].shape).astype(np.float32)), t(s["shs"][:, :1]), t(s["shs"][:, 1:]),
                                                t(np.log(s["scales"])), t(s["rotations"]), t(np.log(op / (1 - op))), extent=60.0, bounding_box=box)
        a.active_sh_degree = 3
        return a
    if with_actors:
        bgs, acts, poses_of, rays_of = scenes.kitti360_dynamic()
        ro, rd = rays_of(0)
        poses = poses_of(0)
        lo, hi = t(np.array([-2.3, -1.05, -0.1], np.float32)), t(np.array([2.3, 1.05, 1.7], np.float32))     # the actors' 4.4 x 1.9 x 1.6 m box with a margin

        def assets(noise):
            out = [mk(bgs, noise, 1)]
            for k, (a, (tt, q)) in enumerate(zip(acts, poses)):
                out.append(mk(a, noise, 2 + k, types.SimpleNamespace(frame={0: (t(tt), t(q).reshape(1, 4), None, None)}, min_xyz=lo, max_xyz=hi)))
            return out
        shape = f"kitti360_dynamic: {bgs['means'].shape[0]} background Gaussians + {len(acts)} boxed actors x {acts[0]['means'].shape[0]}"
    else:
        s1, ro, rd = scenes.s1m()
        assets = lambda noise: [mk(s1, noise, 1)]
        shape = f"S1M: {s1['means'].shape[0]} Gaussians, one asset"
    base = training.default_options()
    args = types.SimpleNamespace(dynamic=with_actors, opt=base, pipe=types.SimpleNamespace())
    frames = training.RangeFrames()
    with torch.no_grad():
        pk = raytracing(0, assets(0.0), (t(ro), t(rd), t(ro[0, 0])), bg, args)
    frames.add_frame(0, t(ro), t(rd), pk["depth"].squeeze(-1).detach(), pk["intensity"].squeeze(-1).detach(), pk["raydrop"].squeeze(-1) < 0.6)
    settings = (("torch.optim.Adam(fused=True) (default)", {}), ("GaussianAdam (--fused-adam)", {"fused_adam": True}),
                ("GaussianAdam, hit rows (--fused-adam --sparse-adam)", {"fused_adam": True, "sparse_adam": True}))
    opts, scs = [], []
    for _, kw in settings:
        o = types.SimpleNamespace(**vars(base))
        for k, v in kw.items():
            setattr(o, k, v)
        sc_ = training.GaussianScene(assets(0.02)); sc_.training_setup(o)
        opts.append(o); scs.append(sc_)
    it = 0
    step = lambda k, o=None: training.training_step(scs[k], frames, 0, it, o or opts[k], bg, dynamic=with_actors)
    for k in range(3):                                            # warm every path (code objects, workspaces, allocator)
        for _ in range(3):
            it += 1; step(k)
    ms = [[], [], []]
    for _ in range(runs):                                         # alternating windows: drift of the machine hits all three alike
        for k in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(10):
                it += 1; step(k)
            torch.cuda.synchronize(); ms[k].append((time.perf_counter() - t0) / 10 * 1e3)
    # the optimizer part alone: one real backward whose optimizer step is left out (iterations = 0) leaves the gradients in place; the rows it
    # touched are those whose densification count moved.  Then the steps of all assets, profiled (profiler on: no wall time taken here)
    part, share = [], None
    for k in range(3):
        hold = types.SimpleNamespace(**vars(opts[k])); hold.iterations = 0
        before = [g.denom.clone() for g in scs[k].gaussians_assets]
        it += 1; step(k, hold)
        touched = [((g.denom - b) > 0).reshape(-1) for g, b in zip(scs[k].gaussians_assets, before)]
        if share is None:
            share = [float(x.float().mean()) for x in touched]
        us, launches = [], []
        for r in range(runs + 2):
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for g, rows in zip(scs[k].gaussians_assets, touched):
                    if getattr(opts[k], "sparse_adam", False):
                        g.optimizer.step(rows=None if (g.bounding_box is not None and opts[k].lambda_reg != 0) else rows)
                    else:
                        g.optimizer.step()
                torch.cuda.synchronize()
            if r >= 2:
                ev = [e for e in prof.key_averages() if e.device_time_total > 0]
                us.append(sum(e.device_time_total for e in ev)); launches.append(sum(e.count for e in ev))
        part.append((statistics.median(us), statistics.median(launches), min(us), max(us)))
    print(f"{shape}; {ro.shape[0]} x {ro.shape[1]} rays; {runs} alternating windows of 10 iterations; optimizer part: {runs} profiled passes")
    print(f"touched rows of the frame (accum_weights > 0): " + ", ".join(f"{'background' if i == 0 else f'actor {i}'} {100 * x:.1f} %" for i, x in enumerate(share)))
    print("| | " + " | ".join(n for n, _ in settings) + " |")
    print("|---|---:|---:|---:|")
    f = lambda v: f"{statistics.median(v):.3f} (min {min(v):.3f}, max {max(v):.3f})"
    print("| training iteration, ms wall | " + " | ".join(f(v) for v in ms) + " |")
    print("| optimizer part, GPU kernel time, us | " + " | ".join(f"{p[0]:.1f} (min {p[2]:.1f}, max {p[3]:.1f})" for p in part) + " |")
    print("| optimizer part, kernel launches | " + " | ".join(f"{p[1]:.0f}" for p in part) + " |")
    print("| optimizer part, share of the iteration's wall time (GPU time / iteration) | " + " | ".join(f"{p[0] / 10 / statistics.median(v):.1f} %" for p, v in zip(part, ms)) + " |")


def compare_densify():
    import statistics
    t = lambda a: torch.as_tensor(a, device=dev)
    runs = max(5, int(os.environ.get("RUNS", "7")))
    bg = torch.tensor([0.0, 0.0, 1.0], device=dev)
    s1, ro, rd = scenes.s1m()
    op = s1["opacities"]

    def mk(noise):
        r = np.random.default_rng(1)
        a = training.GaussianAsset.from_tensors(t(s1["means"] + noise * r.normal(size=s1["means"].shape).astype(np.float32)), t(s1["shs"][:, :1]), t(s1["shs"][:, 1:]),
                                                t(np.log(s1["scales"])), t(s1["rotations"]), t(np.log(op / (1 - op))), extent=60.0)
        a.active_sh_degree = 3
        return a
    base = training.default_options()
    base.densify_from_iter = 10 ** 9                               # statistics in every iteration, no event
    args = types.SimpleNamespace(dynamic=False, opt=base, pipe=types.SimpleNamespace())
    frames = training.RangeFrames()
    with torch.no_grad():
        pk = raytracing(0, [mk(0.0)], (t(ro), t(rd), t(ro[0, 0])), bg, args)
    frames.add_frame(0, t(ro), t(rd), pk["depth"].squeeze(-1).detach(), pk["intensity"].squeeze(-1).detach(), pk["raydrop"].squeeze(-1) < 0.6)
    settings = (("PyTorch statistics (default)", {}), ("fused statistics (--fused-densify)", {"fused_densify": True}))
    opts, scs = [], []
    for _, kw in settings:
        o = types.SimpleNamespace(**vars(base))
        for k, v in kw.items():
            setattr(o, k, v)
        sc_ = training.GaussianScene([mk(0.02)]); sc_.training_setup(o)
        opts.append(o); scs.append(sc_)
    it = 0
    for k in range(2):
        for _ in range(3):
            it += 1; training.training_step(scs[k], frames, 0, it, opts[k], bg)
    ms = [[], []]
    for _ in range(runs):
        for k in range(2):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(10):
                it += 1; training.training_step(scs[k], frames, 0, it, opts[k], bg)
            torch.cuda.synchronize(); ms[k].append((time.perf_counter() - t0) / 10 * 1e3)
    print(f"S1M: {s1['means'].shape[0]} Gaussians, one asset; {ro.shape[0]} x {ro.shape[1]} rays; {runs} alternating windows of 10 iterations, no densification event")
    print("| | " + " | ".join(n for n, _ in settings) + " |")
    print("|---|---:|---:|")
    f = lambda v: f"{statistics.median(v):.3f} (min {min(v):.3f}, max {max(v):.3f})"
    print("| training iteration, ms wall | " + " | ".join(f(v) for v in ms) + " |")


if "--compare-adam" in sys.argv:
    compare_adam()
    sys.exit(0)
if "--compare-densify" in sys.argv:
    compare_densify()
    sys.exit(0)
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
if "--compare-chamfer" in sys.argv:
    import statistics
    from torch.profiler import profile, ProfilerActivity
    from lidar_rt_amd import grid_chamfer as gcd
    from lidar_rt_amd.chamfer3D import chamfer_3DDist
    runs = max(5, int(os.environ.get("RUNS", "7")))
    it = 0
    ms = {False: [], True: []}
    for grid in (False, True):
        opt.grid_chamfer = grid
        for _ in range(3):
            it += 1; training.training_step(scene, frames, 0, it, opt, bg, chamfer_points_detached=False)
    for _ in range(runs):
        for grid in (False, True):
            opt.grid_chamfer = grid
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(10):
                it += 1; training.training_step(scene, frames, 0, it, opt, bg, chamfer_points_detached=False)
            torch.cuda.synchronize(); ms[grid].append((time.perf_counter() - t0) / 10 * 1e3)
    with torch.no_grad():
        pred = raytracing(0, scene.gaussians_assets, frames, bg, args)["depth"].squeeze(-1).detach().clone()
    o_, d_ = frames.get_range_rays(0)
    gt_d, mask = frames.get_depth(0), frames.get_mask(0)
    gen = torch.Generator(device=dev).manual_seed(3)
    clouds = {"coherent (this scene's prediction against its ground truth)": (pred, gt_d),
              "incoherent (independent random ranges, 1-80 m)": (1 + 79 * torch.rand(pred.shape, device=dev, generator=gen), 1 + 79 * torch.rand(pred.shape, device=dev, generator=gen))}

    def existing(ra, rb):
        a = frames.inverse_projection_with_range(0, ra); b = frames.inverse_projection_with_range(0, rb)
        d1, d2, _, _ = chamfer_3DDist()(a[None].contiguous(), b[None].contiguous())
        return opt.lambda_cd * (d1 + d2).mean() * 0.5

    def grid_op(ra, rb):
        return gcd.grid_chamfer(o_, d_, ra, rb, mask, weight=opt.lambda_cd)[0]

    def timed(fn):
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            out = fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.key_averages() if e.device_time_total > 0]
        return out, sum(e.device_time_total for e in ev), sum(e.count for e in ev)
    print(f"S1M, {pred.shape[0]} x {pred.shape[1]} image, {int(mask.sum())} valid pixels, {runs} alternating windows of 10 iterations, chamfer_points_detached=False")
    print("| | chamfer_3DDist on the masked points (default) | grid operator (--grid-chamfer) |")
    print("|---|---:|---:|")
    f = lambda v: f"{statistics.median(v):.3f} (min {min(v):.3f}, max {max(v):.3f})"
    print(f"| training iteration, ms wall | {f(ms[False])} | {f(ms[True])} |")
    for name, (ra, rb) in clouds.items():
        row = {}
        for grid, fn in ((False, existing), (True, grid_op)):
            fw, bw = [], []
            for k in range(runs + 2):
                x = ra.clone().requires_grad_(True)
                loss, us_f, n_f = timed(lambda: fn(x, rb))
                _, us_b, n_b = timed(lambda: loss.backward())
                if k >= 2:
                    fw.append((us_f, n_f)); bw.append((us_b, n_b))
            med = lambda v: (statistics.median(u for u, _ in v), statistics.median(n for _, n in v), min(u for u, _ in v), max(u for u, _ in v))
            row[grid] = (med(fw), med(bw))
        for i, part in enumerate(("forward", "backward")):
            c = lambda g: f"{row[g][i][0]:.1f} us (min {row[g][i][2]:.1f}, max {row[g][i][3]:.1f}), {row[g][i][1]:.0f} launches"
            print(f"| operator alone, {name}: {part} (points included) | {c(False)} | {c(True)} |")
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
