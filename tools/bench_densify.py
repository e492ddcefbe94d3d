#!/usr/bin/env python3
"""Developer tool: one densify-and-prune event of a large asset, the PyTorch bookkeeping (GaussianAsset.densify_and_prune, the default) against
the fused operator (opt.fused_densify), and the statistics step of an iteration.  profiles/fused_densify.md holds its output.

    python tools/bench_densify.py [--rows 1000000] [--sh 3] [--runs 5]

The asset is tests/densify_cases.py's seeded "mixed" one (about 10 % clone, 5 % split, 5 % pruned), with Adam moments, under torch.optim.Adam.
Both paths run on fresh copies of it in ALTERNATING events; per event: GPU time between two device events, wall time between two device
synchronisations, and torch.cuda.max_memory_allocated over the event minus what was allocated before it.  Then, in a pass of its own under the
torch profiler: kernel launches (memsets and copies included) and summed kernel time; and under set_sync_debug_mode("warn"): the host waits.
The apply kernel's share of the HBM peak is by the byte model (rows read + rows written) x row bytes x 3 (parameter and two moments)."""
import argparse
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, REPO)
from lidar_rt_amd import build as lrt_build, densify as dn, training   # noqa: E402
from tests import densify_cases as dc                                  # noqa: E402

HBM_PEAK = 8.0e12                                                      # bytes / s, the MI355X's specified peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--sh", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_densify: needs a GPU; nothing is measured without one")
    dev = torch.device("cuda:0")
    from torch.profiler import profile, ProfilerActivity
    c = dc.build(args.rows, 41, "mixed", sh_degree=args.sh)
    master = dc.tensors(c, dev)
    P = args.rows

    def options(fused):
        opt = training.default_options()
        opt.densify_grad_threshold, opt.densify_scale_threshold, opt.prune_size_threshold, opt.thresh_opa_prune = dc.GRAD_THR, dc.BIG_THR, dc.HUGE_THR / 0.1, dc.OPA_THR
        opt.fused_densify = fused
        return opt

    def fresh(opt):
        g, m, acc, den, _, _ = master
        a = training.GaussianAsset.from_tensors(g["xyz"], g["f_dc"], g["f_rest"], g["scaling"], g["rotation"], g["opacity"], extent=1.0, dimension=c.S)
        a.training_setup(opt)
        for p in a._params().values():
            p.grad = torch.zeros_like(p)
        a.optimizer.step(); a.optimizer.zero_grad(set_to_none=True)
        for n, p in a._params().items():
            st = a.optimizer.state[p]
            st["exp_avg"].copy_(m[n][0]); st["exp_avg_sq"].copy_(m[n][1])
        a.xyz_gradient_accum, a.denom = acc.clone(), den.clone()
        return a

    opts = {False: options(False), True: options(True)}
    res = {False: dict(gpu=[], wall=[], peak=[]), True: dict(gpu=[], wall=[], peak=[])}
    info = {}
    for r in range(args.runs + 1):                                     # the first round warms both paths (code objects, allocator)
        for fused in (False, True):
            a = fresh(opts[fused])
            torch.manual_seed(1000 + r)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter(); e0.record()
            out = a.densify_and_prune(opts[fused], 20)
            e1.record(); torch.cuda.synchronize(); t1 = time.perf_counter()
            if r:
                res[fused]["gpu"].append(e0.elapsed_time(e1)); res[fused]["wall"].append((t1 - t0) * 1e3)
                res[fused]["peak"].append((torch.cuda.max_memory_allocated() - base) / 2 ** 20)
            info[fused] = (out, a._xyz.shape[0])
            del a
    assert info[False] == info[True], info                             # the same rule: the same counts and the same length
    # launches and kernel time, profiled; host waits, counted
    prof_res, waits, apply_us = {}, {}, []
    for fused in (False, True):
        ks, ls = [], []
        for r in range(3):
            a = fresh(opts[fused])
            torch.manual_seed(2000 + r)
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                a.densify_and_prune(opts[fused], 20)
                torch.cuda.synchronize()
            ev = [e for e in prof.key_averages() if e.device_time_total > 0]
            ks.append(sum(e.device_time_total for e in ev)); ls.append(sum(e.count for e in ev))
            if fused:
                apply_us += [e.device_time_total / e.count for e in ev if "k_densify_apply" in e.key]
            del a
        prof_res[fused] = (statistics.median(ks), statistics.median(ls))
        a = fresh(opts[fused])
        torch.manual_seed(3000)
        torch.cuda.synchronize()
        before = torch.cuda.get_sync_debug_mode()
        with warnings.catch_warnings(record=True) as wlist:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                a.densify_and_prune(opts[fused], 20)
            finally:
                torch.cuda.set_sync_debug_mode(before)
        waits[fused] = sum("synchroniz" in str(w.message).lower() for w in wlist)
        del a
    (n_clone, n_split, n_scale, n_opa), P_new = info[True]
    row_bytes = 4 * sum(int(np.prod(t.shape[1:])) for t in c.groups.values())
    model = (P + P_new) * row_bytes * 3
    med = lambda v: f"{statistics.median(v):.3f} (min {min(v):.3f}, max {max(v):.3f})"
    print(f"densify-and-prune event: {P} rows, SH degree {args.sh} ({row_bytes} bytes per row and tensor), torch.optim.Adam moments; {n_clone} clones, {n_split} splits, "
          f"{n_opa} low-opacity and {n_scale} oversized outputs; {P} -> {P_new} rows; {args.runs} alternating events; sources {lrt_build.densify_source_hash()}")
    print("| | PyTorch bookkeeping (default) | fused operator (--fused-densify) |")
    print("|---|---:|---:|")
    print(f"| event, GPU time between device events, ms | {med(res[False]['gpu'])} | {med(res[True]['gpu'])} |")
    print(f"| event, wall time, ms | {med(res[False]['wall'])} | {med(res[True]['wall'])} |")
    print(f"| summed kernel time (profiled pass), ms | {prof_res[False][0] / 1e3:.3f} | {prof_res[True][0] / 1e3:.3f} |")
    print(f"| launches (kernels, fills, copies; profiled pass) | {prof_res[False][1]:.0f} | {prof_res[True][1]:.0f} |")
    print(f"| host waits (synchronising calls, counted) | {waits[False]} | {waits[True]} |")
    print(f"| max_memory_allocated over the event, MiB above the asset | {med(res[False]['peak'])} | {med(res[True]['peak'])} |")
    if apply_us:
        us = statistics.median(apply_us)
        print(f"k_densify_apply: {us:.1f} us (median of {len(apply_us)}); byte model ({P} + {P_new}) rows x {row_bytes} B x 3 = {model / 1e9:.3f} GB -> "
              f"{model / us / 1e6:.2f} TB/s, {100 * model / (us * 1e-6) / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak")
    # the statistics step of an iteration
    g, m, acc, den, _, _ = master
    mg, w = torch.randn((P, 3), device=dev) * 1e-4, torch.rand((P, 1), device=dev) * (torch.rand((P, 1), device=dev) < 0.15)
    paths = {False: lambda a_, d_: (a_.__iadd__(torch.norm(mg, dim=-1, keepdim=True)), d_.__iadd__((w > 0).reshape(-1).reshape(-1, 1).to(d_.dtype))),
             True: lambda a_, d_: dn.densify_stats(a_, d_, mg, w)}
    st = {}
    for fused in (False, True):
        a_, d_ = acc.clone(), den.clone()
        for _ in range(3):
            paths[fused](a_, d_)
        us, ls = [], []
        for r in range(args.runs):
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                paths[fused](a_, d_)
                torch.cuda.synchronize()
            ev = [e for e in prof.key_averages() if e.device_time_total > 0]
            us.append(sum(e.device_time_total for e in ev)); ls.append(sum(e.count for e in ev))
        st[fused] = (statistics.median(us), statistics.median(ls), min(us), max(us))
    print("| statistics of one iteration | PyTorch ops (default) | fused operator |")
    print("|---|---:|---:|")
    print(f"| GPU kernel time, us | {st[False][0]:.1f} (min {st[False][2]:.1f}, max {st[False][3]:.1f}) | {st[True][0]:.1f} (min {st[True][2]:.1f}, max {st[True][3]:.1f}) |")
    print(f"| kernel launches | {st[False][1]:.0f} | {st[True][1]:.0f} |")


if __name__ == "__main__":
    main()
