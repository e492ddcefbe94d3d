"""Time the ray-drop refinement operator against the same network through torch on the same GPU, and print one JSON object.

    python tools/bench_refine.py [--height 64 --width 2048 --channels 32 --rounds 10 --reps 100 --per-kernel DIR]

One frame, 9 inputs, randomised weights and batch-norm statistics:

  operator  ``refine_raydrop(render, rays, packed, backend="hip")`` with a workspace and an output that are reused: the launches only
  torch     the module in ``eval()`` under ``no_grad`` on ``refine_inputs(render, rays)`` -- the input assembled per frame as the reference's
            eval.py does (reshape, cat, permute) -- and the reshape of the result

A round times ``reps`` calls of one side between two device synchronisations with the host clock; the sides alternate round by round in one
process after a warm-up of both.  Reported: the median round of each side per call, the 10th / 90th percentiles, the FLOP count derived from
the layer shapes, the operator's share of the float32 peak (157.3 TFLOP/s: 256 CUs x 4 SIMDs x 64 FLOP per clock x 2.4 GHz; a whole-call
figure, launch gaps included), the launches and the bytes of intermediates each path writes (the operator's: its workspace; torch's: every
tensor an ATen operation of the forward allocates), and the largest difference of the two logit images.

``--per-kernel DIR``: two more runs of this file under ``rocprofv3 --kernel-trace --stats`` (a child process each, ``--only operator`` /
``--only torch``), their kernel tables summed per kernel name into the object; the raw tables stay under DIR.  Those sums are over the child's warm-up
calls too (first launches, the framework's algorithm search), divided by all its calls: they can exceed the timed call.  A child that fails
ends the collection; the other side is not started.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np
import torch

from lidar_rt_amd import raydrop_refine as rr

PEAK_F32 = 157.3e12


def flops(H, W, Cin, c):
    """(total FLOP, {layer: FLOP}): 2 x pixels x K x C_out of every convolution, the attention's two products; the element-wise work is left out."""
    n = [(H >> l) * (W >> l) for l in range(5)]
    out = {"in": 2 * n[0] * Cin * c}
    pairs = (("down1", 1, c, 2 * c, 2 * c), ("down2", 2, 2 * c, 4 * c, 4 * c), ("down3", 3, 4 * c, 8 * c, 8 * c), ("down4", 4, 8 * c, 8 * c, 8 * c),
             ("up1", 3, 16 * c, 16 * c, 4 * c), ("up2", 2, 8 * c, 8 * c, 2 * c), ("up3", 1, 4 * c, 4 * c, c), ("up4", 0, 2 * c, 2 * c, c))
    for name, l, ci, cm, co in pairs:
        out[name + ".1"] = 2 * n[l] * 9 * ci * cm
        out[name + ".2"] = 2 * n[l] * 9 * cm * co
    T, C8 = n[4], 8 * c
    out["attn.qkv"] = 2 * T * C8 * 3 * C8
    out["attn.scores+values"] = 2 * 2 * T * T * C8
    out["attn.proj"] = 2 * T * C8 * C8
    out["out"] = 2 * n[0] * c
    return sum(out.values()), out


def network(Cin, c, dev):
    torch.manual_seed(0)
    net = rr.RaydropUNet(Cin, c)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.5)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) * 1.5 + 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.3)
    return net.to(dev).eval()


def frame(H, W, dev):
    g = torch.Generator().manual_seed(2)
    render = {"raydrop": torch.rand((H, W, 1), generator=g).to(dev), "intensity": torch.rand((H, W, 1), generator=g).to(dev),
              "depth": (torch.rand((H, W, 1), generator=g) * 80.0).to(dev)}
    d = torch.randn((H, W, 3), generator=g)
    return render, ((torch.randn(3, generator=g) * 10.0).expand(H, W, 3).contiguous().to(dev), (d / d.norm(dim=-1, keepdim=True)).to(dev))


def torch_traffic(fn):
    """(ATen operations that allocate, bytes they allocate) of one call of fn."""
    from torch.utils._python_dispatch import TorchDispatchMode
    from torch.utils._pytree import tree_flatten
    count = {"ops": 0, "bytes": 0}

    class Mode(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            seen = {t.untyped_storage().data_ptr() for t in tree_flatten((args, kwargs))[0] if torch.is_tensor(t)}
            fresh = [t for t in tree_flatten(out)[0] if torch.is_tensor(t) and t.untyped_storage().data_ptr() not in seen]
            if fresh:
                count["ops"] += 1
                count["bytes"] += sum(t.numel() * t.element_size() for t in fresh)
            return out
    with Mode():
        fn()
    return count["ops"], count["bytes"]


def kernel_table(directory):
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r.get("Name") or r.get("KernelName") or ""
                e = rows.setdefault(name, {"calls": 0, "total_us": 0.0})
                e["calls"] += int(float(r.get("Calls", 0)))
                e["total_us"] += float(r.get("TotalDurationNs", 0.0)) / 1e3
    return rows


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", choices=("operator", "torch"), default=None, help="run that side alone, warm-up and reps calls (for a profiler); no JSON")
    ap.add_argument("--per-kernel", default=None, metavar="DIR", help="also collect kernel tables under DIR with rocprofv3 (child processes)")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_refine: needs a HIP device (a timing taken anywhere else says nothing)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    H, W, c, Cin = a.height, a.width, a.channels, 9
    net = network(Cin, c, dev)
    pk = rr.pack(net)
    render, rays = frame(H, W, dev)
    ws = torch.empty(rr.work_bytes(H, W, Cin, c), dtype=torch.uint8, device=dev)
    out = torch.empty((H, W, 1), device=dev)

    def op_call():
        return rr.refine_raydrop(render, rays, pk, out=out, workspace=ws, backend="hip")

    def torch_call():
        with torch.no_grad():
            return net(rr.refine_inputs(render, rays)).reshape(H, W, 1)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.reps * 1e6

    if a.only:
        fn = op_call if a.only == "operator" else torch_call
        for _ in range(a.warmup + a.reps):
            fn()
        torch.cuda.synchronize()
        return 0
    for _ in range(a.warmup):
        op_call(); torch_call()
    t_op, t_torch = [], []
    for _ in range(a.rounds):
        t_op.append(timed(op_call))
        t_torch.append(timed(torch_call))
    with torch.no_grad():
        z_op = rr.refine_raydrop(render, rays, pk, return_logits=True, backend="hip")[1].reshape(H, W)
        z_t = net.logits(rr.refine_inputs(render, rays)).reshape(H, W)
    total, per_layer = flops(H, W, Cin, c)
    ops, nbytes = torch_traffic(torch_call)
    q = lambda v, p: float(np.percentile(v, p))
    res = {"bench": "raydrop_refine", "height": H, "width": W, "in_channels": Cin, "channels": c, "rounds": a.rounds, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "unit": "microseconds per frame",
           "operator": {"median": q(t_op, 50), "p10": q(t_op, 10), "p90": q(t_op, 90), "launches": len(per_layer), "intermediate_bytes": int(ws.numel())},
           "torch": {"median": q(t_torch, 50), "p10": q(t_torch, 10), "p90": q(t_torch, 90), "allocating_aten_ops": ops, "intermediate_bytes": int(nbytes)},
           "operator_over_torch": q(t_op, 50) / q(t_torch, 50),
           "flop": int(total), "flop_per_layer": {k: int(v) for k, v in per_layer.items()},
           "operator_share_of_f32_peak": total / (q(t_op, 50) * 1e-6) / PEAK_F32, "torch_share_of_f32_peak": total / (q(t_torch, 50) * 1e-6) / PEAK_F32,
           "max_logit_difference": float((z_op - z_t).abs().max())}
    if a.per_kernel:
        n_calls = a.warmup + a.reps
        for side in ("operator", "torch"):
            d = os.path.join(a.per_kernel, side)
            os.makedirs(d, exist_ok=True)
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "k", "--", sys.executable, os.path.abspath(__file__),
                   "--only", side, "--height", str(H), "--width", str(W), "--channels", str(c), "--reps", str(a.reps), "--warmup", str(a.warmup)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
                rows = kernel_table(d)
                if p.returncode != 0 or not rows:                   # a child that failed on the device: nothing more is started on it
                    res[side]["kernels"] = {"error": f"rocprofv3 child ended with {p.returncode}: " + (p.stderr or p.stdout)[-400:]}
                    break
                # pack / upload / input construction run once per process; the rest runs n_calls times
                res[side]["kernels"] = {k: {"calls_per_frame": v["calls"] / n_calls, "us_per_frame": v["total_us"] / n_calls}
                                        for k, v in sorted(rows.items(), key=lambda kv: -kv[1]["total_us"])[:24]}
                res[side]["kernel_launches_per_frame"] = sum(v["calls"] for v in rows.values()) / n_calls
                res[side]["kernel_us_per_frame"] = sum(v["total_us"] for v in rows.values()) / n_calls
            except (OSError, subprocess.TimeoutExpired) as e:
                res[side]["kernels"] = {"error": str(e)[-400:]}
                break
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
