#!/usr/bin/env python3
"""Time the scan registration (`lidar_rt_amd/registration.py`, `liblrt_reg.so`) against the same arithmetic written as float32 torch expressions.

  operator   ``registration.align(src, tgt, None, DEFAULT_SCHEDULE)``: 2 K launches for all F pairs
  torch      the rule as torch expressions on the same device, float32 (the solve in float64): the pixel of X p, one gather per window offset,
             the point-to-plane residual, the Huber weight, the 27 sums by matrix products, ``torch.linalg.cholesky``.  No status: it takes all K
             steps, as the operator's launches do.

64 x 2048, F = 1 and F = 16 pairs of the analytic room of tests/registration_cases.py (the ranges from the planes on the host, points and normals
by ``registration.frame_geometry`` on the device).  A round times ``reps`` calls of one side between two device synchronisations with the host
clock; the sides alternate round by round in one process after a warm-up of both; the median and the 10th / 90th percentile of the rounds are
reported.  A separate, untimed pass under the torch profiler counts the launches of one call of each side.  One JSON object on stdout, the same
and the resource table into ``--out`` (profiles/registration.md).
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

from lidar_rt_amd import build, registration as rg, resources
from tests import registration_cases as rc


def torch_align(sp, sm, tp, tn, tm, schedule, H, W, inc, huber=0.1, lam=1e-6):
    """The rule in float32 torch on (F, H W, .) tensors; X (F, 3, 4) float64."""
    F = sp.shape[0]
    dev = sp.device
    X = torch.eye(4, dtype=torch.float64, device=dev)[:3].expand(F, 3, 4).contiguous()
    fidx = torch.arange(F, device=dev)[:, None]
    for rh, rw, md in schedule:
        X32 = X.to(torch.float32)
        q = sp @ X32[:, :, :3].transpose(1, 2) + X32[:, None, :, 3]
        r = q.norm(dim=-1)
        az = torch.atan2(q[..., 1], q[..., 0])
        el = torch.asin((q[..., 2] / r).clamp(-1.0, 1.0))
        w0 = torch.remainder(torch.round((math.pi - az) * (W / (2.0 * math.pi))), W).long()
        h0 = torch.round(H - (el - inc[0]) / (inc[1] - inc[0]) * H).long()
        keep = sm & (h0 >= 0) & (h0 < H) & (r > 0)
        best = torch.full_like(r, float("inf"))
        arg = torch.zeros_like(w0)
        for dh in range(-int(rh), int(rh) + 1):
            h = h0 + dh
            ok = keep & (h >= 0) & (h < H)
            hc = h.clamp(0, H - 1)
            for dw in range(-int(rw), int(rw) + 1):
                j = hc * W + torch.remainder(w0 + dw, W)
                d2 = ((tp[fidx, j] - q) ** 2).sum(-1)
                d2 = torch.where(ok & tm[fidx, j], d2, torch.full_like(d2, float("inf")))
                better = d2 < best
                best = torch.where(better, d2, best)
                arg = torch.where(better, j, arg)
        n = tn[fidx, arg]
        has = (best <= md * md) & (n != 0).any(-1)
        e = (n * (q - tp[fidx, arg])).sum(-1)
        wt = torch.where(e.abs() <= huber, torch.ones_like(e), huber / e.abs())
        wt = torch.where(has, wt, torch.zeros_like(wt))
        e = torch.where(has, e, torch.zeros_like(e))
        m = n @ X32[:, :, :3]
        J = torch.cat([m, torch.cross(sp, m, dim=-1)], -1)
        J = torch.where(has[..., None], J, torch.zeros_like(J))
        A = ((J * wt[..., None]).transpose(1, 2) @ J).double()
        b = ((J * (wt * e)[..., None]).sum(1)).double()
        M = A + lam * torch.diag_embed(torch.diagonal(A, dim1=1, dim2=2)) + rg.EPS * torch.eye(6, dtype=torch.float64, device=dev)
        d = torch.cholesky_solve(-b[..., None], torch.linalg.cholesky(M))[..., 0]
        T = torch.linalg.matrix_exp(_hat6(d))
        X = torch.cat([X, torch.tensor([[[0.0, 0.0, 0.0, 1.0]]], dtype=torch.float64, device=dev).expand(F, 1, 4)], 1) @ T
        X = X[:, :3].contiguous()
    return X


def _hat6(d):
    """(F, 4, 4): the se(3) matrices of (F, 6) twists (rho, phi)."""
    G = torch.zeros((d.shape[0], 4, 4), dtype=d.dtype, device=d.device)
    G[:, 0, 1], G[:, 0, 2], G[:, 1, 2] = -d[:, 5], d[:, 4], -d[:, 3]
    G[:, 1, 0], G[:, 2, 0], G[:, 2, 1] = d[:, 5], -d[:, 4], d[:, 3]
    G[:, :3, 3] = d[:, :3]
    return G


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--pairs", type=int, nargs="*", default=[1, 16])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "registration.md"), help="the document the result is also written into")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_registration: needs a HIP device (a timing taken anywhere else says nothing)", file=sys.stderr)
        return 2
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device("cuda", 0)
    H, W, inc = a.height, a.width, list(rc.BOUNDS)
    sched = [tuple(r) for r in rg.DEFAULT_SCHEDULE]
    d_local = rc.local_directions(H, W, inc, "KITTI", None)

    def frame(pose):
        depth = rc.room_depth(d_local, pose)
        return rg.frame_geometry(depth.to(dev), torch.isfinite(depth).to(dev), inc, H, W)

    tgt1 = frame(np.eye(4))
    res = {"bench": "registration", "height": H, "width": W, "schedule": sched, "rounds": a.rounds, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", "").split(":")[0], "sources": build.reg_source_hash(),
           "unit": "milliseconds per align of all F pairs", "pairs": {}}
    q = lambda v, p: float(np.percentile(v, p))
    side = lambda v: {"median": q(v, 50), "p10": q(v, 10), "p90": q(v, 90)}
    for F in a.pairs:
        xis = [rc.twist(100 + f, 0.5, 2.0) for f in range(F)]
        srcs = [frame(rc.exp4(xi)) for xi in xis]
        src = tuple(torch.stack([s[k] for s in srcs]) for k in range(3))
        tgt = tuple(t[None].expand(F, *t.shape).contiguous() for t in tgt1)
        ws = torch.empty(rg.work_bytes(F, H, W), dtype=torch.uint8, device=dev)
        init = torch.eye(4, dtype=torch.float64, device=dev)[:3].expand(F, 3, 4).contiguous()
        flat = (src[0].reshape(F, H * W, 3), src[2].reshape(F, H * W), tgt[0].reshape(F, H * W, 3), tgt[1].reshape(F, H * W, 3), tgt[2].reshape(F, H * W))
        op = lambda: rg.align(src, tgt, init, sched, inclination=inc, workspace=ws)
        th = lambda: torch_align(*flat, sched, H, W, inc)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.reps * 1e3

        for _ in range(a.warmup):
            op(); th()
        t_op, t_th = [], []
        for _ in range(a.rounds):
            t_op.append(timed(op))
            t_th.append(timed(th))
        launches = {}
        for name, fn in (("operator", op), ("torch", th)):                   # untimed: the profiler slows the host
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            ev = [e for e in prof.key_averages() if e.device_time_total > 0]
            launches[name] = {"launches": int(sum(e.count for e in ev)), "kernel_ms": sum(e.device_time_total for e in ev) / 1e3,
                              "k_reg": int(sum(e.count for e in ev if "k_reg_" in e.key)),
                              **({k: sum(e.device_time_total for e in ev if k in e.key) / 1e3 for k in ("k_reg_linearize", "k_reg_solve")} if name == "operator" else {})}
        r = op()
        Xt = th()
        truth = torch.from_numpy(np.stack([rc.exp4(xi)[:3] for xi in xis]))
        err = lambda X: [rc.pose_error(X[f].cpu().numpy(), truth[f].numpy())[0] for f in range(F)]
        res["pairs"][str(F)] = {"operator": side(t_op), "torch": side(t_th), "ratio_torch_to_operator": q(t_th, 50) / q(t_op, 50), "launches": launches,
                                "status": r.status.cpu().tolist(), "translation_error_m": {"operator": max(err(r.X)), "torch": max(err(Xt))}}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(f"# Scan registration (`liblrt_reg.so`, `lidar_rt_amd/registration.py`): `tools/bench_registration.py` on {res['device']} ({res['arch']})\n\n"
                 f"Sources `{res['sources']}` (`build.reg_source_hash()`).  {H} x {W}, `DEFAULT_SCHEDULE` ({len(sched)} iterations), pairs of the analytic room of\n"
                 f"`tests/registration_cases.py` 0.5 m and 2 degrees apart.  Milliseconds per `align` of all F pairs, host clock around {a.reps} calls between two device\n"
                 f"synchronisations, {a.rounds} rounds per side alternating in one process after a warm-up of both; median (10th .. 90th percentile).  `torch` is the\n"
                 "rule as float32 torch expressions on the same device (one gather per window offset, the sums by matrix products, `torch.linalg.cholesky`).\n"
                 "Launches and summed kernel time are from a separate pass of one call under the torch profiler (copies and fills included).\n\n"
                 "| F | `align` | torch expressions | ratio | launches: `align` (of them `k_reg_*`) | launches: torch | kernel time `align` / torch, ms | of it `k_reg_linearize` / `k_reg_solve`, ms |\n|---:|---:|---:|---:|---:|---:|---:|---:|\n")
        for F, p in res["pairs"].items():
            o, t, l = p["operator"], p["torch"], p["launches"]
            fh.write(f"| {F} | {o['median']:.3f} ({o['p10']:.3f} .. {o['p90']:.3f}) | {t['median']:.2f} ({t['p10']:.2f} .. {t['p90']:.2f}) | {p['ratio_torch_to_operator']:.1f} | "
                     f"{l['operator']['launches']} ({l['operator']['k_reg']}) | {l['torch']['launches']} | {l['operator']['kernel_ms']:.3f} / {l['torch']['kernel_ms']:.2f} | "
                     f"{l['operator']['k_reg_linearize']:.3f} / {l['operator']['k_reg_solve']:.3f} |\n")
        fh.write("\nThe target window of a workgroup is not staged in LDS, and that variant was not tried: with one lane per source pixel and consecutive lanes on\n"
                 "consecutive columns the windows of a wave overlap, so its target loads already fall into few cache lines; a staged window would have to cover the\n"
                 "workgroup's whole range of centre pixels, which is not known before the projection and is unbounded under a large motion.\n\n"
                 "```json\n" + line + "\n```\n\n"
                 "## Resources (`resources.table_md`, hipcc `--offload-arch=" + build.ARCH + " " + " ".join(build.CODEGEN_FLAGS) + "`)\n\n"
                 + resources.table_md(resources.kernel_resources(build.REG_LIB)) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
