"""Sensor pose refinement through the tracer's ray gradients: a frame rendered at a true pose, a recorded pose 0.15 m and 0.5 deg
(yaw and pitch) off, frozen Gaussians, masked depth L1 -- poses.SensorPoses must remove at least two thirds of both errors in at most
300 steps (the gate was fixed before the first run).  With LRT_POSE_REFINE_OUT=FILE the curve is written to FILE as JSON (the
table of profiles/pose_refine.md)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from lidar_rt_amd import poses, scenes, training
from lidar_rt_amd.diff_lidar_tracer import Tracer

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tests.hip_util import settings, DEV, DEFAULT_OPTS

KB = [math.radians(-24.9), math.radians(2.0)]
H, W = 32, 1024
STEPS = 300


def _rot(axis, deg):
    a = math.radians(deg); c, s = math.cos(a), math.sin(a)
    R = torch.eye(4, dtype=torch.float32)
    i, j = {"z": (0, 1), "y": (2, 0)}[axis]
    R[i, i] = c; R[i, j] = -s; R[j, i] = s; R[j, j] = c
    return R


def _errors(s2w, true):
    s2w, true = s2w.double(), true.double()
    dt = float(torch.linalg.norm(s2w[:3, 3] - true[:3, 3]))
    Rr = s2w[:3, :3].T @ true[:3, :3]
    sk = torch.stack([Rr[2, 1] - Rr[1, 2], Rr[0, 2] - Rr[2, 0], Rr[1, 0] - Rr[0, 1]])
    ang = math.degrees(math.atan2(0.5 * float(torch.linalg.norm(sk)), 0.5 * (float(torch.trace(Rr)) - 1.0)))
    return dt, ang


def test_pose_refinement_recovers_a_perturbed_pose():
    sc = scenes.make_scene(200_000, radius_scale=1.0 / 3.0)
    t = {k: torch.as_tensor(v, device=DEV) for k, v in sc.items()}         # frozen: no requires_grad
    tr = Tracer()
    for k, v in DEFAULT_OPTS.items():
        tr.optix_context.set_option(k, v)
    tr.build_from_gaussians(t["means"], t["scales"], t["rotations"], t["opacities"])
    st = settings(scenes.BG_DEFAULT, 3)

    def render(o, d):
        out, _ = tr(o, d, None, t["means"], torch.zeros_like(t["means"]), shs=t["shs"], opacities=t["opacities"],
                    scales=t["scales"], rotations=t["rotations"], tracer_settings=st)
        return out

    true = torch.eye(4, dtype=torch.float32); true[:3, 3] = torch.tensor([0.3, -0.2, 0.1])
    true = true @ _rot("z", 10.0)
    o, d = training.RangeFrames.range_rays(H, W, KB, true.to(DEV))
    with torch.no_grad():
        target = render(o, d)
    gt_depth = target[..., 3].clone()
    mask = target[..., 4] > 0.5                                            # rays that hit something
    assert mask.float().mean() > 0.3

    off = torch.tensor([0.1, -0.1, 0.05]); off = off / off.norm() * 0.15
    init = true.clone(); init[:3, 3] += off
    init = init @ _rot("z", 0.5) @ _rot("y", 0.5)
    fr = training.RangeFrames()
    fr.add_range_image(0, gt_depth, torch.zeros_like(gt_depth), mask, KB, init.to(DEV))
    sp = poses.SensorPoses(fr, [0], lr_trans=3e-3, lr_rot=1e-4)
    e0 = _errors(init, true)
    curve = [(0,) + e0]
    mf = mask.float()
    for it in range(1, STEPS + 1):
        sp.zero_grad()
        ro, rd = sp.get_range_rays(0)
        out = render(ro, rd)
        loss = ((out[..., 3] - gt_depth).abs() * mf).sum() / mf.sum()
        loss.backward()
        sp.step()
        if it % 10 == 0:
            curve.append((it,) + _errors(sp.sensor2world(0).detach().cpu(), true))
    e1 = curve[-1][1:]
    dst = os.environ.get("LRT_POSE_REFINE_OUT")
    if dst:
        with open(dst, "w") as f:
            json.dump({"steps": STEPS, "init": e0, "final": e1, "curve": curve}, f)
    assert e1[0] <= e0[0] / 3.0, curve
    assert e1[1] <= e0[1] / 3.0, curve


def test_train_entry_refines_poses_and_resumes_them(tmp_path):
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(repo, "tools"))
    import make_sequence
    data = str(tmp_path / "seq")
    make_sequence.make("kitti360_dynamic", data, n_frames=4, scale=0.1)
    common = ["--data", data, "--log-every", "5", "--save-every", "10", "--max-points", "60000", "--refine-poses", "--pose-lr-trans", "1e-3"]
    run = lambda out, extra: subprocess.run([sys.executable, "-m", "lidar_rt_amd.train", "--out", out] + common + extra, cwd=repo,
                                            capture_output=True, text=True, timeout=1200)
    a = run(str(tmp_path / "a"), ["--iters", "20"])
    assert a.returncode == 0, a.stdout[-2000:] + a.stderr[-3000:]
    for it in (10, 20):
        assert os.path.exists(tmp_path / "a" / f"chkpnt{it}.pth") and os.path.exists(tmp_path / "a" / f"poses{it}.pth")
    params, it20 = torch.load(tmp_path / "a" / "chkpnt20.pth", map_location="cpu", weights_only=False)
    assert it20 == 20 and len(params[0]) == 12                                 # the checkpoint tuple is unchanged
    p10 = torch.load(tmp_path / "a" / "poses10.pth", map_location="cpu", weights_only=False)
    p20 = torch.load(tmp_path / "a" / "poses20.pth", map_location="cpu", weights_only=False)
    moved = [float((p20["xi"][f] - p10["xi"][f]).abs().max()) for f in p20["xi"]]
    assert all(np.isfinite(m) for m in moved) and max(moved) > 0, moved      # the corrections are learnt
    b = run(str(tmp_path / "b"), ["--iters", "20", "--resume", str(tmp_path / "a" / "chkpnt10.pth")])
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-3000:]
    assert os.path.exists(tmp_path / "b" / "poses20.pth")
