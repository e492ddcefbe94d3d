"""Actor box refinement on the GPU.

Recovery: a static background plus one car-sized actor, frozen Gaussians, a range image rendered at the actor's true box pose; the recorded
box 0.2 m and 2 deg (yaw) off; masked depth L1 through the fused pre-processing and the tracer -- actor_poses.ActorPoses must remove at least
two thirds of both errors within 300 steps (the gate was fixed before the first run).

Entry points: python -m lidar_rt_amd.train --refine-boxes on a reduced kitti360_dynamic sequence writes boxes<it>.pth; with --deterministic a
resumed run's parameters and box corrections (and, with --refine-poses, sensor corrections) equal the uninterrupted run's bit for bit; python -m lidar_rt_amd.evaluate --boxes renders with
them; with --gpus 2 on one device (gloo) the ranks' corrections are verified identical after every step (training_step raises otherwise)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lidar_rt_amd import actor_poses, scenes, training
from lidar_rt_amd.diff_lidar_tracer import Tracer
from lidar_rt_amd.preprocess import fused_activations, pack_poses
from lidar_rt_amd.sequence import TrackingBox

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if torch.cuda.is_available():
    from tests.hip_util import settings, DEV, DEFAULT_OPTS

KB = [math.radians(-24.9), math.radians(2.0)]
H, W = scenes.KITTI360_HW
STEPS = 300


def _yaw_q(deg):
    a = math.radians(deg)
    return np.array([math.cos(a / 2), 0.0, 0.0, math.sin(a / 2)])


def _qmul(a, b):
    aw, ax, ay, az = a; bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def _errors(t, q, t_true, q_true):
    R = lambda q_: training._rotation_matrix(torch.as_tensor(np.asarray(q_, np.float64)).reshape(1, 4)).squeeze(0)
    Rr = R(q).T @ R(q_true)
    ang = math.degrees(math.acos(max(-1.0, min(1.0, 0.5 * (float(torch.trace(Rr)) - 1.0)))))
    return float(np.linalg.norm(np.asarray(t, np.float64) - t_true)), ang


def test_box_refinement_recovers_a_perturbed_actor_pose():
    rng = np.random.default_rng(17)
    bg = scenes.make_scene(150_000, seed=scenes.SEED + 29, radius_scale=1.0)
    car = scenes.actor_asset(20_000, rng)
    counts = [bg["means"].shape[0], car["means"].shape[0]]
    cat = lambda k: torch.as_tensor(np.concatenate([bg[k], car[k]], 0), device=DEV)
    xyz, rot, shs = cat("means"), cat("rotations"), cat("shs")
    ls, lo = torch.log(cat("scales")), training.inverse_sigmoid(cat("opacities"))        # frozen: nothing requires grad
    t_true = np.array([8.0, 3.0, scenes.GROUND_Z])
    q_true = _yaw_q(35.0) * 1.3                                                       # stored non-unit, as boxes may be
    off = np.array([0.6, -0.8, 0.0]) * 0.2
    t_rec, q_rec = t_true + off, _qmul(q_true, _yaw_q(2.0))
    tr = Tracer()
    for k, v in DEFAULT_OPTS.items():
        tr.optix_context.set_option(k, v)
    st = settings(scenes.BG_DEFAULT, 3)
    o, d = training.RangeFrames.range_rays(H, W, KB, torch.eye(4, device=DEV))

    def render(pose):
        seg, tab = pack_poses([None, pose], counts, DEV)
        m, s, r, op = fused_activations(xyz, ls, rot, lo, seg, tab)
        tr.build_from_gaussians(m.detach(), s.detach(), r.detach(), op.detach())
        out, _ = tr(o, d, None, m, torch.zeros_like(m), shs=shs, opacities=op, scales=s, rotations=r, tracer_settings=st)
        return out

    f32 = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV)
    with torch.no_grad():
        target = render((f32(t_true), f32(q_true).reshape(1, 4)))
        away = render((f32(t_true + np.array([0.0, 0.0, 100.0])), f32(q_true).reshape(1, 4)))
    gt_depth = target[..., 3].clone()
    mask = target[..., 4] > 0.5
    assert float(((target[..., 3] - away[..., 3]).abs() > 0.1).float().mean()) > 0.005        # the car covers part of the image
    tb = TrackingBox([4.4, 1.9, 1.6], DEV)
    tb.frame[0] = (f32(t_rec), f32(q_rec).reshape(1, 4), None, None)
    ap = actor_poses.ActorPoses([tb], [0], lr_trans=5e-3, lr_rot=1e-3)
    e0 = _errors(t_rec, q_rec, t_true, q_true)
    curve = [(0,) + e0]
    mf = mask.float()
    for it in range(1, STEPS + 1):
        ap.zero_grad()
        t, q, _, _ = ap.views[0].frame[0]
        out = render((t, q))
        loss = ((out[..., 3] - gt_depth).abs() * mf).sum() / mf.sum()
        loss.backward()
        ap.step()
        if it % 10 == 0:
            t, q, _, _ = ap.views[0].frame[0]
            curve.append((it,) + _errors(t.detach().cpu().double().numpy(), q.detach().cpu().double().numpy().reshape(4), t_true, q_true))
    e1 = curve[-1][1:]
    dst = os.environ.get("LRT_BOX_REFINE_OUT")
    if dst:
        with open(dst, "w") as f:
            json.dump({"steps": STEPS, "init": e0, "final": e1, "curve": curve}, f)
    assert e1[0] <= e0[0] / 3.0, curve
    assert e1[1] <= e0[1] / 3.0, curve


def _load(p):
    return torch.load(p, map_location="cpu", weights_only=False)


# --deterministic repeats a run bit for bit when no loss term adds with float atomics.  With boxes alone that holds at the default options (the
# Chamfer term carries no gradient: its points come from the frames' fixed rays and the detached depth).  With --refine-poses the Chamfer points
# come from the refined rays, so their gradient reaches the sensor poses through the Chamfer backward's float atomics: lambda_cd = 0 there, the
# condition --deterministic states for itself.
RESUME_CASES = {"boxes": [], "boxes_and_sensor_poses": ["--refine-poses", "--opt", "lambda_cd=0"]}


@pytest.mark.parametrize("case", list(RESUME_CASES))
def test_train_entry_refines_boxes_resumes_them_bit_for_bit_and_evaluates_with_them(tmp_path, case):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import make_sequence
    data = str(tmp_path / "seq")
    make_sequence.make("kitti360_dynamic", data, n_frames=4, scale=0.1)
    common = ["--data", data, "--log-every", "1", "--save-every", "10", "--max-points", "60000", "--deterministic", "--refine-boxes",
              "--box-lr-trans", "1e-3"] + RESUME_CASES[case]
    run = lambda out, extra: subprocess.run([sys.executable, "-m", "lidar_rt_amd.train", "--out", out] + common + extra, cwd=REPO,
                                            capture_output=True, text=True, timeout=1200)
    a = run(str(tmp_path / "a"), ["--iters", "20"])
    assert a.returncode == 0, a.stdout[-2000:] + a.stderr[-3000:]
    for it in (10, 20):
        assert os.path.exists(tmp_path / "a" / f"boxes{it}.pth") and os.path.exists(tmp_path / "a" / f"chkpnt{it}.pth")
    b10, b20 = _load(tmp_path / "a" / "boxes10.pth"), _load(tmp_path / "a" / "boxes20.pth")
    assert len(b20["xi"]) == 8 * 4                                               # 8 actors with a box in each of the 4 training frames
    moved = [float((b20["xi"][k] - b10["xi"][k]).abs().max()) for k in b20["xi"]]
    assert all(np.isfinite(m) for m in moved) and max(moved) > 0, moved         # the corrections are learnt
    b = run(str(tmp_path / "b"), ["--iters", "20", "--resume", str(tmp_path / "a" / "chkpnt10.pth")])
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-3000:]
    rb = _load(tmp_path / "b" / "boxes20.pth")
    for k in b20["xi"]:
        assert torch.equal(b20["xi"][k], rb["xi"][k]), k
    pa, pb = _load(tmp_path / "a" / "chkpnt20.pth")[0], _load(tmp_path / "b" / "chkpnt20.pth")[0]
    for ga, gb in zip(pa, pb):
        for i in (1, 2, 3, 4, 5, 6):
            assert torch.equal(ga[i].detach().cpu(), gb[i].detach().cpu()), i
    if "--refine-poses" in common:
        sa, sb = _load(tmp_path / "a" / "poses20.pth"), _load(tmp_path / "b" / "poses20.pth")
        for f in sa["xi"]:
            assert torch.equal(sa["xi"][f], sb["xi"][f]), f
        return
    e = subprocess.run([sys.executable, "-m", "lidar_rt_amd.evaluate", "--data", data, "--ckpt", str(tmp_path / "a" / "chkpnt20.pth"), "--frames", "all",
                        "--use-gt-mask", "--max-points", "60000", "--boxes", str(tmp_path / "a" / "boxes20.pth")], cwd=REPO, capture_output=True, text=True,
                       timeout=900)
    assert e.returncode == 0, e.stdout[-2000:] + e.stderr[-3000:]
    res = json.loads([l for l in e.stdout.splitlines() if l.startswith("{")][-1])
    assert len(res["frames"]) == 4 and all(np.isfinite(v) for ms in res["mean"].values() for v in ms.values())


def test_two_ranks_on_one_gpu_keep_identical_box_corrections(tmp_path):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import make_sequence
    data = str(tmp_path / "seq")
    make_sequence.make("kitti360_dynamic", data, n_frames=4, scale=0.1)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", LRT_SINGLE_DEVICE="1", LRT_DIST_BACKEND="gloo")
    r = subprocess.run([sys.executable, "-m", "lidar_rt_amd.train", "--data", data, "--out", str(tmp_path / "out"), "--gpus", "2", "--iters", "6",
                        "--log-every", "1", "--save-every", "6", "--max-points", "60000", "--refine-boxes", "--box-lr-trans", "1e-3"],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]                # training_step compares the ranks' corrections after every step
    sd = _load(tmp_path / "out" / "boxes6.pth")
    assert max(float(x.abs().max()) for x in sd["xi"].values()) > 0
