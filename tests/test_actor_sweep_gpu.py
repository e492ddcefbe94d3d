"""Actors that move within a sweep on the GPU (`liblrt_actorsweep.so` through `lidar_rt_amd.actor_sweep`): columns and counts equal to the float64
twin's, outputs and gradients within the bounds of tests/actor_sweep_cases.py, equal bits for equal inputs, a dirty workspace, no host wait, the
refused calls, the renderer's switch with all twists zero, and a physical test: a moving actor seen by a moving sensor, against a truth assembled
from one static render per column."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lidar_rt_amd import actor_sweep as asw, renderer, scenes, sweep, training
from lidar_rt_amd.sequence import TrackingBox
from tests import actor_sweep_cases as ac

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# P in {1, 63, 64, 65, 255, 256, 257, 1000}; an unposed asset in the middle, an empty asset and an asset boundary inside a wave ("mixed"); one workgroup
# spanning three assets ("three" at P <= 256); one asset spanning four workgroups ("one" at P = 1000); W in {64, 1030}; both conventions and directions
CASES = [ac.case(P, "mixed", 64) for P in ac.SIZES] + [
    ac.case(255, "three", 64, "waymo_yaw", "ccw"), ac.case(256, "three", 1030, "kitti", "ccw"), ac.case(257, "three", 1030, "waymo_yaw", "ccw"),
    ac.case(1000, "one", 1030), ac.case(1000, "one", 64), ac.case(256, "still", 64, "waymo_yaw"), ac.case(1000, "mixed", 1030, "waymo_yaw", "ccw"),
    ac.case(257, "mixed", 64, "kitti", "ccw"), ac.case(65, "mixed", 64, sensor_twist=None)]


def bits(t):
    t = t.detach().contiguous()
    return (t.view(torch.int32) if t.dtype == torch.float32 else t).cpu()


def run(c, workspace=None, **over):
    """Forward and backward of the operator on a case: (xyz_s, rot_s, column, counts, d_xyz, d_rot_raw, d_actor_twist) on the device."""
    kw = ac.arguments(c, DEV, **over)
    keep = {k: v.clone() for k, v in kw.items() if torch.is_tensor(v)}
    for k in ("xyz", "rot_raw", "actor_twist"):
        kw[k] = kw[k].requires_grad_(True)
    xyz_s, rot_s, info = asw.actor_sweep(**kw, workspace=workspace)
    torch.autograd.backward([xyz_s, rot_s], [c.g_xyz.to(DEV), c.g_rot.to(DEV)])
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(bits(kw[k]), bits(v)), f"{k} changed"
    return xyz_s.detach(), rot_s.detach(), info.column, info.counts, kw["xyz"].grad, kw["rot_raw"].grad, kw["actor_twist"].grad


def against_the_twin(c, got, label=""):
    xyz_s, rot_s, column, counts, dx, dr, dt = got
    r = c.ref
    assert xyz_s.dtype == rot_s.dtype == dx.dtype == dr.dtype == dt.dtype == torch.float32 and column.dtype == torch.int32 and counts.dtype == torch.int64
    assert xyz_s.shape == (c.P, 3) and rot_s.shape == (c.P, 4) and column.shape == (c.P,) and counts.shape == (4,) and dt.shape == (c.A, 6)
    assert torch.equal(column.cpu(), r.column), label
    assert counts.tolist() == r.counts.tolist() and int(counts[0] + counts[1]) == c.P, (label, counts.tolist(), r.counts.tolist())
    ex = {"xyz_s": ac.excess(xyz_s, r.xyz_s, r.A_xyz), "rot_s": ac.excess(rot_s, r.rot_s, r.A_rot), "d_xyz": ac.excess(dx, r.d_xyz, r.A_dx),
          "d_rot_raw": ac.excess(dr, r.d_rot, r.A_dr), "d_actor_twist": ac.twist_excess(dt, r.d_twist, r.A_tw)}
    print(f"{c.key[:5]} {label}: excess over the bounds: " + ", ".join(f"{k} {v:.3e}" for k, v in ex.items()))
    assert all(v <= 0.0 for v in ex.values()), (label, ex)
    passing = ~r.moved
    assert torch.equal(bits(xyz_s)[passing], bits(c.xyz)[passing]) and torch.equal(bits(rot_s)[passing], bits(c.rot)[passing]), label
    assert torch.equal(bits(dx)[passing], bits(c.g_xyz)[passing]) and torch.equal(bits(dr)[passing], bits(c.g_rot)[passing]), label
    dead = torch.tensor([not (p and m) for p, m in zip(c.posed, c.moving)]) | (c.seg[1:] == c.seg[:-1])
    assert float(dt.cpu()[dead].abs().sum()) == 0.0, label


# ---- 1. the operator against the twin -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", CASES, ids=lambda c: "-".join(str(k) for k in c.key[:5]) + ("" if c.sensor_twist is not None else "-static"))
def test_forward_and_backward_against_the_twin(c):
    against_the_twin(c, run(c))


def test_the_steering_arguments_may_live_on_the_device_and_no_gaussians_at_all():
    c = ac.case(257, "mixed", 64)
    a = run(c)
    b = run(c, sensor_pose=c.sensor_pose.to(DEV), sensor_twist=c.sensor_twist.to(DEV), tau=c.tau.to(DEV))
    for x, y in zip(a, b):
        assert torch.equal(bits(x), bits(y))
    e = ac.case(1, "mixed", 64)
    kw = ac.arguments(e, DEV, xyz=torch.zeros((0, 3), device=DEV), rot_raw=torch.zeros((0, 4), device=DEV), seg_start=torch.zeros(5, dtype=torch.int32, device=DEV))
    kw["actor_twist"] = kw["actor_twist"].requires_grad_(True)
    xs, rs, info = asw.actor_sweep(**kw)
    assert xs.shape == (0, 3) and rs.shape == (0, 4) and info.counts.tolist() == [0, 0, 0, 0]


# ---- 2. equal bits, a dirty workspace ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [ac.case(1000, "mixed", 1030, "waymo_yaw", "ccw"), ac.case(1000, "one", 64), ac.case(255, "three", 64, "waymo_yaw", "ccw")],
                         ids=lambda c: "-".join(str(k) for k in c.key[:5]))
def test_equal_inputs_give_equal_bits_and_a_dirty_workspace_does_not_leak(c):
    a = run(c)
    b = run(c)
    for x, y in zip(a, b):
        assert torch.equal(bits(x), bits(y))
    n = asw.work_bytes(c.P, c.A, c.W)
    for fill in (0xFF, 0x7F, 0x00):                                                             # NaNs, huge numbers, zeros in the table and the partial sums
        ws = torch.full((n + 256,), fill, dtype=torch.uint8, device=DEV)
        ws = ws[(-ws.data_ptr()) % 256:][:n]
        w = run(c, workspace=ws)
        for x, y in zip(a, w):
            assert torch.equal(bits(x), bits(y))
    other = ac.case(257, "three", 1030, "waymo_yaw", "ccw")                                      # another case's table and partial sums left behind
    big = torch.zeros(max(n, asw.work_bytes(other.P, other.A, other.W)), dtype=torch.uint8, device=DEV)
    against_the_twin(other, run(other, workspace=big), "shared workspace")
    for x, y in zip(a, run(c, workspace=big)):
        assert torch.equal(bits(x), bits(y))


# ---- 3. no host wait --------------------------------------------------------------------------------------------------------------------------------------------

def test_a_call_does_not_wait_for_the_device():
    c = ac.case(1000, "mixed", 1030, "waymo_yaw", "ccw")
    run(c)                                                                                      # warm: the loaded library, the allocators
    kw = ac.arguments(c, DEV)
    for k in ("xyz", "rot_raw", "actor_twist"):
        kw[k] = kw[k].requires_grad_(True)
    g_xyz, g_rot = c.g_xyz.to(DEV), c.g_rot.to(DEV)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        xyz_s, rot_s, info = asw.actor_sweep(**kw)
        torch.autograd.backward([xyz_s, rot_s], [g_xyz, g_rot])
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    against_the_twin(c, (xyz_s.detach(), rot_s.detach(), info.column, info.counts, kw["xyz"].grad, kw["rot_raw"].grad, kw["actor_twist"].grad), "sync debug mode")


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------------------------------

def test_refused_calls_raise_and_launch_nothing():
    c = ac.case(257, "mixed", 64)
    kw = ac.arguments(c, DEV)
    n = asw.work_bytes(c.P, c.A, c.W)
    ws = torch.full((n,), 0x5A, dtype=torch.uint8, device=DEV)
    with pytest.raises(asw.ActorSweepError, match="workspace must be a contiguous uint8 tensor"):
        asw.actor_sweep(**kw, workspace=ws[:n - 256])                                           # work_bytes too small
    with pytest.raises(asw.ActorSweepError, match="workspace must be a contiguous uint8 tensor"):
        asw.actor_sweep(**kw, workspace=ws.cpu())
    with pytest.raises(asw.ActorSweepError, match="columns"):
        asw.actor_sweep(**{**kw, "W": 0}, workspace=ws)
    with pytest.raises(asw.ActorSweepError, match="seg_start is on cpu"):
        asw.actor_sweep(**{**kw, "seg_start": c.seg}, workspace=ws)                             # a seg_start that is not on the device
    with pytest.raises(asw.ActorSweepError, match="float32"):
        asw.actor_sweep(**{**kw, "xyz": kw["xyz"].double()}, workspace=ws)
    # the library's own refusals, on the device that exists
    lib = asw.load()
    out = [torch.zeros(c.P * 4, dtype=torch.float32, device=DEV) for _ in range(3)]
    cnt = torch.full((4,), 77, dtype=torch.int64, device=DEV)
    d = torch.zeros(4096, dtype=torch.float64, device=DEV)
    p = lambda t: t.data_ptr()
    fwd = lambda W=64, xyz=p(kw["xyz"]), w2s=p(d), wb=n, col=p(out[2]): lib.lrt_actorsweep_forward(
        0, c.P, c.A, xyz, p(kw["rot_raw"]), p(kw["seg_start"]), p(kw["poses"]), p(kw["actor_twist"]), w2s, None, p(d), W, 0.0, 0.0, p(out[0]), p(out[1]), col,
        p(cnt), p(ws), wb, None)
    assert fwd(wb=n - 1) < 0 and b"a workspace of" in lib.lrt_actorsweep_last_error()
    assert fwd(W=0) < 0 and b"0 columns" in lib.lrt_actorsweep_last_error()
    assert fwd(xyz=None) < 0 and b"null xyz" in lib.lrt_actorsweep_last_error()
    assert fwd(w2s=None) < 0 and b"null world2sensor" in lib.lrt_actorsweep_last_error()
    assert fwd(col=None) < 0 and b"null xyz_s / rot_s / column / counts" in lib.lrt_actorsweep_last_error()
    bwd = lambda W=64, wb=n, dt=p(out[2]): lib.lrt_actorsweep_backward(
        0, c.P, c.A, p(kw["xyz"]), p(kw["rot_raw"]), p(kw["seg_start"]), p(kw["poses"]), p(kw["actor_twist"]), p(d), W, p(out[2]), p(out[0]), p(out[1]),
        p(out[0]), p(out[1]), dt, p(ws), wb, None)
    assert bwd(wb=n - 1) < 0 and b"a workspace of" in lib.lrt_actorsweep_last_error()
    assert bwd(W=-1) < 0 and b"-1 columns" in lib.lrt_actorsweep_last_error()
    assert bwd(dt=None) < 0 and b"null d_actor_twist" in lib.lrt_actorsweep_last_error()
    torch.cuda.synchronize()
    assert bool((ws == 0x5A).all()) and all(float(o.abs().sum()) == 0.0 for o in out) and cnt.tolist() == [77] * 4, "a refused call wrote"
    against_the_twin(c, run(c, workspace=ws), "after the refusals")


# ---- 5. the renderer's switch -------------------------------------------------------------------------------------------------------------------------------------

INC = (-0.15, 0.15)
H, W = 8, 64
LINE = np.array([math.cos(0.75 * math.pi), math.sin(0.75 * math.pi), 0.0])                       # the azimuth of column 8: tau = -0.3672 sweeps
ACROSS = np.array([-LINE[1], LINE[0], 0.0])
SENSOR_TWIST = (2.0, 0.0, 0.0, 0.0, 0.0, 0.0)                                                    # 2 m forward over the sweep
ACTOR_TWIST = (0.0, 3.0, 0.0, 0.0, 0.0, 0.0)                                                     # 3 m along the actor's y: across the line of sight
ACTOR_RANGE, WALL_RANGE = 10.0, 20.0
SPACING, SIGMA = 0.2, 0.12                                                                       # of the actor's Gaussians


def _asset(xyz, normal, sigma, box=None):
    n = xyz.shape[0]
    f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)
    rot = scenes._frame_quaternions(np.tile(np.asarray(normal, np.float64), (n, 1)), np.zeros(n))
    return SimpleNamespace(_xyz=f32(xyz), _scaling=torch.full((n, 2), math.log(sigma), device=DEV), _rotation=f32(rot), _opacity=torch.full((n, 1), 5.0, device=DEV),
                           get_features=torch.zeros((n, 16, 3), device=DEV), active_sh_degree=0, bounding_box=box)


def moving_scene():
    """A static wall 20 m away and, 10 m away on the line of sight of column 8, an actor: a plate of 26 x 13 Gaussians that faces the sensor."""
    u, v = np.meshgrid(np.arange(-12.0, 12.01, 0.3), np.arange(-5.0, 5.01, 0.3), indexing="ij")
    wall = WALL_RANGE * LINE[None] + u.reshape(-1, 1) * ACROSS[None] + v.reshape(-1, 1) * np.array([[0.0, 0.0, 1.0]])
    y, z = np.meshgrid(np.arange(-2.5, 2.51, SPACING), np.arange(-1.2, 1.21, SPACING), indexing="ij")
    plate = np.stack([np.zeros(y.size), y.reshape(-1), z.reshape(-1)], 1)
    box = TrackingBox([0.5, 5.2, 2.6], DEV)
    yaw = 0.75 * math.pi                                                                        # the actor's x axis is the line of sight
    t = torch.tensor(ACTOR_RANGE * LINE, dtype=torch.float32, device=DEV)
    q = torch.tensor([[math.cos(yaw / 2), 0.0, 0.0, math.sin(yaw / 2)]], dtype=torch.float32, device=DEV)
    box.frame[0] = (t, q, None, None)
    frames = training.RangeFrames()
    zeros = torch.zeros((H, W), device=DEV)
    frames.add_range_image(0, zeros, zeros, torch.ones((H, W), dtype=torch.bool, device=DEV), INC, torch.eye(4, device=DEV), twist=torch.tensor(SENSOR_TWIST))
    return [_asset(wall, LINE, 0.25), _asset(plate, [1.0, 0.0, 0.0], SIGMA, box)], box, frames, (t, q)


def _depth(assets, sensor, frame=0):
    with torch.no_grad():
        pkg = renderer.raytracing(frame, assets, sensor, torch.tensor(scenes.BG_DEFAULT), SimpleNamespace(dynamic=True))
    return pkg["depth"][..., 0].clone()


def test_all_twists_zero_with_the_switch_on_gives_the_bits_of_today():
    assets, box, frames, _ = moving_scene()
    want = [t.clone() for t in renderer._fused_inputs(0, assets, True, False, frames)]
    before = renderer.actor_sweep
    renderer.actor_sweep = True
    try:
        no_twist = renderer._fused_inputs(0, assets, True, False, frames)                       # no posed asset has a twist: the stage does not run
        box.twist[0] = torch.zeros(6, device=DEV)
        renderer.last_actor_sweep = None
        zero = renderer._fused_inputs(0, assets, True, False, frames)
        info = renderer.last_actor_sweep
        box.twist[0] = torch.tensor(ACTOR_TWIST, device=DEV)
        moved = renderer._fused_inputs(0, assets, True, False, frames)
    finally:
        renderer.actor_sweep = before
    n = assets[1]._xyz.shape[0]
    for got in (no_twist, zero):
        for a, b in zip(got, want):                                                             # means, scales, rotations, opacities
            assert torch.equal(bits(a), bits(b))
    assert info is not None and info.counts.tolist() == [0, want[0].shape[0], 0, 0] and bool((info.column == -1).all())
    assert renderer.last_actor_sweep.counts.tolist()[0] == n and not torch.equal(moved[0][-n:], want[0][-n:]) and torch.equal(bits(moved[0][:-n]), bits(want[0][:-n]))


# ---- 6. the physical test -----------------------------------------------------------------------------------------------------------------------------------------

def test_a_moving_actor_seen_by_a_moving_sensor_against_one_static_render_per_column():
    """H = 8, W = 64, inclinations +-0.15 rad.  The sensor moves 2 m along x over the sweep; the actor, a plate of 26 x 13 Gaussians (sigma 0.12 m, 0.2 m
    apart) 10 m away on the line of sight of column 8 (tau = -0.367 sweeps), moves 3 m along its own y axis, across that line; a wall stands 20 m away.

    Truth: for each column w the scene with the actor at A Exp(tau[w] eta), rendered by the existing static path with that column's 8 sweep rays alone
    (`sensor` as a tuple); the 64 renders are assembled into one image.  A pixel "hits the actor" when its depth lies in (5, 15) m.

    On the pixels where truth or render hits the actor, the actor-sweep render's silhouette mismatch count and its mean |depth error| are strictly
    below the plain sweep render's: at tau = -0.367 the plain render leaves the actor 1.1 m -- more than the 0.98 m a column is wide at 10 m -- from
    where the sensor saw it.

    The bound on the depth error, on the pixels where truth AND the actor-sweep render hit the actor (elsewhere the error is the 10 m between actor
    and wall, which the mismatch count measures): a Gaussian is placed at the instant of its centre's column and is seen by a column at most
    (columns it spans + 1) away, that is (columns + 1) / W sweeps earlier or later, during which actor and sensor move against each other by the
    relative speed |3 ACROSS - 2 x| = |(-2.121 - 2, -2.121, 0)| = 4.636 m per sweep.  A Gaussian reaches 3 sigma = 0.36 m to either side, 0.72 m,
    less than the 0.98 m of a column: it spans at most 2 columns.  Bound: 4.636 * (2 + 1) / 64 = 0.2173 m; a displacement of that size moves the
    depth of a surface by no more than itself."""
    assets, box, frames, (t0, q0) = moving_scene()
    tau = sweep.column_times(W)
    o, d = frames.rays[0]
    before = renderer.actor_sweep
    renderer.actor_sweep = False
    try:
        plain = _depth(assets, frames)
        truth = torch.zeros((H, W), device=DEV)
        Ra = training._rotation_matrix(q0).reshape(3, 3)
        for w in range(W):
            shift = Ra @ (float(tau[w]) * torch.tensor(ACTOR_TWIST[:3], device=DEV))               # Exp of a pure translation
            box.frame[1] = (t0 + shift, q0, None, None)                                         # frame 1: a ray set of its own, 8 rays
            truth[:, w] = _depth(assets, (o[:, w:w + 1].contiguous(), d[:, w:w + 1].contiguous(), o[0, w]), 1)[:, 0]
        box.twist[0] = torch.tensor(ACTOR_TWIST, device=DEV)
        renderer.actor_sweep = True
        swept = _depth(assets, frames)
        counts = renderer.last_actor_sweep.counts.tolist()
    finally:
        renderer.actor_sweep = before
    on = lambda img: (img > 5.0) & (img < 15.0)
    assert int(on(truth).sum()) >= 20 and counts[0] == assets[1]._xyz.shape[0] and counts[3] == 0

    def figures(img):
        union = on(truth) | on(img)
        both = on(truth) & on(img)
        return int((on(truth) != on(img)).sum()), float((img - truth).abs()[union].mean()), float((img - truth).abs()[both].mean()) if bool(both.any()) else float("nan")
    rel = np.linalg.norm(3.0 * ACROSS - np.array([2.0, 0.0, 0.0]))
    bound = rel * (2 + 1) / W
    ms, es, bs = figures(swept)
    mp, ep, bp = figures(plain)
    line = (f"physical test: actor pixels in truth {int(on(truth).sum())}; silhouette mismatches actor-sweep {ms} / plain sweep {mp}; mean |depth error| on the "
            f"union actor-sweep {es:.4f} m / plain sweep {ep:.4f} m; on the pixels both hit actor-sweep {bs:.5f} m / plain sweep {bp:.5f} m; bound {bound:.4f} m")
    print(line)
    dst = os.environ.get("LRT_ACTOR_SWEEP_OUT")                                                 # where to keep the figures for profiles/actor_sweep.md
    if dst:
        with open(dst, "w") as f:
            f.write(line + "\n")
    assert abs(rel - 4.636) < 1e-3
    assert ms < mp and es < ep, line
    assert bs < bound and es < bound, line                                                      # on the pixels both hit, and on the union the issue names


# ---- 7. the training loop, the sequence tool, the simulator ------------------------------------------------------------------------------------------------------

def test_train_on_a_sequence_of_moving_actors_refines_the_twists_resumes_them_and_simulates(tmp_path, capsys):
    import json
    import subprocess
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import make_sequence
    from lidar_rt_amd import sequence
    data, frozen = str(tmp_path / "seq"), str(tmp_path / "frozen")
    make_sequence.make("kitti360_dynamic", data, n_frames=4, scale=0.01, sweep_speed=2.0, hw=(8, 64), actor_sweep=True)
    make_sequence.make("kitti360_dynamic", frozen, n_frames=4, scale=0.01, sweep_speed=2.0, hw=(8, 64))
    # the tool: the twists are stored, they are the boxes' own, and the ground truth differs from the one with frozen actors
    stored = sequence.load_sequence(data, device="cpu", actor_sweep="stored").boxes
    derived = sequence.load_sequence(data, device="cpu", actor_sweep="boxes").boxes
    assert "twist" not in np.load(os.path.join(frozen, "boxes.npz")).files and len(stored) == 8
    for a_, b_ in zip(stored, derived):
        assert sorted(a_.twist) == [0, 1, 2, 3] and all(torch.allclose(a_.twist[f], b_.twist[f], atol=1e-6) for f in a_.twist) and float(a_.twist[0].abs().max()) > 0.0
    depth = lambda root, f: np.load(os.path.join(root, "frames", f"{f:06d}.npz"))["depth"]
    assert any(not np.array_equal(depth(data, f), depth(frozen, f)) for f in range(4))
    common = ["--data", data, "--log-every", "1", "--save-every", "5", "--max-points", "20000", "--sweep", "stored"]
    run = lambda out, extra: subprocess.run([sys.executable, "-m", "lidar_rt_amd.train", "--out", out] + common + extra, cwd=REPO, capture_output=True, text=True,
                                            timeout=600)
    on = ["--actor-sweep", "stored", "--refine-actor-twist", "--actor-twist-lr-trans", "1e-2"]
    # with --refine-poses --refine-twist the stage reads the sensor's CURRENT pose and twist (a poses.SensorPoses)
    a = run(str(tmp_path / "a"), ["--iters", "5", "--refine-poses", "--refine-twist"] + on)
    assert a.returncode == 0, a.stdout[-2000:] + a.stderr[-3000:]
    rows = [json.loads(l) for l in a.stdout.splitlines() if l.startswith("{") and "iteration" in l]
    assert [r["iteration"] for r in rows] == [1, 2, 3, 4, 5] and all(np.isfinite(r["loss"]) for r in rows)
    load = lambda p_: torch.load(p_, map_location="cpu", weights_only=False)
    sd = load(tmp_path / "a" / "actor_twists5.pth")
    assert len(sd["eta"]) == 8 * 4                                                              # 8 actors with a box in each of the 4 frames
    moved = [float((sd["eta"][(a_, f)] - stored[a_].twist[f]).abs().max()) for (a_, f) in sd["eta"]]
    assert all(np.isfinite(m) for m in moved) and max(moved) > 0.0, moved                       # the twists move
    # the checkpoint resumes, the twists with it: one more iteration at learning rates of zero must write back exactly what was saved
    b = run(str(tmp_path / "b"), ["--iters", "6", "--resume", str(tmp_path / "a" / "chkpnt5.pth"), "--actor-sweep", "stored", "--refine-actor-twist",
                                  "--actor-twist-lr-trans", "0", "--actor-twist-lr-rot", "0"])
    assert b.returncode == 0 and "is missing" not in b.stderr, b.stdout[-2000:] + b.stderr[-3000:]
    rb = load(tmp_path / "b" / "actor_twists6.pth")
    assert all(torch.equal(rb["eta"][k], sd["eta"][k]) for k in sd["eta"])
    assert any(not torch.equal(rb["eta"][(a_, f)], stored[a_].twist[f]) for (a_, f) in rb["eta"])
    plain = run(str(tmp_path / "c"), ["--iters", "5"])                                          # a checkpoint written without the switch ...
    assert plain.returncode == 0 and not os.path.exists(tmp_path / "c" / "actor_twists5.pth"), plain.stdout[-2000:] + plain.stderr[-3000:]
    d = run(str(tmp_path / "d"), ["--iters", "6", "--resume", str(tmp_path / "c" / "chkpnt5.pth"), "--actor-sweep", "boxes", "--refine-actor-twist"])      # ... still loads, and says so
    assert d.returncode == 0 and os.path.exists(tmp_path / "d" / "actor_twists6.pth") and "actor_twists5.pth is missing" in d.stderr, d.stdout[-2000:] + d.stderr[-3000:]
    from lidar_rt_amd import train                                                              # the refusals come from the argument parser, before any device
    for bad, msg in ((["--actor-sweep", "boxes", "--sweep", "off"], "--actor-sweep needs a sweep"), (["--refine-actor-twist"], "--refine-actor-twist needs --actor-sweep"),
                     (on + ["--gpus", "2"], "refused with --gpus")):
        with pytest.raises(SystemExit) as e:
            train.main(["--out", str(tmp_path / "x"), "--data", data, "--sweep", "stored", "--iters", "1"] + bad)
        assert e.value.code == 2 and msg in capsys.readouterr().err
    # the simulator: a moved actor keeps its twist, and the scan of moving actors is another one than the scan of frozen ones
    from lidar_rt_amd import simulate
    # every pixel is kept (a ray-drop ratio above 1) and the twists given with --actor-twists are large, 6 m and 0.5 rad per sweep, so that the few
    # rays of an 8 x 64 image that meet an actor of this small scene see it elsewhere
    sim = dict(data=data, ckpt=str(tmp_path / "a" / "chkpnt5.pth"), frames="all", max_points=20000, sweep="stored", raydrop_ratio=1.01,
               move_actor=[[0, 0.0, 1.0, 0.0, 10.0]], remove_actor=[1])
    large = str(tmp_path / "large_twists.pth")
    torch.save({"eta": {k: torch.tensor([0.0, 6.0, 0.0, 0.0, 0.0, 0.5]) for k in sd["eta"]}}, large)
    before = renderer.actor_sweep
    r_on = simulate.simulate(out=str(tmp_path / "s_on"), actor_sweep="stored", actor_twists=large, **sim)
    r_off = simulate.simulate(out=str(tmp_path / "s_off"), **sim)
    assert renderer.actor_sweep == before and r_on["arguments"]["actor_sweep"] == "stored" and r_off["arguments"]["actor_sweep"] == "off"
    assert renderer.last_actor_sweep is not None and int(renderer.last_actor_sweep.counts[0]) > 0
    cloud = lambda root, f: np.fromfile(os.path.join(root, f"{f:06d}.bin"), np.float32)
    ids = [fr["id"] for fr in r_on["frames"]]
    differ = [f for f in ids if cloud(str(tmp_path / "s_on"), f).tobytes() != cloud(str(tmp_path / "s_off"), f).tobytes()]
    print(f"simulate --actor-sweep: frames whose cloud differs from the frozen actors' {differ} of {ids}; counts {renderer.last_actor_sweep.counts.tolist()}")
    assert differ
    with pytest.raises(simulate.SimulateError, match="--actor-sweep needs a moving sensor"):
        simulate.simulate(out=str(tmp_path / "s_x"), actor_sweep="stored", **{**sim, "sweep": "off"})
