"""Sweep rays on the GPU: forward and backward of `liblrt_sweep.so` against the float64 twin on every case of tests/sweep_cases.py, equal bits
for equal inputs, frames in one call against frames one by one, a dirty workspace, unchanged inputs, no host wait inside a call, the grid
operators fed per-column origins, and the training / evaluation loop on a sequence of a moving sensor."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lidar_rt_amd import sweep as sw
from tests import sweep_cases as sc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def bits(t):
    return t.contiguous().view(torch.int32)


def run(c, workspace=None, frames=None):
    """Forward and backward of the operator on a case (or on some of its frames): (o, d, d_pose, d_twist) on the device."""
    sel = slice(None) if frames is None else frames
    pose = c.pose[sel].to(DEV).requires_grad_(True)
    twist = None if c.twist is None else c.twist[sel].to(DEV).requires_grad_(True)
    o, d = sw.sweep_rays(pose, twist, **c.kw, workspace=workspace)
    torch.autograd.backward([o, d], [c.g_o[sel].to(DEV), c.g_d[sel].to(DEV)])
    return o.detach(), d.detach(), pose.grad, None if twist is None else twist.grad


# ---- 6. / 7. forward and backward against the twin -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", sc.all_cases(), ids=lambda c: c.key)
def test_forward_and_backward_against_the_twin(c):
    r = sc.reference(c)
    o, d, dp, dt = run(c)
    assert o.shape == d.shape == (c.F, c.H, c.W, 3) and o.dtype == d.dtype == torch.float32 and o.is_contiguous() and d.is_contiguous()
    fd, fo = sc.forward_excess(d, r.d, 1.0), sc.forward_excess(o, r.o, r.scale)
    bp = sc.backward_excess(dp.reshape(c.F, 12), r.d_pose.reshape(c.F, 12), r.A[:, :12])
    bt = None if dt is None else sc.backward_excess(dt, r.d_twist, r.A[:, 12:])
    print(f"{c.key}: excess over the bounds: directions {fd:.3e}, origins {fo:.3e}, d_pose {bp:.3e}, d_twist {bt if bt is None else format(bt, '.3e')}")
    assert fd <= 0.0 and fo <= 0.0
    assert dp.shape == (c.F, 3, 4) and dp.dtype == torch.float32 and bp <= 0.0
    if c.twist is None:
        assert dt is None
        assert torch.equal(o.cpu(), c.pose[:, None, None, :, 3].expand(c.F, c.H, c.W, 3))          # a static sensor: the pose's translation, bit for bit
    else:
        assert dt.shape == (c.F, 6) and dt.dtype == torch.float32 and bt <= 0.0


def test_an_unbatched_pose_and_one_output_alone():
    c = sc.case(5, 37, 3, "table", "waymo_yaw", "above", "explicit")
    o, d, dp, dt = run(c)
    pose = c.pose[1].to(DEV).requires_grad_(True)
    twist = c.twist[1].to(DEV).requires_grad_(True)
    o1, d1 = sw.sweep_rays(pose, twist, **c.kw)
    assert o1.shape == d1.shape == (c.H, c.W, 3) and torch.equal(bits(o1), bits(o[1])) and torch.equal(bits(d1), bits(d[1]))
    (d1 * c.g_d[1].to(DEV)).sum().backward()                                                    # ray_o unused: its gradient is zero
    # against float64 autograd of the directions alone
    p64 = c.pose[1].double().requires_grad_(True)
    x64 = c.twist[1].double().requires_grad_(True)
    _, dd = sw.sweep_rays_reference(p64, x64, **c.kw)
    (dd * c.g_d[1].double()).sum().backward()
    A = sw.sweep_rays_reference(c.pose[1], c.twist[1], **c.kw, per_ray=True, g_o=torch.zeros_like(c.g_o[1]), g_d=c.g_d[1])[2].abs().sum((0, 1))
    assert sc.backward_excess(pose.grad.reshape(12), p64.grad.reshape(12), A[:12]) <= 0.0
    assert sc.backward_excess(twist.grad, x64.grad, A[12:]) <= 0.0
    # a 4 x 4 pose reads as its first three rows
    P4 = torch.eye(4, device=DEV)
    P4[:3] = c.pose[1].to(DEV)
    o4, d4 = sw.sweep_rays(P4, c.twist[1].to(DEV), **c.kw)
    assert torch.equal(bits(o4), bits(o1)) and torch.equal(bits(d4), bits(d1))


# ---- 8. reproducibility, host waits ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [sc.case(66, 1030, 3, "table", "waymo_yaw", "wide", "explicit"), sc.case(3, 70, 3, "bounds", "kitti", "above", "default"),
                               sc.case(5, 37, 3, "table", "kitti", "none", "default")], ids=lambda c: c.key)
def test_equal_bits_frames_one_by_one_a_dirty_workspace_and_unchanged_inputs(c):
    pose0, twist0 = c.pose.clone(), None if c.twist is None else c.twist.clone()
    a = run(c)
    b = run(c)
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(bits(x), bits(y))
    for f in range(c.F):                                                                        # F frames in one call equal the frames one by one
        one = run(c, frames=slice(f, f + 1))
        for x, y in zip(a, one):
            assert (x is None and y is None) or torch.equal(bits(x[f:f + 1]), bits(y))
    n = sw.work_bytes(c.F, c.H, c.W)
    for fill in (0xFF, 0x7F, 0x00):                                                             # NaNs, huge numbers, zeros in the tables and the partial sums
        ws = torch.full((n + 256,), fill, dtype=torch.uint8, device=DEV)
        ws = ws[(-ws.data_ptr()) % 256:][:n]
        w = run(c, workspace=ws)
        for x, y in zip(a, w):
            assert (x is None and y is None) or torch.equal(bits(x), bits(y))
    assert torch.equal(c.pose, pose0) and (twist0 is None or torch.equal(c.twist, twist0))
    pose, twist = c.pose.to(DEV), None if c.twist is None else c.twist.to(DEV)
    inc, tau = torch.tensor(c.kw["inclination"], dtype=torch.float32, device=DEV), None if c.kw["tau"] is None else torch.tensor(c.kw["tau"], device=DEV)
    keep = [t.clone() for t in (pose, inc) + (() if twist is None else (twist,)) + (() if tau is None else (tau,))]
    o, d = sw.sweep_rays(pose, twist, **{**c.kw, "inclination": inc, "tau": tau})                  # device tensors are used as they are
    assert torch.equal(bits(o), bits(a[0])) and torch.equal(bits(d), bits(a[1]))
    for t, k in zip((pose, inc) + (() if twist is None else (twist,)) + (() if tau is None else (tau,)), keep):
        assert torch.equal(t, k)
    with pytest.raises(sw.SweepError, match="workspace"):
        sw.sweep_rays(pose, twist, **c.kw, workspace=torch.empty(n - 1, dtype=torch.uint8, device=DEV))
    with pytest.raises(sw.SweepError, match="float32"):
        sw.sweep_rays(pose.double(), None if twist is None else twist.double(), **c.kw)


def test_a_call_does_not_wait_for_the_device():
    c = sc.case(66, 1030, 3, "table", "waymo_yaw", "wide", "explicit")
    r = sc.reference(c)
    run(c)                                                                                      # warm: the loaded library, the allocators
    g_o, g_d = c.g_o.to(DEV), c.g_d.to(DEV)
    pose, twist = c.pose.to(DEV).requires_grad_(True), c.twist.to(DEV).requires_grad_(True)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        o, d = sw.sweep_rays(pose, twist, **c.kw)
        torch.autograd.backward([o, d], [g_o, g_d])
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert sc.forward_excess(d, r.d, 1.0) <= 0.0 and sc.forward_excess(o, r.o, r.scale) <= 0.0
    assert sc.backward_excess(pose.grad.reshape(c.F, 12), r.d_pose.reshape(c.F, 12), r.A[:, :12]) <= 0.0
    assert sc.backward_excess(twist.grad, r.d_twist, r.A[:, 12:]) <= 0.0


# ---- 9. the grid operators with per-column origins ---------------------------------------------------------------------------------------------------------

GRID_SIZES = [(5, 37), (16, 256)]


def _grid_case(H, W, cloud, mask, seed=0):
    """Sweep rays of a fast sensor (3 m and 0.5 rad per sweep: the origins differ by metres between columns) with ranges and masks like the
    operators' own tests: (o, d, range_a, range_b, mask_a, mask_b) float32 / bool on the device."""
    c = sc.case(H, W, 1, "bounds", "kitti", "large", "default")
    with torch.no_grad():
        o, d = sw.sweep_rays(c.pose[0].to(DEV), c.twist[0].to(DEV), **c.kw)
    assert float((o[0, 0] - o[0, -1]).norm()) > 2.0 and torch.equal(o[0], o[-1])
    rng = np.random.default_rng(seed + 1000 * H + W)
    gt = (6.0 + 30.0 * rng.uniform(size=(H, 1)) + 3.0 * np.sin(np.arange(W) / 9.0)[None, :] + rng.uniform(0, 0.5, (H, W))).astype(np.float32)
    if cloud == "coherent":
        ra, rb = (gt + rng.normal(0, 0.03, (H, W))).astype(np.float32), gt
    else:                                                                    # independent random ranges: the search degenerates towards brute force
        ra, rb = rng.uniform(1, 80, (H, W)).astype(np.float32), rng.uniform(1, 80, (H, W)).astype(np.float32)
    ma = np.ones((H, W), bool)
    mb = ma
    if mask == "drop30":
        ma = rng.uniform(size=(H, W)) >= 0.3; mb = ma
    elif mask == "two":
        ma = rng.uniform(size=(H, W)) >= 0.3; mb = rng.uniform(size=(H, W)) >= 0.4
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=DEV)
    return o.contiguous(), d.contiguous(), t(ra), t(rb), t(ma), t(mb)


def _brute(pa, pb):
    """chamfer_3DDist in its brute-force mode on two point lists: (d1, d2, i1, i2)."""
    from lidar_rt_amd.chamfer3D import chamfer_3DDist, _C
    _C.set_option("mode", 0, DEV)
    try:
        d1, d2, i1, i2 = chamfer_3DDist()(pa[None].contiguous(), pb[None].contiguous())
    finally:
        _C.set_option("mode", 2, DEV)                                        # the state is per device: back to the default (auto)
    return d1[0], d2[0], i1[0], i2[0]


@pytest.mark.parametrize("H,W", GRID_SIZES)
def test_grid_chamfer_with_sweep_rays_equals_brute_force(H, W):
    from lidar_rt_amd import grid_chamfer as gc
    for cloud in ("coherent", "incoherent"):
        for mask in ("all", "drop30", "two"):
            o, d, ra, rb, ma, mb = _grid_case(H, W, cloud, mask)
            ia, ib = torch.nonzero(ma.reshape(-1)).squeeze(1), torch.nonzero(mb.reshape(-1)).squeeze(1)
            pa = (o + d * ra[..., None]).reshape(-1, 3).index_select(0, ia)
            pb = (o + d * rb[..., None]).reshape(-1, 3).index_select(0, ib)
            d1, d2, i1, i2 = _brute(pa, pb)
            da, db, xa, xb = gc.grid_chamfer_nearest(o, d, ra, rb, ma, mb)
            tag = (H, W, cloud, mask)
            assert torch.equal(da.reshape(-1)[ia], d1) and torch.equal(db.reshape(-1)[ib], d2), tag
            assert torch.equal(xa.reshape(-1)[ia].long(), ib[i1.long()]) and torch.equal(xb.reshape(-1)[ib].long(), ia[i2.long()]), tag
            loss, m_a, m_b = gc.grid_chamfer(o, d, ra, rb, ma, mb, weight=0.3)
            w_a, w_b = float(d1.double().mean()), float(d2.double().mean())
            assert abs(float(m_a) - w_a) <= 2.0 ** -23 * w_a and abs(float(m_b) - w_b) <= 2.0 ** -23 * w_b, tag


@pytest.mark.parametrize("H,W", [(8, 37), (16, 256)])                        # the operator's 7 x 7 SSIM window must fit
def test_frame_metrics_with_sweep_rays_carry_the_brute_force_distances(H, W):
    from lidar_rt_amd import metrics as mt
    for cloud in ("coherent", "incoherent"):
        o, d, ra, rb, ma, mb = _grid_case(H, W, cloud, "two")
        rng = np.random.default_rng(H * W)
        gi = torch.as_tensor(rng.uniform(0, 1, (H, W)).astype(np.float32), device=DEV)
        pr = torch.where(mb, torch.tensor(0.1, device=DEV), torch.tensor(0.9, device=DEV))       # the predicted hits are exactly mask_b at ratio 0.4
        pa = (o + d * rb[..., None]).reshape(-1, 3)[ma.reshape(-1)]                              # ground truth: range_b under mask_a
        pb = (o + d * ra[..., None]).reshape(-1, 3)[mb.reshape(-1)]                              # prediction: range_a under mask_b
        d1, d2, _, _ = _brute(pa, pb)
        row = mt.frame_metrics((ra, gi, pr), rb, gi, ma, (o, d), raydrop_ratio=0.4).tolist()
        want = float(d1.double().mean() + d2.double().mean())
        assert abs(row[13] - want) <= 2.0 ** -23 * want, (H, W, cloud, row[13], want)
        thr = torch.tensor(0.05, dtype=torch.float32, device=DEV)
        p1, p2 = float((d1 < thr).double().mean()), float((d2 < thr).double().mean())
        f = 2 * p1 * p2 / (p1 + p2) if p1 + p2 > 0 else 0.0
        assert abs(row[14] - f) <= 2.0 ** -23 * max(f, 1e-30) and row[15] == pb.shape[0] and row[16] == pa.shape[0]
        twin = mt.frame_metrics_reference((ra, gi, pr), rb, gi, ma, (o, d), raydrop_ratio=0.4).tolist()
        assert abs(twin[13] - want) <= 1e-9 * want


@pytest.mark.parametrize("H,W", GRID_SIZES)
def test_scene_init_neighbour_lists_with_sweep_rays_equal_brute_force(H, W):
    from lidar_rt_amd import scene_init as si
    for cloud in ("coherent", "incoherent"):
        for mask in ("all", "drop30"):
            o, d, r, _, m, _ = _grid_case(H, W, cloud, mask)
            pts = o + d * r[..., None]
            want8 = si.neighbours_reference(pts, m, 8, pairs=1 << 25).reshape(-1, 8)
            for k in (6, 4):
                nbr = si.estimate_normals(o, d, r, m, k)[1].reshape(-1, 8)
                want = want8.clone(); want[:, k:] = -1
                assert torch.equal(nbr, want), (H, W, cloud, mask, k, int((nbr != want).any(1).sum()))


# ---- 10. the loop ------------------------------------------------------------------------------------------------------------------------------------------

def test_train_and_evaluate_on_a_sequence_of_a_moving_sensor(tmp_path):
    import json
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import make_sequence
    from lidar_rt_amd import sequence
    data = str(tmp_path / "seq")
    meta = make_sequence.make("kitti360_dynamic", data, n_frames=4, scale=0.01, sweep_speed=1.5, hw=(16, 256))
    assert (meta["height"], meta["width"]) == (16, 256)
    z = np.load(os.path.join(data, "frames", "000002.npz"))
    assert z["twist"].shape == (6,) and z["twist"][0] == np.float32(1.5) and "tau" not in z.files
    seq = sequence.load_sequence(data, DEV, sweep="stored")
    o, d = seq.frames.get_range_rays(2)
    assert 1.3 < float((o[0, 0] - o[0, -1]).norm()) < 1.6 and sorted(seq.frames.sweep_meta) == [0, 1, 2, 3]
    out = str(tmp_path / "out")
    a = subprocess.run([sys.executable, "-m", "lidar_rt_amd.train", "--data", data, "--out", out, "--iters", "3", "--log-every", "1", "--save-every", "3",
                        "--max-points", "4000", "--sweep", "stored", "--refine-poses", "--refine-twist"], cwd=REPO, capture_output=True, text=True, timeout=600)
    assert a.returncode == 0, a.stdout[-2000:] + a.stderr[-3000:]
    rows = [json.loads(l) for l in a.stdout.splitlines() if l.startswith("{") and "iteration" in l]
    assert [r["iteration"] for r in rows] == [1, 2, 3] and all(np.isfinite(r["loss"]) for r in rows), rows
    assert os.path.exists(os.path.join(out, "chkpnt3.pth"))
    p3 = torch.load(os.path.join(out, "poses3.pth"), map_location="cpu", weights_only=False)
    seen = sorted({r["frame"] for r in rows})
    for f in seen:                                                           # Adam moves a parameter exactly when its gradient is not zero
        assert bool(torch.isfinite(p3["xi"][f]).all()) and float(p3["xi"][f].abs().max()) > 0.0, (f, p3["xi"][f])
        moved = (p3["twist"][f] - torch.as_tensor(z["twist"])).abs()
        assert bool(torch.isfinite(p3["twist"][f]).all()) and float(moved.max()) > 0.0, (f, p3["twist"][f])
    for f in set(p3["xi"]) - set(seen):                                      # a frame no iteration drew keeps what it had
        assert not p3["xi"][f].any() and torch.equal(p3["twist"][f], torch.as_tensor(z["twist"]))
    assert p3["refine_twist"] is True
    e = subprocess.run([sys.executable, "-m", "lidar_rt_amd.evaluate", "--data", data, "--ckpt", os.path.join(out, "chkpnt3.pth"), "--frames", "train", "--sweep", "stored"],
                       cwd=REPO, capture_output=True, text=True, timeout=600)
    assert e.returncode == 0, e.stdout[-2000:] + e.stderr[-3000:]
    res = json.loads([l for l in e.stdout.splitlines() if l.startswith("{")][-1])
    assert res["iteration"] == 3 and res["frames"] == [0, 1, 2, 3] and np.isfinite(res["mean"]["depth"]["rmse"])
