"""Beam rays on the GPU: forward and backward of `liblrt_beams.so` against the float64 twin on every case of tests/beam_cases.py, the bits of the
sweep rays under a zero table, equal bits for equal inputs, frames in one call against frames one by one, a dirty workspace, unchanged inputs,
each gradient alone, no host wait inside a call, the ABI, and the training / evaluation / simulation loop on a sequence with a beam error."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lidar_rt_amd import beams as bm, sweep as sw
from tests import beam_cases as bc, sweep_cases as sc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def bits(t):
    return t.contiguous().view(torch.int32)


def same(x, y):
    return (x is None and y is None) or torch.equal(bits(x), bits(y))


def run(c, workspace=None, frames=None, want=("pose", "beams"), beams=None):
    """Forward and backward of the operator on a case (or on some of its frames): (o, d, d_pose, d_twist, d_beams) on the device."""
    sel = slice(None) if frames is None else frames
    pose = c.pose[sel].to(DEV).requires_grad_("pose" in want)
    twist = None if c.twist is None else c.twist[sel].to(DEV).requires_grad_("pose" in want)
    tab = (c.beams if beams is None else beams).to(DEV).requires_grad_("beams" in want)
    o, d = bm.beam_rays(pose, twist, beams=tab, **c.kw, workspace=workspace)
    torch.autograd.backward([o, d], [c.g_o[sel].to(DEV), c.g_d[sel].to(DEV)])
    return o.detach(), d.detach(), pose.grad, None if twist is None else twist.grad, tab.grad


def run_sweep(c):
    pose = c.pose.to(DEV).requires_grad_(True)
    twist = None if c.twist is None else c.twist.to(DEV).requires_grad_(True)
    o, d = sw.sweep_rays(pose, twist, **c.kw)
    torch.autograd.backward([o, d], [c.g_o.to(DEV), c.g_d.to(DEV)])
    return o.detach(), d.detach(), pose.grad, None if twist is None else twist.grad


# ---- 1. forward and backward against the twin ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", bc.all_cases(), ids=lambda c: c.key)
def test_forward_and_backward_against_the_twin(c):
    r = bc.reference(c)
    o, d, dp, dt, db = run(c)
    assert o.shape == d.shape == (c.F, c.H, c.W, 3) and o.dtype == d.dtype == torch.float32 and o.is_contiguous() and d.is_contiguous()
    fd, fo = sc.forward_excess(d, r.d, 1.0), sc.forward_excess(o, r.o, r.scale)
    bp = sc.backward_excess(dp.reshape(c.F, 12), r.d_pose.reshape(c.F, 12), r.A[:, :12])
    bt = None if dt is None else sc.backward_excess(dt, r.d_twist, r.A[:, 12:])
    bb = sc.backward_excess(db, r.d_beams, r.A_beams)
    print(f"{c.key}: excess over the bounds: directions {fd:.3e}, origins {fo:.3e}, d_pose {bp:.3e}, d_twist {bt if bt is None else format(bt, '.3e')}, d_beams {bb:.3e}")
    assert fd <= 0.0 and fo <= 0.0
    assert dp.shape == (c.F, 3, 4) and dp.dtype == torch.float32 and bp <= 0.0
    assert db.shape == (c.H, 2) and db.dtype == torch.float32 and bb <= 0.0
    if c.twist is None:
        assert dt is None
    else:
        assert dt.shape == (c.F, 6) and dt.dtype == torch.float32 and bt <= 0.0


# ---- 2. the bits of the sweep rays ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [c for c in bc.all_cases() if c.table_kind in ("zero", "one_row")], ids=lambda c: c.key)
def test_rows_without_offsets_carry_the_bits_of_the_sweep_rays(c):
    o, d, dp, dt, db = run(c)
    so, sd, sdp, sdt = run_sweep(c)
    assert torch.equal(bits(o), bits(so))                                                       # the origins never depend on the table
    if c.table_kind == "zero":
        assert torch.equal(bits(d), bits(sd)) and torch.equal(bits(dp), bits(sdp)) and same(dt, sdt)
    else:
        plain = ~c.beams.to(DEV).bool().any(1)
        assert int(plain.sum()) == c.H - 1 and torch.equal(bits(d[:, plain]), bits(sd[:, plain]))
        if c.H > 1:
            assert not torch.equal(bits(d[:, ~plain]), bits(sd[:, ~plain]))


# ---- 3. reproducibility ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [bc.case(64, 256, 3, "table", "large", "large"), bc.case(3, 70, 3, "bounds", "zero", "small"), bc.case(5, 37, 3, "table", "none", "one_row")],
                         ids=lambda c: c.key)
def test_equal_bits_frames_one_by_one_a_dirty_workspace_and_unchanged_inputs(c):
    pose0, twist0, tab0 = c.pose.clone(), None if c.twist is None else c.twist.clone(), c.beams.clone()
    a = run(c)
    b = run(c)
    assert all(same(x, y) for x, y in zip(a, b))
    r = bc.reference(c)
    per_frame = torch.zeros(c.H, 2, dtype=torch.float64)
    for f in range(c.F):                                                                        # F frames in one call equal the frames one by one
        one = run(c, frames=slice(f, f + 1))
        assert all(same(x if x is None else x[f:f + 1], y) for x, y in zip(a[:4], one[:4]))
        assert sc.backward_excess(one[4], r.beams_f[f], r.A_beams_f[f]) <= 0.0                  # a frame alone: its own part of the table's gradient
        per_frame += one[4].double().cpu()
    # The table's gradient sums over the frames, so the one-by-one results are F values rounded to float32 where the batched one is rounded once.
    # Each meets the backward bound of its frame, 2^-23 |ref_f| + 2^-34 A_f; added up that is 2^-23 sum_f |ref_f| + 2^-34 A, which backward_excess
    # states with A + 2^11 sum_f |ref_f| in the place of A.  Against the batched result the batched result's own bound comes on top.
    A_sum = r.A_beams + 2.0 ** 11 * r.beams_f.abs().sum(0)
    assert sc.backward_excess(per_frame, r.d_beams, A_sum) <= 0.0
    assert sc.backward_excess(per_frame, a[4].double().cpu(), A_sum + r.A_beams + 2.0 ** 11 * r.d_beams.abs()) <= 0.0
    n = bm.work_bytes(c.F, c.H, c.W)
    ws = torch.full((n + 256,), 0xFF, dtype=torch.uint8, device=DEV)                            # NaNs in the tables and the partial sums
    ws = ws[(-ws.data_ptr()) % 256:][:n]
    w = run(c, workspace=ws)
    assert all(same(x, y) for x, y in zip(a, w))
    assert torch.equal(c.pose, pose0) and (twist0 is None or torch.equal(c.twist, twist0)) and torch.equal(c.beams, tab0)
    pose, twist, tab = c.pose.to(DEV), None if c.twist is None else c.twist.to(DEV), c.beams.to(DEV)
    keep = [t.clone() for t in (pose, tab) + (() if twist is None else (twist,))]
    o, d = bm.beam_rays(pose, twist, beams=tab, **c.kw)
    assert torch.equal(bits(o), bits(a[0])) and torch.equal(bits(d), bits(a[1]))
    for t, k in zip((pose, tab) + (() if twist is None else (twist,)), keep):
        assert torch.equal(t, k)
    with pytest.raises(bm.BeamError, match="workspace"):
        bm.beam_rays(pose, twist, beams=tab, **c.kw, workspace=torch.empty(n - 1, dtype=torch.uint8, device=DEV))
    with pytest.raises(bm.BeamError, match="differ"):
        bm.beam_rays(pose, twist, beams=tab.cpu(), **c.kw)


# ---- 4. each gradient alone --------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [bc.case(64, 256, 3, "table", "large", "large"), bc.case(5, 37, 1, "bounds", "none", "small")], ids=lambda c: c.key)
def test_each_gradient_alone_equals_its_value_beside_the_other(c):
    o, d, dp, dt, db = run(c)
    _, _, dp1, dt1, none = run(c, want=("pose",))
    assert none is None and torch.equal(bits(dp1), bits(dp)) and same(dt1, dt)
    _, _, none_p, none_t, db1 = run(c, want=("beams",))
    assert none_p is None and none_t is None and torch.equal(bits(db1), bits(db))


# ---- 5. no host wait ---------------------------------------------------------------------------------------------------------------------------------------------

def test_a_call_does_not_wait_for_the_device():
    c = bc.case(64, 256, 3, "table", "large", "large")
    r = bc.reference(c)
    run(c)                                                                                      # warm: the loaded library, the allocators
    g_o, g_d = c.g_o.to(DEV), c.g_d.to(DEV)
    pose, twist, tab = c.pose.to(DEV).requires_grad_(True), c.twist.to(DEV).requires_grad_(True), c.beams.to(DEV).requires_grad_(True)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        o, d = bm.beam_rays(pose, twist, beams=tab, **c.kw)
        torch.autograd.backward([o, d], [g_o, g_d])
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert sc.forward_excess(d, r.d, 1.0) <= 0.0 and sc.forward_excess(o, r.o, r.scale) <= 0.0
    assert sc.backward_excess(pose.grad.reshape(c.F, 12), r.d_pose.reshape(c.F, 12), r.A[:, :12]) <= 0.0
    assert sc.backward_excess(twist.grad, r.d_twist, r.A[:, 12:]) <= 0.0 and sc.backward_excess(tab.grad, r.d_beams, r.A_beams) <= 0.0


# ---- 6. the ABI ----------------------------------------------------------------------------------------------------------------------------------------------------

def test_the_abi_refuses_with_a_message_and_launches_nothing():
    lib = bm.load()
    assert lib.lrt_beams_abi_version() == bm.ABI_VERSION == 1
    assert lib.lrt_beams_work_bytes(0, 4, 8) < 0 and lib.lrt_beams_work_bytes(1, 0, 8) < 0 and lib.lrt_beams_work_bytes(1, 4, -1) < 0
    assert lib.lrt_beams_work_bytes(3, 30000, 30000) < 0
    F, H, W = 1, 4, 8
    n = bm.work_bytes(F, H, W)
    assert n > 0 and n % 256 == 0
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)
    pose, inc, tab, ws = f32(F, 3, 4), f32(2), f32(H, 2), torch.zeros(n, dtype=torch.uint8, device=DEV)
    pose[0, :, :3] = torch.eye(3)
    o, d = torch.full((F, H, W, 3), 7.0, device=DEV), torch.full((F, H, W, 3), 7.0, device=DEV)
    g, dp, db = f32(F, H, W, 3), torch.full((F, 3, 4), 7.0, device=DEV), torch.full((H, 2), 7.0, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    fwd = lambda tab_p, nbytes: lib.lrt_beams_rays(0, F, H, W, pose.data_ptr(), None, inc.data_ptr(), 2, 0.0, 0.0, None, tab_p, o.data_ptr(), d.data_ptr(), ws.data_ptr(), nbytes, stream)
    bwd = lambda tab_p, nbytes: lib.lrt_beams_backward(0, F, H, W, pose.data_ptr(), None, inc.data_ptr(), 2, 0.0, 0.0, None, tab_p, g.data_ptr(), g.data_ptr(), dp.data_ptr(), None,
                                                       db.data_ptr(), ws.data_ptr(), nbytes, stream)
    for call in (fwd, bwd):
        assert call(tab.data_ptr(), n - 256) < 0 and b"a workspace of" in lib.lrt_beams_last_error()
        assert call(None, n) < 0 and b"null beams pointer" in lib.lrt_beams_last_error()
    torch.cuda.synchronize()
    assert bool((o == 7).all()) and bool((d == 7).all()) and bool((dp == 7).all()) and bool((db == 7).all())      # a refused call launched nothing
    assert fwd(tab.data_ptr(), n) == 0 and bwd(tab.data_ptr(), n) == 0
    torch.cuda.synchronize()
    assert not bool((d == 7).any()) and not bool(dp.any()) and not bool(db.any())                                   # every output element written


# ---- 7. the loop ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_train_resume_evaluate_and_simulate_on_a_sequence_with_a_beam_error(tmp_path):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import make_sequence
    from lidar_rt_amd import renderer, sequence
    data = str(tmp_path / "seq")
    meta = make_sequence.make("kitti360_dynamic", data, n_frames=4, scale=0.01, sweep_speed=1.5, hw=(16, 256), beam_error=2e-3)
    assert (meta["height"], meta["width"]) == (16, 256)
    true = np.load(os.path.join(data, "beams_true.npy"))
    assert true.shape == (16, 2) and true.dtype == np.float32 and 5e-4 < float(np.abs(true).std()) < 4e-3
    z = np.load(os.path.join(data, "frames", "000000.npz"))
    assert z["inclination"].shape == (2,)                                                       # the stored inclination stays nominal
    out = str(tmp_path / "out")
    common = ["--data", data, "--out", out, "--log-every", "1", "--max-points", "4000", "--sweep", "stored", "--refine-beams"]
    a = subprocess.run([sys.executable, "-m", "lidar_rt_amd.train", "--iters", "3", "--save-every", "3"] + common, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert a.returncode == 0, a.stdout[-2000:] + a.stderr[-3000:]
    rows = [json.loads(l) for l in a.stdout.splitlines() if l.startswith("{") and "iteration" in l]
    assert [r["iteration"] for r in rows] == [1, 2, 3] and all(np.isfinite(r["loss"]) for r in rows), rows
    b3 = torch.load(os.path.join(out, "beams3.pth"), map_location="cpu", weights_only=False)
    assert set(b3) == {"beams", "optimizer", "lr", "zero_mean_azimuth"} and b3["beams"].shape == (16, 2)
    assert bool(torch.isfinite(b3["beams"]).all()) and float(b3["beams"].abs().max()) > 0.0 and not os.path.exists(os.path.join(out, "poses3.pth"))
    # --resume reads the table back and says so; the first resumed iteration starts from it
    b = subprocess.run([sys.executable, "-m", "lidar_rt_amd.train", "--iters", "4", "--save-every", "1", "--resume", os.path.join(out, "chkpnt3.pth")] + common,
                       cwd=REPO, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-3000:]
    said = [json.loads(l) for l in b.stdout.splitlines() if l.startswith("{") and "beams_resumed" in l]
    assert len(said) == 1 and said[0]["beams_resumed"] == os.path.join(out, "beams3.pth")
    assert said[0]["sha256"] == hashlib.sha256(b3["beams"].numpy().tobytes()).hexdigest()
    b4 = torch.load(os.path.join(out, "beams4.pth"), map_location="cpu", weights_only=False)
    assert b4["optimizer"]["state"][0]["step"] == 4 and float((b4["beams"] - b3["beams"]).abs().max()) <= 4 * b3["lr"]       # one more Adam step of the same moments
    # evaluate and simulate render through the table
    e = subprocess.run([sys.executable, "-m", "lidar_rt_amd.evaluate", "--data", data, "--ckpt", os.path.join(out, "chkpnt3.pth"), "--frames", "train", "--sweep", "stored",
                        "--beams", os.path.join(out, "beams3.pth")], cwd=REPO, capture_output=True, text=True, timeout=600)
    assert e.returncode == 0, e.stdout[-2000:] + e.stderr[-3000:]
    res = json.loads([l for l in e.stdout.splitlines() if l.startswith("{")][-1])
    assert res["iteration"] == 3 and res["frames"] == [0, 1, 2, 3] and np.isfinite(res["mean"]["depth"]["rmse"])
    txt = str(tmp_path / "true.txt")
    np.savetxt(txt, true.astype(np.float64), fmt="%.9e")
    s = subprocess.run([sys.executable, "-m", "lidar_rt_amd.simulate", "--data", data, "--ckpt", os.path.join(out, "chkpnt3.pth"), "--out", str(tmp_path / "sim"), "--frames", "train",
                        "--max-frames", "1", "--sweep", "stored", "--beams", txt], cwd=REPO, capture_output=True, text=True, timeout=600)
    assert s.returncode == 0, s.stdout[-2000:] + s.stderr[-3000:]
    assert json.load(open(tmp_path / "sim" / "simulate.json"))["arguments"]["beams"] == txt
    # the synthetic ground truth again through the tracer: the true table explains the first frame better than the zero table
    seq = sequence.load_sequence(data, DEV, sweep="stored")
    gt, mask = seq.frames.get_depth(0), seq.frames.get_mask(0)
    l1 = {}
    for name, table in (("zero", torch.zeros(16, 2, device=DEV)), ("true", torch.as_tensor(true, device=DEV))):
        bm.apply_table(seq.frames, table, [0])
        depth = make_sequence.render_ground_truth("kitti360_dynamic", 0, seq.frames.rays[0], n_frames=4, scale=0.01, device=DEV)
        l1[name] = float(((depth - gt).abs() * mask).sum() / mask.sum())
    print(f"depth L1 of frame 0 against the ground truth: zero table {l1['zero']:.6f}, true table {l1['true']:.6f}")
    assert l1["true"] < l1["zero"]
