"""Beam rays without a GPU: the twin against the sweep rays' twin, its geometry, gradcheck, two closed forms of the table gradient, the rule's
header compiled for the host against the twin, the fourteenth product library (`liblrt_beams.so`), BeamCalibration and its files, SensorPoses
with and without a table, and what the Python side and the command lines refuse."""
import ctypes as C
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

from lidar_rt_amd import beams as bm, build as lrt_build, poses, resources, sweep as sw
from lidar_rt_amd.training import RangeFrames
from tests import beam_cases as bc, sweep_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


# ---- 1. a zero table is the sweep rays ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [c for c in bc.all_cases() if c.table_kind == "zero"], ids=lambda c: c.key)
def test_the_twin_with_a_zero_table_is_the_sweep_twin(c):
    o, d = bm.beam_rays_reference(c.pose, c.twist, beams=c.beams, **c.kw)
    wo, wd = sw.sweep_rays_reference(c.pose, c.twist, **c.kw)
    assert o.dtype == d.dtype == torch.float64 and torch.equal(o, wo) and torch.equal(d, wd)
    no, nd = bm.beam_rays(c.pose, c.twist, beams=None, **c.kw)                                   # beams=None is sweep_rays
    so, sd = sw.sweep_rays(c.pose, c.twist, **c.kw)
    assert no.dtype == torch.float32 and torch.equal(no, so) and torch.equal(nd, sd)
    co, cd = bm.beam_rays(c.pose, c.twist, beams=c.beams, **c.kw)                                # a CPU tensor: the twin rounded to float32
    assert torch.equal(co, o.float()) and torch.equal(cd, d.float())


# ---- 2. geometry ----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,inc,data_type", [(5, 37, "bounds", "KITTI"), (16, 64, "table", "Waymo"), (1, 1, "bounds", "KITTI")])
def test_elevation_and_azimuth_are_the_nominal_ones_plus_the_offsets(H, W, inc, data_type):
    rng = np.random.default_rng(H * W)
    incl = list(sc.KITTI_INC) if inc == "bounds" else np.sort(rng.uniform(-0.31, 0.04, size=H)).astype(np.float32).tolist()
    tab = torch.tensor(rng.uniform(-0.3, 0.3, size=(H, 2)))
    P = torch.eye(4, dtype=torch.float64)[:3]
    o, d = bm.beam_rays_reference(P, None, H, W, incl, tab, data_type)
    off, yaw = sw.convention(data_type, None)
    el, az = bm._angles(H, W, torch.tensor(incl, dtype=torch.float32), off, yaw, torch.device("cpu"))
    if inc == "table":
        assert torch.equal(el, torch.tensor(incl, dtype=torch.float32).double().flip(0))         # the inclination table is flipped, the beam table is not
    assert float((torch.asin(d[..., 2]) - (el + tab[:, 0])[:, None]).abs().max()) <= 1e-12
    diff = torch.atan2(d[..., 1], d[..., 0]) - (az[None, :] + tab[:, 1:2])
    diff = torch.remainder(diff + math.pi, 2 * math.pi) - math.pi
    assert float(diff.abs().max()) <= 1e-12
    assert not o.any()


# ---- 3. gradcheck -----------------------------------------------------------------------------------------------------------------------------------------------

def test_gradcheck_of_the_twin_in_pose_twist_and_beams():
    c = bc.case(3, 7, 2, "table", "large", "large")
    pose, twist, tab = c.pose.double().requires_grad_(True), c.twist.double().requires_grad_(True), c.beams.double().requires_grad_(True)
    fn = lambda P, x, b: bm.beam_rays_reference(P, x, beams=b, **c.kw)
    assert torch.autograd.gradcheck(fn, (pose, twist, tab), eps=1e-6, atol=1e-7, rtol=1e-6)
    c0 = bc.case(3, 7, 2, "bounds", "none", "small")
    fn0 = lambda P, b: bm.beam_rays_reference(P, None, beams=b, **c0.kw)
    assert torch.autograd.gradcheck(fn0, (c0.pose.double().requires_grad_(True), c0.beams.double().requires_grad_(True)), eps=1e-6, atol=1e-7, rtol=1e-6)


# ---- 4. closed forms ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("twist", ["none", "large"])
def test_closed_forms_of_the_table_gradient(twist):
    """Against target rays of a table T*, loss sum |d - d*|^2.  Both rays of a pixel are the same rotation of two local unit vectors, so the
    rotations cancel.  Elevations apart by D: d/d eps |l(e) - l(e*)|^2 = -2 l* . dl/de = 2 sin(D), F W times per row.  Azimuths apart by D:
    -2 l* . dl/da = 2 cos^2(e) sin(D)."""
    F, H, W = 3, 5, 37
    c = bc.case(H, W, F, "table", twist, "small")
    rng = np.random.default_rng(5)
    D = torch.tensor(rng.uniform(0.5e-3, 1.5e-3, size=H) * rng.choice([-1.0, 1.0], size=H))
    base = c.beams.double()
    pose, xi = c.pose.double(), None if c.twist is None else c.twist.double()
    for f in range(F):                                                                          # rotations to float64: a pose rounded to float32 is orthogonal to 6e-8 only
        pose[f, :, :3] = torch.from_numpy(sc._rot([0.3 + f, -0.7, 0.2 * f + 0.1]))
    off, yaw = sw.convention(c.kw["data_type"], c.kw["sensor2ego"])
    el, _ = bm._angles(H, W, torch.tensor(c.kw["inclination"], dtype=torch.float32), off, yaw, torch.device("cpu"))
    for col, want in ((0, 2 * F * W * torch.sin(D)), (1, 2 * F * W * torch.cos(el + base[:, 0]) ** 2 * torch.sin(D))):
        star = base.clone()
        star[:, col] -= D                                                                       # T = T* + D in that column
        _, d_star = bm.beam_rays_reference(pose, xi, beams=star, **c.kw)
        tab = base.clone().requires_grad_(True)
        _, d = bm.beam_rays_reference(pose, xi, beams=tab, **c.kw)
        ((d - d_star.detach()) ** 2).sum().backward()
        assert float(((tab.grad[:, col] - want).abs() / want.abs()).max()) <= 1e-9, (col, tab.grad[:, col], want)


# ---- 5. per-ray contributions -------------------------------------------------------------------------------------------------------------------------------------

def test_the_per_ray_contributions_add_up_to_the_gradient():
    for c in (bc.case(5, 37, 3, "table", "large", "large"), bc.case(3, 70, 1, "bounds", "none", "one_row")):
        r = bc.reference(c)
        assert float((r.total_beams - r.d_beams).abs().max()) <= 1e-12 * float(r.A_beams.max())
        want = torch.cat([r.d_pose.reshape(c.F, 12), torch.zeros(c.F, 6, dtype=torch.float64) if r.d_twist is None else r.d_twist], 1)
        assert float((r.total - want).abs().max()) <= 1e-12 * float(r.A.max())
        assert bool((r.A_beams >= r.total_beams.abs() * (1 - 1e-12)).all())


# ---- 6. the rule's header on the host ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("beams_check") / "beams_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "host_check", "beams_check.cpp")])
    return exe


def run_host(exe, c, tmp_path):
    kw = c.kw
    inc = np.asarray(kw["inclination"], np.float64).astype(np.float32)
    tau = (sw.column_times(c.W).numpy() if kw["tau"] is None else np.asarray(kw["tau"])).astype(np.float32)
    off, yaw = sw.convention(kw["data_type"], kw["sensor2ego"])
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<8i", c.F, c.H, c.W, inc.size, int(c.twist is not None), 0, 0, 0))
        f.write(struct.pack("<2d", off, yaw))
        f.write(c.pose.numpy().tobytes())
        if c.twist is not None:
            f.write(c.twist.numpy().tobytes())
        f.write(inc.tobytes()); f.write(tau.tobytes()); f.write(c.beams.numpy().tobytes()); f.write(c.g_o.numpy().tobytes()); f.write(c.g_d.numpy().tobytes())
    res = subprocess.run([exe, inp, out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "BEAMSCHECK ok" in res.stdout, res.stdout + res.stderr
    rest = np.frombuffer(open(out, "rb").read(), np.float32)
    n3 = c.F * c.H * c.W * 3
    t = lambda a, *shape: torch.from_numpy(a.reshape(*shape).copy())
    return (t(rest[:n3], c.F, c.H, c.W, 3), t(rest[n3:2 * n3], c.F, c.H, c.W, 3), t(rest[2 * n3:2 * n3 + 12 * c.F], c.F, 12),
            t(rest[2 * n3 + 12 * c.F:2 * n3 + 18 * c.F], c.F, 6), t(rest[2 * n3 + 18 * c.F:], c.H, 2))


def test_the_rule_header_on_the_host_against_the_twin(host_check, tmp_path):
    """Every ray within one float32 ulp and the three gradients within the backward bound, on every small case and one of several workgroups."""
    cases = bc.all_cases_small()
    assert {c.table_kind for c in cases} == set(bc.TABLES) and {c.twist_kind for c in cases} == set(bc.TWISTS)
    for c in cases:
        o, d, dp, dt, db = run_host(host_check, c, tmp_path)
        r = bc.reference(c)
        assert sc.forward_excess(d, r.d, 1.0) <= 0.0 and sc.forward_excess(o, r.o, r.scale) <= 0.0, c.key
        assert sc.backward_excess(dp, r.d_pose.reshape(c.F, 12), r.A[:, :12]) <= 0.0, c.key
        assert sc.backward_excess(db, r.d_beams, r.A_beams) <= 0.0, c.key
        if c.twist is not None:
            assert sc.backward_excess(dt, r.d_twist, r.A[:, 12:]) <= 0.0, c.key
        else:
            assert not dt.any()
        if c.table_kind == "zero":                                                               # the host text of the two headers agrees bit for bit too
            so, sd = sw.sweep_rays_reference(c.pose, c.twist, **c.kw)
            assert sc.forward_excess(d, sd, 1.0) <= 0.0


# ---- the library -------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def beams_lib():
    return lrt_build.build_beams()


def test_the_library_has_a_source_list_of_its_own_and_leaves_the_sweep_header_alone():
    assert lrt_build.BEAMS_SOURCES == ["lrt_beams.hip"] and {"lrt_beams_math.h", "lrt_sweep_math.h", "lrt_device_guard.h"} <= set(lrt_build.BEAMS_HEADERS)
    others = lrt_build.SOURCES + lrt_build.HEADERS + lrt_build.SWEEP_SOURCES + lrt_build.SWEEP_HEADERS + lrt_build.SWEEPPROJ_HEADERS + lrt_build.ACTORSWEEP_HEADERS
    assert not any("lrt_beams" in f for f in others)
    assert os.path.basename(lrt_build.BEAMS_LIB) == "liblrt_beams.so" and os.path.basename(lrt_build.BEAMS_STAMP) == "liblrt_beams.srchash"
    src = open(lrt_build.__file__).read()
    assert "build_beams(force, verbose)" in src[src.index("def _build_product"):src.index("def _build_lib")]
    assert "csrc/liblrt_beams.so" in open(os.path.join(REPO, "setup.py")).read()
    body = src[src.index("def build_beams"):src.index("EXT_SRC =")]
    assert "CODEGEN_FLAGS" in body and "resources.check(BEAMS_LIB)" in body
    mh = open(os.path.join(REPO, "lidar_rt_amd", "csrc", "lrt_beams_math.h")).read()
    assert '#include "lrt_sweep_math.h"' in mh
    assert not re.search(r"\bfloat\b(?!\s*\*)", re.sub(r"//.*", "", mh).replace("const float*", ""))        # float64 throughout


def test_the_library_builds_and_exports_what_its_header_declares(beams_lib):
    assert os.path.exists(beams_lib) and not lrt_build.beams_is_stale()
    hdr = open(os.path.join(REPO, "include", "lrt_beams.h")).read()
    declared = set(re.findall(r"\b(lrt_beams_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(bm.EXPORTS), declared ^ set(bm.EXPORTS)
    lib = bm.load()
    exported = set(re.findall(r"\blrt_beams_[a-z_]+\b", subprocess.run(["nm", "-D", "--defined-only", beams_lib], capture_output=True, text=True, check=True).stdout))
    assert exported == declared, exported ^ declared
    assert lib.lrt_beams_abi_version() == int(re.search(r"#define\s+LRT_BEAMS_ABI_VERSION\s+(\d+)", hdr).group(1)) == bm.ABI_VERSION


def test_the_kernels_pass_the_resource_gate(beams_lib):
    res = resources.kernel_resources(beams_lib)
    own = sorted(n for n in res if resources.is_own_kernel(n))
    assert own == ["k_beams_bwd_cols", "k_beams_bwd_finish", "k_beams_rays", "k_beams_tables"], own       # two launches forward, two backward
    assert all(any(re.search(g_, n) for g_ in resources.GATED) for n in own)
    assert resources.violations(res) == []
    for n in own:
        r = res[n]
        assert r["vgpr_spill"] == 0 and r["scratch_bytes"] == 0 and not r["dynamic_stack"], (n, r)
    resources.check(beams_lib)


def test_argument_errors_come_before_the_device_and_launch_nothing(beams_lib):
    lib = bm.load()
    buf = (C.c_char * 8192)()
    p = (C.addressof(buf) + 255) // 256 * 256
    err = lambda: lib.lrt_beams_last_error()
    nodev = 1 << 20                                                                     # a device that does not exist: what passes the checks ends there
    wb = lib.lrt_beams_work_bytes
    assert wb(0, 8, 64) < 0 and wb(1, 0, 64) < 0 and wb(1, 8, 0) < 0 and wb(3, 30000, 30000) < 0 and wb(1 << 40, 1, 1) < 0
    assert wb(3, 5, 37) == (8 * (12 * 3 * 37 + 4 * 5 + 18 * 3 * 1 + 2 * 3 * 1 * 5) + 255) // 256 * 256
    assert wb(1, 64, 2048) == (8 * (12 * 2048 + 4 * 64 + 18 * 32 + 2 * 32 * 64) + 255) // 256 * 256
    need = wb(1, 8, 64)

    def fwd(F=1, H=8, W=64, pose=p, twist=p, inc=p, n_inc=2, off=0.0, yaw=0.0, tau=p, beams=p, outs=(p, p), ws=p, ws_bytes=need):
        return lib.lrt_beams_rays(nodev, F, H, W, pose, twist, inc, n_inc, off, yaw, tau, beams, *outs, ws, ws_bytes, None)

    def bwd(F=1, H=8, W=64, pose=p, twist=p, inc=p, n_inc=2, off=0.0, yaw=0.0, tau=p, beams=p, gs=(p, p), d_pose=p, d_twist=p, d_beams=p, ws=p, ws_bytes=need):
        return lib.lrt_beams_backward(nodev, F, H, W, pose, twist, inc, n_inc, off, yaw, tau, beams, *gs, d_pose, d_twist, d_beams, ws, ws_bytes, None)
    for call in (fwd, bwd):
        assert call(F=0) < 0 and b"0 frames of 8 x 64" in err()
        assert call(n_inc=3) < 0 and b"3 inclinations" in err()
        assert call(off=1.0) < 0 and b"pixel offset" in err()
        assert call(yaw=float("nan")) < 0 and b"yaw" in err()
        assert call(pose=None) < 0 and b"null pose / inclination" in err()
        assert call(beams=None) < 0 and b"null beams pointer" in err()
        assert call(tau=None) < 0 and b"null tau" in err()
        assert call(ws=p + 8) < 0 and b"256-byte aligned" in err()
        assert call(ws_bytes=need - 1) < 0 and (b"a workspace of %d bytes, 1 frames of 8 x 64 need %d" % (need - 1, need)) in err()
        assert call() < 0 and b"no HIP device" in err()
        assert call(twist=None, tau=None) < 0 and b"no HIP device" in err()
    assert fwd(outs=(None, p)) < 0 and b"null ray_o / ray_d" in err()
    assert bwd(gs=(None, p)) < 0 and b"null g_o / g_d" in err()
    assert bwd(d_pose=None, d_twist=None, d_beams=None) < 0 and b"neither d_pose nor d_beams" in err()
    assert bwd(d_twist=None) < 0 and b"without a d_twist" in err()
    assert bwd(d_pose=None) < 0 and b"d_twist goes with d_pose" in err()
    assert bwd(d_pose=None, d_twist=None) < 0 and b"no HIP device" in err()                 # the table alone
    assert bwd(d_beams=None) < 0 and b"no HIP device" in err()                               # the pose alone
    assert bwd(F=70000, H=1, W=1, ws_bytes=1 << 30) < 0 and b"70000 frames" in err()


# ---- 7. BeamCalibration -----------------------------------------------------------------------------------------------------------------------------------------

def _one_step(cal, seed=0):
    g = torch.Generator().manual_seed(seed)
    cal.zero_grad()
    (cal.table * torch.randn(cal.H, 2, generator=g)).sum().backward()
    cal.step()


def test_beam_calibration_state_gauge_and_files(tmp_path):
    H = 6
    init = torch.tensor(np.random.default_rng(1).normal(0, 1e-3, (H, 2)), dtype=torch.float32)
    a = bm.BeamCalibration(H, init=init, lr=1e-3)
    assert torch.equal(a.table.detach(), init) and not bm.BeamCalibration(H).table.any()
    g = a.optimizer.param_groups[0]
    assert g["betas"] == (0.9, 0.999) and g["eps"] == 1e-15 and g["lr"] == 1e-3
    _one_step(a)
    assert float((a.table.detach() - init).abs().max()) > 0
    # the state dict round trip: table, moments, and the next step equal bit for bit
    b = bm.BeamCalibration(H, lr=5.0)
    b.load_state_dict(a.state_dict())
    assert torch.equal(b.table.detach(), a.table.detach()) and b.lr == 1e-3
    _one_step(a, 1); _one_step(b, 1)
    assert torch.equal(b.table.detach(), a.table.detach())
    # the gauge: the mean of the azimuth column is removed after the step, the elevation column is the plain step's
    plain, gauged = bm.BeamCalibration(H, init=init, lr=1e-3), bm.BeamCalibration(H, init=init, lr=1e-3, zero_mean_azimuth=True)
    _one_step(plain, 2); _one_step(gauged, 2)
    col = plain.table.detach()[:, 1].double()
    assert torch.equal(gauged.table.detach()[:, 1], (col - col.mean()).float()) and torch.equal(gauged.table.detach()[:, 0], plain.table.detach()[:, 0])
    assert abs(float(gauged.table.detach()[:, 1].double().mean())) <= 2.0 ** -24 * float(col.abs().max())       # exact up to the float32 store
    assert abs(float(col.mean())) > 1e-5                                                                     # and there was a mean to remove
    # the files: a .pth holds the table and the optimizer state, a text table one `eps delta` pair per row; both load to the same tensor
    pth, txt = str(tmp_path / "beams7.pth"), str(tmp_path / "beams.txt")
    a.save(pth)
    assert set(torch.load(pth, weights_only=False)) == {"beams", "optimizer", "lr", "zero_mean_azimuth"}
    np.savetxt(txt, a.table.detach().numpy().astype(np.float64), fmt="%.9e")
    assert torch.equal(bm.load_table(pth), a.table.detach()) and torch.equal(bm.load_table(txt, H), a.table.detach())
    c = bm.BeamCalibration(H)
    c.load(pth)
    assert torch.equal(c.table.detach(), a.table.detach())
    with pytest.raises(bm.BeamError, match="the images have 7 rows"):
        bm.load_table(txt, 7)
    with pytest.raises(bm.BeamError, match="neither"):
        bm.load_table(str(tmp_path / "missing.txt"))


# ---- 8. SensorPoses -----------------------------------------------------------------------------------------------------------------------------------------------

def _frames(H=5, W=37, sweep=True):
    rf = RangeFrames()
    for f in range(2):
        P = torch.eye(4)
        P[:3, :3] = torch.from_numpy(sc._rot([0.2 * (f + 1), -0.1, 0.6])).float()
        P[:3, 3] = torch.tensor([8.0 + f, -3.0, 1.5])
        kw = dict(twist=torch.tensor([1.5, 0.2, -0.1, 0.01, -0.02, 0.3 + 0.1 * f])) if sweep and f == 1 else {}
        rf.add_range_image(f, torch.ones(H, W), torch.ones(H, W), torch.ones(H, W, dtype=torch.bool), sc.KITTI_INC, P, **kw)
    return rf, H, W


def test_sensor_poses_without_a_table_gives_the_rays_it_gave_before():
    rf, H, W = _frames()
    sp = poses.SensorPoses(rf, [0, 1], beams=None)
    assert sp.beams is None and not sp.fixed_poses and sorted(sp.xi) == [0, 1] and len(sp.optimizer.param_groups) == 1
    for f in (0, 1):
        o, d = sp.get_range_rays(f)
        assert torch.equal(o.detach(), rf.rays[f][0]) and torch.equal(d.detach(), rf.rays[f][1])
    inc, s2w, data_type, s2e = rf.pose_meta[0]
    wo, wd = rf.range_rays(H, W, inc, s2w.float() @ poses.se3_exp(sp.xi[0]), data_type, s2e)        # the static frame: the torch expression, as before
    o, d = sp.get_range_rays(0)
    assert torch.equal(o, wo) and torch.equal(d, wd)
    assert set(sp.state_dict()) == {"xi", "optimizer", "lr_trans", "lr_rot", "twist", "refine_twist", "lr_twist_trans", "lr_twist_rot"}


def test_sensor_poses_with_a_table_learns_it_alone_or_beside_the_poses():
    rf, H, W = _frames()
    cal = bm.BeamCalibration(H, lr=1e-3)
    sp = poses.SensorPoses(rf, [0, 1], beams=cal, fixed_poses=True)
    assert sp.xi == {} and sp.optimizer is None
    for f in (0, 1):                                                                            # a zero table: the rays of the frames, to float32 rounding
        o, d = sp.get_range_rays(f)
        assert o.shape == d.shape == (H, W, 3) and float((d.detach() - rf.rays[f][1]).abs().max()) <= 2e-6 and float((o.detach() - rf.rays[f][0]).abs().max()) <= 1e-6
    sp.zero_grad()
    o, d = sp.get_range_rays(1)
    g = torch.tensor(np.random.default_rng(0).normal(size=(H, W, 3)), dtype=torch.float32)
    (d * g).sum().backward()
    tab64 = cal.table.detach().double().requires_grad_(True)
    _, d64 = bm.beam_rays_reference(rf.pose_meta[1][1].double(), rf.sweep_meta[1][0].double(), H, W, list(sc.KITTI_INC), tab64, tau=rf.sweep_meta[1][1])
    (d64 * g.double()).sum().backward()
    assert float((cal.table.grad.double() - tab64.grad).abs().max()) <= 1e-5 * float(tab64.grad.abs().max())
    sp.step()
    assert float(cal.table.detach().abs().max()) > 0 and sp.state_dict()["optimizer"] is None
    # beside the poses: both get gradients from one backward; a fixed tensor is read detached
    both = poses.SensorPoses(rf, [0, 1], beams=cal)
    both.zero_grad()
    (both.get_range_rays(0)[1] * g).sum().backward()
    assert both.xi[0].grad is not None and cal.table.grad is not None and both.xi[1].grad is None
    fixed = poses.SensorPoses(rf, [0, 1], beams=cal.table.detach().clone().requires_grad_(True))
    (fixed.get_range_rays(0)[1] * g).sum().backward()
    assert fixed.beams.grad is None and fixed.xi[0].grad is not None
    # apply_table writes the rays of a fixed table into the frames
    t = torch.tensor(np.random.default_rng(3).normal(0, 2e-3, (H, 2)), dtype=torch.float32)
    before = rf.rays[1][1].clone()
    bm.apply_table(rf, t)
    wo, wd = bm.beam_rays(rf.pose_meta[1][1].float(), rf.sweep_meta[1][0], H, W, list(sc.KITTI_INC), t, tau=rf.sweep_meta[1][1])
    assert torch.equal(rf.rays[1][1], wd) and torch.equal(rf.rays[1][0], wo) and float((rf.rays[1][1] - before).abs().max()) > 1e-4


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_a_wrong_table_is_refused_before_anything_runs(capsys):
    P, x = torch.zeros(3, 4), torch.zeros(6)
    ok = dict(H=8, W=64, inclination=list(sc.KITTI_INC))
    for fn in (bm.beam_rays, bm.beam_rays_reference):
        with pytest.raises(bm.BeamError, match=r"beams must be an \(8, 2\) tensor"):
            fn(P, x, beams=torch.zeros(7, 2), **ok)
        with pytest.raises(bm.BeamError, match=r"beams must be an \(8, 2\) tensor"):
            fn(P, x, beams=torch.zeros(8), **ok)
        with pytest.raises(bm.BeamError, match=r"beams must be an \(8, 2\) tensor"):
            fn(P, x, beams=[[0.0, 0.0]] * 8, **ok)
        with pytest.raises(bm.BeamError, match="differ"):
            fn(P, x, beams=torch.zeros(8, 2, dtype=torch.float64), **ok)
        with pytest.raises(bm.BeamError, match="differ"):
            fn(P, x, beams=torch.zeros(8, 2, device="meta"), **ok)
        with pytest.raises(sw.SweepError, match="twist must be"):                                # the checks of sweep_rays come with it
            fn(P, torch.zeros(1, 6), beams=torch.zeros(8, 2), **ok)
    rf, H, W = _frames()
    with pytest.raises(bm.BeamError, match=r"SensorPoses: beams must be"):
        poses.SensorPoses(rf, [0, 1], beams=torch.zeros(H + 1, 2))
    with pytest.raises(bm.BeamError, match=r"SensorPoses: beams must be"):
        poses.SensorPoses(rf, [0, 1], beams=torch.zeros(H, 2, dtype=torch.float64))
    with pytest.raises(bm.BeamError, match="init must be"):
        bm.BeamCalibration(H, init=torch.zeros(H, 3))
    from lidar_rt_amd import train
    for argv in (["--refine-beams", "--gpus", "2"], ["--beams", "table.txt", "--gpus", "2"], ["--refine-beams", "--refine-poses", "--gpus", "2"]):
        with pytest.raises(SystemExit) as e:
            train.main(["--data", "unused"] + argv)
        assert e.value.code == 2 and "--gpus > 1" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        train.main(["--data", "unused", "--refine-beams", "--beam-lr", "0"])
    assert e.value.code == 2 and "--beam-lr must be positive" in capsys.readouterr().err
