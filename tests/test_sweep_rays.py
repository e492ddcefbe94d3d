"""Sweep rays without a GPU: the twin in the static case and its physics, Log against Exp, the rule's header compiled for the host against the
twin, the ninth product library (`liblrt_sweep.so`: a source list and hash of its own that moves no other hash, exports, resource gate, argument
errors before the device is touched) and the plumbing (frames, pose refinement, sequences, the command lines)."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

from lidar_rt_amd import build as lrt_build, poses, resources, sweep as sw
from lidar_rt_amd.training import RangeFrames
from tests import sweep_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


# ---- 1. the twin in the static case -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,inc,conv", [(64, 2048, "bounds", "kitti"), (66, 1030, "table", "kitti"), (64, 2650, "table", "waymo_yaw"), (5, 37, "bounds", "waymo_yaw"),
                                          (1, 1, "bounds", "kitti")])
@pytest.mark.parametrize("twist", ["none", "zero"])
def test_the_static_twin_is_range_rays(H, W, inc, conv, twist):
    c = sc.make(H, W, 1, inc, conv, twist)
    o, d = sw.sweep_rays_reference(c.pose[0], None if c.twist is None else c.twist[0], **c.kw)
    assert o.dtype == d.dtype == torch.float64 and o.shape == d.shape == (H, W, 3)
    assert torch.equal(o, c.pose[0, :, 3].to(torch.float64).expand(H, W, 3))                   # bit for bit
    s2w = torch.eye(4)
    s2w[:3] = c.pose[0]
    o32, d32 = RangeFrames.range_rays(H, W, c.kw["inclination"], s2w, c.kw["data_type"], c.kw["sensor2ego"])
    err = float((d - d32.to(torch.float64)).abs().max())
    print(f"{c.key}: range_rays is {err:.2e} from the twin")
    assert err <= 1e-6
    assert torch.equal(o32.to(torch.float64), o)
    assert float(((d * d).sum(-1) - 1.0).abs().max()) < 1e-14
    # the CPU path of the operator: the twin rounded to float32 once
    oc, dc = sw.sweep_rays(c.pose[0], None if c.twist is None else c.twist[0], **c.kw)
    assert oc.dtype == torch.float32 and torch.equal(oc, o.to(torch.float32)) and torch.equal(dc, d.to(torch.float32))


# ---- 2. the twin's physics ---------------------------------------------------------------------------------------------------------------------------------

def _se3(xi):
    return poses.se3_exp(torch.as_tensor(xi, dtype=torch.float64))


@pytest.mark.parametrize("kind", ["below", "above", "large", "wide"])
def test_the_column_poses_are_the_pose_at_0_and_pose_exp_xi_at_1(kind):
    c = sc.make(5, 37, 3, twist=kind)
    tau = torch.tensor([0.0, 1.0, 0.5, -0.25], dtype=torch.float64)
    R, t = sw.column_poses_reference(c.pose, c.twist, tau)
    P = c.pose.to(torch.float64)
    assert torch.equal(R[:, 0], P[:, :, :3]) and torch.equal(t[:, 0], P[:, :, 3])
    for f in range(c.F):
        P4 = torch.eye(4, dtype=torch.float64)
        P4[:3] = P[f]
        for k, s in enumerate(tau.tolist()):
            want = P4 @ _se3(c.twist[f].to(torch.float64) * s)
            assert float((R[f, k] - want[:3, :3]).abs().max()) < 1e-14
            assert float((t[f, k] - want[:3, 3]).abs().max()) < 1e-11                             # the translation is a kilometre
        P4[:3, :3] = torch.from_numpy(sc._rot([0.3 + f, -1.1, 0.7]))                               # orthonormal in float64, which a float32 pose is not
        got = sw.twist_between(P4, P4 @ _se3(c.twist[f].to(torch.float64)))
        assert np.abs(got - c.twist[f].numpy().astype(np.float64)).max() < 1e-10


@pytest.mark.parametrize("angle", [0.0, 1e-12, 1e-7, 1e-4, 0.3, 0.5, 2.0, 3.0, np.pi - 1e-3, np.pi - 1e-6, np.pi - 1e-9, np.pi])
def test_log_is_the_inverse_of_exp(angle):
    rng = np.random.default_rng(5)
    for _ in range(4):
        a = rng.normal(size=3)
        xi = np.concatenate([rng.normal(size=3) * 3.0, a / np.linalg.norm(a) * angle])
        T = _se3(xi)
        got = sw.se3_log(T)
        back = _se3(got)
        assert float((back - T).abs().max()) < 1e-9, (angle, got, xi)                             # Exp(Log(T)) = T, also where Log is two-valued (pi)
        if angle < np.pi - 1e-7:
            assert np.abs(got - xi).max() < 1e-9, (angle, got, xi)
    assert np.array_equal(sw.se3_log(torch.eye(4)), np.zeros(6))
    assert np.array_equal(sw.twist_between(np.eye(4)[:3], np.eye(4)), np.zeros(6))


def test_column_times():
    t = sw.column_times(8)
    assert t.dtype == torch.float64 and torch.equal(t, (torch.arange(8, dtype=torch.float64) + 0.5) / 8 - 0.5)
    assert torch.equal(sw.column_times(8, t_ref=0.0), (torch.arange(8, dtype=torch.float64) + 0.5) / 8)
    assert torch.equal(sw.column_times(8, 0.25, "ccw"), -sw.column_times(8, 0.25, "cw"))
    assert float(sw.column_times(1)[0]) == 0.0
    with pytest.raises(sw.SweepError, match="direction"):
        sw.column_times(8, direction="up")
    with pytest.raises(sw.SweepError, match="columns"):
        sw.column_times(0)


def test_points_of_a_plane_seen_through_sweep_rays_lie_on_the_plane():
    """A moving sensor looks at a plane: r from the analytic intersection of every sweep ray, o + d r on the plane, and the origins move along the sweep."""
    c = sc.make(64, 256, 1, twist="large")
    o, d = sw.sweep_rays_reference(c.pose[0], c.twist[0], **c.kw)
    n = torch.tensor([0.2, -0.1, 1.0], dtype=torch.float64)
    n = n / n.norm()
    p0 = c.pose[0, :, 3].to(torch.float64) - 2.0 * n                                            # 2 m below the sensor
    r = ((p0 - o) * n).sum(-1) / (d * n).sum(-1)
    pts = o + d * r[..., None]
    assert float((((pts - p0) * n).sum(-1)).abs().max()) < 1e-9
    assert torch.equal(o[0], o[-1]) and float((o[0, 0] - o[0, -1]).norm()) > 2.5                # one origin per column; about |rho| between the first and the last


def test_the_per_ray_contributions_add_up_to_the_gradient():
    for c in (sc.case(5, 37, 3, "table", "waymo_yaw", "above", "explicit"), sc.case(3, 70, 1, "bounds", "kitti", "none", "default")):
        r = sc.reference(c)
        want = torch.cat([r.d_pose.reshape(c.F, 12), torch.zeros(c.F, 6, dtype=torch.float64) if r.d_twist is None else r.d_twist], 1)
        assert float((r.total - want).abs().max()) <= 1e-12 * float(r.A.max())
        assert bool((r.A >= r.total.abs() * (1 - 1e-12)).all())


def test_the_python_side_refuses_before_it_computes():
    P, x = torch.zeros(3, 4), torch.zeros(6)
    ok = dict(H=8, W=64, inclination=list(sc.KITTI_INC))
    for fn in (sw.sweep_rays, sw.sweep_rays_reference):
        with pytest.raises(sw.SweepError, match="pose must be"):
            fn(torch.zeros(3, 3), x, **ok)
        with pytest.raises(sw.SweepError, match="twist must be"):
            fn(P, torch.zeros(1, 6), **ok)
        with pytest.raises(sw.SweepError, match=r"twist must be \(2, 6\)"):
            fn(torch.zeros(2, 3, 4), torch.zeros(3, 6), **ok)
        with pytest.raises(sw.SweepError, match="inclination holds 7"):
            fn(P, x, 8, 64, [0.1] * 7)
        with pytest.raises(sw.SweepError, match="tau holds 63"):
            fn(P, x, **ok, tau=np.zeros(63))
        with pytest.raises(sw.SweepError, match="non-finite tau"):
            fn(P, x, **ok, tau=np.full(64, np.nan))
        with pytest.raises(sw.SweepError, match="data_type"):
            fn(P, x, **ok, data_type="nuScenes")
        with pytest.raises(sw.SweepError, match="a grid of"):
            fn(P, x, 0, 64, list(sc.KITTI_INC))
        with pytest.raises(sw.SweepError, match="differ"):
            fn(P, x.double(), **ok)
    o, d = sw.sweep_rays(torch.zeros(2, 4, 4) + torch.eye(4), None, 4, 8, 0.3)                   # one number: [-x, x]
    assert o.shape == d.shape == (2, 4, 8, 3)


# ---- 3. the rule's header on the host ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sweep_check") / "sweep_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "host_check", "sweep_check.cpp")])
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
        f.write(inc.tobytes()); f.write(tau.tobytes()); f.write(c.g_o.numpy().tobytes()); f.write(c.g_d.numpy().tobytes())
    res = subprocess.run([exe, inp, out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "SWEEPCHECK ok" in res.stdout, res.stdout + res.stderr
    worst = float(re.search(r"SWEEPCHECK branches (\S+)", res.stdout).group(1))
    raw = open(out, "rb").read()
    ncol, n3 = c.F * c.W * 12, c.F * c.H * c.W * 3
    cols = np.frombuffer(raw, np.float64, ncol).reshape(c.F, c.W, 12)
    rest = np.frombuffer(raw, np.float32, offset=8 * ncol)
    o, d = rest[:n3].reshape(c.F, c.H, c.W, 3), rest[n3:2 * n3].reshape(c.F, c.H, c.W, 3)
    dp, dt = rest[2 * n3:2 * n3 + 12 * c.F].reshape(c.F, 12), rest[2 * n3 + 12 * c.F:].reshape(c.F, 6)
    return cols, torch.from_numpy(o.copy()), torch.from_numpy(d.copy()), torch.from_numpy(dp.copy()), torch.from_numpy(dt.copy()), tau, worst


def test_the_rule_header_on_the_host_against_the_twin(host_check, tmp_path):
    """Per-column (R_w, t_w), every ray and the gradient of every small case; the series and the closed branch at the threshold to 2^-40."""
    cases = sc.all_cases_small()
    assert len(cases) >= 20 and {c.twist_kind for c in cases} == set(sc.TWISTS)
    for c in cases:
        cols, o, d, dp, dt, tau, worst = run_host(host_check, c, tmp_path)
        assert worst <= 2.0 ** -40
        r = sc.reference(c)
        R, t = sw.column_poses_reference(c.pose, c.twist, torch.from_numpy(tau))
        assert float((torch.from_numpy(cols[:, :, :9].copy()) - R.reshape(c.F, c.W, 9)).abs().max()) <= 2.0 ** -45, c.key
        assert float((torch.from_numpy(cols[:, :, 9:].copy()) - t).abs().max()) <= 2.0 ** -45 * r.scale, c.key
        assert sc.forward_excess(d, r.d, 1.0) <= 0.0, c.key
        assert sc.forward_excess(o, r.o, r.scale) <= 0.0, c.key
        assert sc.backward_excess(dp, r.d_pose.reshape(c.F, 12), r.A[:, :12]) <= 0.0, c.key
        if c.twist is not None:
            assert sc.backward_excess(dt, r.d_twist, r.A[:, 12:]) <= 0.0, c.key
        else:
            assert not dt.any()


# ---- 4. the library ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sweep_lib():
    return lrt_build.build_sweep()


def test_the_library_has_a_source_list_of_its_own_and_moves_no_other_hash():
    assert lrt_build.SWEEP_SOURCES == ["lrt_sweep.hip"] and "lrt_sweep_math.h" in lrt_build.SWEEP_HEADERS and "lrt_device_guard.h" in lrt_build.SWEEP_HEADERS
    others = (lrt_build.SOURCES + lrt_build.HEADERS + lrt_build.LOSS_SOURCES + lrt_build.LOSS_HEADERS + lrt_build.GRIDCD_SOURCES + lrt_build.GRIDCD_HEADERS
              + lrt_build.INIT_SOURCES + lrt_build.INIT_HEADERS + lrt_build.METRICS_SOURCES + lrt_build.METRICS_HEADERS + lrt_build.ADAM_SOURCES + lrt_build.ADAM_HEADERS
              + lrt_build.DENSIFY_SOURCES + lrt_build.DENSIFY_HEADERS + lrt_build.PROJECT_SOURCES + lrt_build.PROJECT_HEADERS)
    assert not any("lrt_sweep" in f for f in others)
    # the other libraries' hashes as tests/test_range_image.py pins them, and the projection library's at the commit this library was added on
    pinned = {"source_hash": "2c98b54882a7ff74", "loss_source_hash": "cc56b0c83f72d5ca", "gridcd_source_hash": "fd279d9f7ff67722", "init_source_hash": "0fd7105f5d08ab22",
              "metrics_source_hash": "9e8267ef6335030b", "adam_source_hash": "1b4949dcebd155a4", "densify_source_hash": "223b0fc546560708",
              "project_source_hash": "974b6f2b8535fc99"}
    for fn, want in pinned.items():
        assert getattr(lrt_build, fn)() == want, fn
    assert lrt_build.CODEGEN_FLAGS == ["-O3", "-munsafe-fp-atomics", "-fno-slp-vectorize"]
    assert "lrt_sweep" not in open(lrt_build.EXT_SRC).read()
    assert lrt_build.sweep_source_hash() not in pinned.values()
    assert os.path.basename(lrt_build.SWEEP_LIB) == "liblrt_sweep.so" and os.path.basename(lrt_build.SWEEP_STAMP) == "liblrt_sweep.srchash"
    src = open(lrt_build.__file__).read()
    assert "build_sweep(force, verbose)" in src[src.index("def _build_product"):src.index("def _build_lib")]
    assert "csrc/liblrt_sweep.so" in open(os.path.join(REPO, "setup.py")).read()
    body = src[src.index("def build_sweep"):src.index("EXT_SRC =")]
    assert "CODEGEN_FLAGS" in body and "resources.check(SWEEP_LIB)" in body


def test_the_library_builds_and_exports_what_its_header_declares(sweep_lib):
    assert os.path.exists(sweep_lib) and not lrt_build.sweep_is_stale()
    assert open(lrt_build.SWEEP_STAMP).read().strip() == lrt_build.sweep_source_hash()
    hdr = open(os.path.join(REPO, "include", "lrt_sweep.h")).read()
    declared = set(re.findall(r"\b(lrt_sweep_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(sw.EXPORTS), declared ^ set(sw.EXPORTS)
    lib = sw.load()
    for n in declared:
        assert hasattr(lib, n), n
    exported = set(re.findall(r"\blrt_sweep_[a-z_]+\b", subprocess.run(["nm", "-D", "--defined-only", sweep_lib], capture_output=True, text=True, check=True).stdout))
    assert exported == declared, exported ^ declared
    const = lambda name: int(re.search(r"#define\s+%s\s+\(?(\d+)" % name, hdr).group(1))
    assert lib.lrt_sweep_abi_version() == const("LRT_SWEEP_ABI_VERSION") == sw.ABI_VERSION
    assert const("LRT_SWEEP_BLOCK") == sw.BLOCK and const("LRT_SWEEP_COLS") == sw.COLS and const("LRT_SWEEP_MAX_RAYS") == sw.MAX_RAYS
    mh = open(os.path.join(REPO, "lidar_rt_amd", "csrc", "lrt_sweep_math.h")).read()
    assert len(re.findall(r"#define\s+SW_SERIES_TH2\b", mh)) == 1 and float(re.search(r"#define\s+SW_SERIES_TH2\s+(\S+)", mh).group(1)) == sw.SERIES_TH2
    assert int(re.search(r"#define\s+SW_SERIES_TERMS\s+(\d+)", mh).group(1)) == sw.SERIES_TERMS
    assert not re.search(r"\bfloat\b(?!\s*\*)", re.sub(r"//.*", "", mh).replace("const float*", ""))        # float64 throughout: float appears only as an input pointer


def test_the_kernels_pass_the_resource_gate(sweep_lib):
    res = resources.kernel_resources(sweep_lib)
    own = sorted(n for n in res if resources.is_own_kernel(n))
    assert own == ["k_sweep_bwd_cols", "k_sweep_bwd_finish", "k_sweep_rays", "k_sweep_tables"], own     # two launches forward, two backward
    assert all(n.startswith("k_sweep_") and any(re.search(g_, n) for g_ in resources.GATED) for n in own)
    assert resources.violations(res) == []
    for n in own:
        r = res[n]
        assert r["vgpr_spill"] == 0 and r["scratch_bytes"] == 0 and not r["dynamic_stack"], (n, r)
    resources.check(sweep_lib)


def test_argument_errors_come_before_the_device_and_launch_nothing(sweep_lib):
    lib = sw.load()
    buf = (C.c_char * 8192)()
    p = (C.addressof(buf) + 255) // 256 * 256
    err = lambda: lib.lrt_sweep_last_error()
    nodev = 1 << 20                                                                     # a device that does not exist: what passes the checks ends there
    wb = lib.lrt_sweep_work_bytes
    assert wb(0, 8, 64) < 0 and wb(1, 0, 64) < 0 and wb(1, 8, 0) < 0 and wb(3, 30000, 30000) < 0 and wb(1 << 40, 1, 1) < 0
    assert wb(1, 1, 1) == 256 and wb(3, 5, 37) == (8 * (9 * 3 * 37 + 2 * 5 + 18 * 3 * 1) + 255) // 256 * 256
    assert wb(3, 66, 1030) == (8 * (9 * 3 * 1030 + 2 * 66 + 18 * 3 * 17) + 255) // 256 * 256
    need = wb(1, 8, 64)

    def fwd(F=1, H=8, W=64, pose=p, twist=p, inc=p, n_inc=2, off=0.0, yaw=0.0, tau=p, outs=(p, p), ws=p, ws_bytes=need):
        return lib.lrt_sweep_rays(nodev, F, H, W, pose, twist, inc, n_inc, off, yaw, tau, *outs, ws, ws_bytes, None)

    def bwd(F=1, H=8, W=64, pose=p, twist=p, inc=p, n_inc=2, off=0.0, yaw=0.0, tau=p, gs=(p, p), d_pose=p, d_twist=p, ws=p, ws_bytes=need):
        return lib.lrt_sweep_backward(nodev, F, H, W, pose, twist, inc, n_inc, off, yaw, tau, *gs, d_pose, d_twist, ws, ws_bytes, None)
    for call in (fwd, bwd):
        assert call(F=0) < 0 and b"0 frames of 8 x 64" in err()
        assert call(F=3, H=30000, W=30000) < 0 and b"3 frames of 30000 x 30000" in err()
        assert call(n_inc=3) < 0 and b"3 inclinations" in err()
        assert call(off=1.0) < 0 and b"pixel offset" in err()
        assert call(yaw=float("nan")) < 0 and b"yaw" in err()
        assert call(yaw=float("inf")) < 0 and b"yaw" in err()
        assert call(pose=None) < 0 and b"null pose / inclination" in err()
        assert call(inc=None) < 0 and b"null pose / inclination" in err()
        assert call(tau=None) < 0 and b"null tau" in err()
        assert call(ws=p + 8) < 0 and b"256-byte aligned" in err()
        assert call(ws=None) < 0 and b"256-byte aligned" in err()
        assert call(ws_bytes=need - 1) < 0 and (b"a workspace of %d bytes, 1 frames of 8 x 64 need %d" % (need - 1, need)) in err()
        assert call() < 0 and b"no HIP device" in err()
        assert call(twist=None, tau=None) < 0 and b"no HIP device" in err()              # a static sensor reads no tau
        assert call(H=8, n_inc=8) < 0 and b"no HIP device" in err()
    assert fwd(outs=(None, p)) < 0 and b"null ray_o / ray_d" in err()
    assert fwd(outs=(p, None)) < 0 and b"null ray_o / ray_d" in err()
    assert bwd(gs=(None, p)) < 0 and b"null g_o / g_d" in err()
    assert bwd(gs=(p, None)) < 0 and b"null g_o / g_d" in err()
    assert bwd(d_pose=None) < 0 and b"null d_pose" in err()
    assert bwd(d_twist=None) < 0 and b"without a d_twist" in err()
    assert bwd(twist=None, d_twist=None) < 0 and b"no HIP device" in err()
    assert bwd(F=70000, H=1, W=1, ws_bytes=1 << 30) < 0 and b"70000 frames" in err()


# ---- 5. the plumbing ---------------------------------------------------------------------------------------------------------------------------------------

def _frames(n, H=4, W=16, twist_of=None, tau_of=None, ids=None):
    from lidar_rt_amd import scenes
    rng = np.random.default_rng(3)
    out = []
    for k, fid in enumerate(ids or range(n)):
        fr = {"id": fid, "depth": rng.uniform(2, 30, (H, W)).astype(np.float32), "intensity": rng.uniform(0, 1, (H, W)).astype(np.float32),
              "mask": rng.uniform(size=(H, W)) > 0.2, "inclination": np.array(sc.KITTI_INC, np.float32),
              "sensor2world": scenes.pose_matrix((0.5 * k, 0.1, 1.7), yaw=0.02 * k).astype(np.float32)}
        if twist_of is not None and twist_of(fid) is not None:
            fr["twist"] = twist_of(fid)
        if tau_of is not None and tau_of(fid) is not None:
            fr["tau"] = tau_of(fid)
        out.append(fr)
    return out


def test_a_sequence_keeps_its_twists_and_column_times(tmp_path):
    from lidar_rt_amd import sequence
    H, W = 4, 16
    tw = lambda f: np.array([1.5, 0.1 * f, 0.0, 0.0, 0.0, 0.02], np.float32)
    tau1 = np.linspace(0.4, -0.4, W).astype(np.float32)
    fr = _frames(3, H, W, twist_of=tw, tau_of=lambda f: tau1 if f == 1 else None)
    meta = sequence.write_sequence(str(tmp_path / "a"), fr)
    assert meta["format"] == sequence.FORMAT == "lidar-rt-amd-sequence/1"                        # the format string is unchanged
    z0, z1 = np.load(tmp_path / "a" / "frames" / "000000.npz"), np.load(tmp_path / "a" / "frames" / "000001.npz")
    assert set(z0.files) == {"depth", "intensity", "mask", "inclination", "sensor2world", "twist"} and "tau" in z1.files
    seq = sequence.load_sequence(str(tmp_path / "a"), "cpu", sweep="stored", sweep_ref=0.25, sweep_direction="ccw")
    assert seq.sweep == "stored" and sorted(seq.frames.sweep_meta) == [0, 1, 2]
    for f in range(3):
        t, tau = seq.frames.sweep_meta[f]
        assert torch.equal(t, torch.from_numpy(tw(f)))
        assert torch.equal(tau, torch.from_numpy(tau1) if f == 1 else sw.column_times(W, 0.25, "ccw").to(torch.float32))
        o, d = seq.frames.get_range_rays(f)
        wo, wd = sw.sweep_rays(torch.from_numpy(fr[f]["sensor2world"]), torch.from_numpy(tw(f)), H, W, list(sc.KITTI_INC), tau=tau)
        assert torch.equal(o, wo) and torch.equal(d, wd) and len(seq.frames.pose_meta[f]) == 4    # pose_meta keeps its 4-tuple
    # without a sweep nothing changes: the stored twists are not read, the rays are range_rays's
    for kw in ({}, {"sweep": None}, {"sweep": "off"}):
        plain = sequence.load_sequence(str(tmp_path / "a"), "cpu", **kw)
        assert plain.frames.sweep_meta == {}
        o, d = plain.frames.get_range_rays(1)
        wo, wd = RangeFrames.range_rays(H, W, tuple(float(np.float32(x)) for x in sc.KITTI_INC), torch.from_numpy(fr[1]["sensor2world"]))
        assert torch.equal(o, wo) and torch.equal(d, wd)
    # frames written without a twist have no such entry, and "stored" refuses them
    sequence.write_sequence(str(tmp_path / "b"), _frames(2, H, W))
    assert set(np.load(tmp_path / "b" / "frames" / "000000.npz").files) == {"depth", "intensity", "mask", "inclination", "sensor2world"}
    with pytest.raises(ValueError, match="no stored twist"):
        sequence.load_sequence(str(tmp_path / "b"), "cpu", sweep="stored")
    with pytest.raises(ValueError, match="sweep 'rolling'"):
        sequence.load_sequence(str(tmp_path / "b"), "cpu", sweep="rolling")
    with pytest.raises(ValueError, match="column times without a twist"):
        sequence.write_sequence(str(tmp_path / "c"), _frames(1, H, W, tau_of=lambda f: tau1))
    with pytest.raises(ValueError, match="16 column times"):
        sequence.write_sequence(str(tmp_path / "d"), _frames(1, H, W, twist_of=tw, tau_of=lambda f: tau1[:5]))
    with pytest.raises(ValueError, match="column times but no twist"):
        RangeFrames().add_range_image(0, torch.ones(H, W), torch.ones(H, W), torch.ones(H, W), sc.KITTI_INC, torch.eye(4), tau=tau1)


def test_twists_from_the_poses_of_a_constructed_trajectory(tmp_path):
    from lidar_rt_amd import sequence
    xi = np.array([1.2, -0.1, 0.03, 0.004, -0.002, 0.05])
    T0 = np.eye(4)
    T0[:3, :3], T0[:3, 3] = sc._rot([0.1, -0.2, 0.9]), [30.0, -12.0, 1.8]
    step = _se3(xi).numpy()
    ids = [0, 1, 3, 4]                                                                          # a gap of two: that interval holds two steps
    T = {i: T0 @ np.linalg.matrix_power(step, i) for i in ids}
    got = sw.twists_from_poses(T, 1.0)
    assert sorted(got) == ids
    for i in ids:
        assert np.abs(got[i] - xi).max() < 1e-12, (i, got[i])
    half = sw.twists_from_poses(T, 0.5)
    assert all(np.abs(half[i] - 0.5 * xi).max() < 1e-12 for i in ids)
    assert np.array_equal(got[4], got[3])                                                       # the last frame takes the previous interval
    with pytest.raises(sw.SweepError, match="at least two frames"):
        sw.twists_from_poses({7: T0})
    # through a sequence directory (float32 poses on disk: 2^-24 of 30 m over a 1.2 m step)
    fr = _frames(4, ids=ids)
    for f in fr:
        f["sensor2world"] = T[f["id"]].astype(np.float32)
    sequence.write_sequence(str(tmp_path / "a"), fr)
    seq = sequence.load_sequence(str(tmp_path / "a"), "cpu", frames=[1, 4], sweep="poses", sweep_fraction=0.5)     # the neighbours count, loaded or not
    assert sorted(seq.frames.sweep_meta) == [1, 4]
    for f in (1, 4):
        t, tau = seq.frames.sweep_meta[f]
        assert float((t.double() - torch.from_numpy(0.5 * xi)).abs().max()) < 1e-5
        assert torch.equal(tau, sw.column_times(16).to(torch.float32))
    sequence.write_sequence(str(tmp_path / "one"), fr[:1])
    with pytest.raises(ValueError, match="at least two frames"):
        sequence.load_sequence(str(tmp_path / "one"), "cpu", sweep="poses")


def _sweep_frames(waymo=False):
    H, W = 5, 37
    rf = RangeFrames()
    rng = np.random.default_rng(11)
    s2e = None
    if waymo:
        s2e = torch.eye(4)
        s2e[:3, :3] = torch.from_numpy(sc._rot([0.0, 0.0, 0.7])).float()
    for f in range(2):
        P = torch.eye(4)
        P[:3, :3] = torch.from_numpy(sc._rot([0.2 * (f + 1), -0.1, 0.6])).float()
        P[:3, 3] = torch.tensor([8.0 + f, -3.0, 1.5])
        inc = np.sort(rng.uniform(-0.3, 0.04, H)).astype(np.float32).tolist() if waymo else sc.KITTI_INC
        rf.add_range_image(f, torch.ones(H, W), torch.ones(H, W), torch.ones(H, W, dtype=torch.bool), inc, P, "Waymo" if waymo else "KITTI", s2e,
                           twist=torch.tensor([1.5, 0.2, -0.1, 0.01, -0.02, 0.3 + 0.1 * f]), tau=None if f == 0 else rng.uniform(-0.6, 0.6, W).astype(np.float32))
    return rf, H, W


@pytest.mark.parametrize("waymo", [False, True], ids=["kitti", "waymo_table_yaw"])
def test_sensor_poses_gradients_of_xi_and_twist_equal_float64_autograd_of_the_chain(waymo):
    """SensorPoses forms pose @ Exp(xi) in float32 and hands it to the operator (the twin on the CPU).  Against the whole chain in float64: the
    float32 product is 2^-24 relative per entry of a pose of at most 10 m, and d(ray)/d(pose) is O(1) here, so gradients of size G agree to a few
    2^-24 * 10 * G; the bound is 1e-5 of the largest entry."""
    rf, H, W = _sweep_frames(waymo)
    sp = poses.SensorPoses(rf, [0, 1], refine_twist=True)
    rng = np.random.default_rng(2)
    for f in (0, 1):
        with torch.no_grad():
            sp.xi[f].copy_(torch.tensor(rng.normal(size=6) * [0.05, 0.05, 0.05, 0.01, 0.01, 0.01], dtype=torch.float32))
        g_o, g_d = torch.tensor(rng.normal(size=(H, W, 3))), torch.tensor(rng.normal(size=(H, W, 3)))
        sp.zero_grad()
        o, d = sp.get_range_rays(f)
        assert o.shape == d.shape == (H, W, 3) and o.dtype == torch.float32
        ((o * g_o.float()).sum() + (d * g_d.float()).sum()).backward()
        inc, s2w, data_type, s2e = rf.pose_meta[f]
        xi64 = sp.xi[f].detach().double().requires_grad_(True)
        tw64 = sp.twist[f].detach().double().requires_grad_(True)
        o64, d64 = sw.sweep_rays_reference(s2w.double() @ poses.se3_exp(xi64), tw64, H, W, inc, data_type, s2e, tau=rf.sweep_meta[f][1])
        ((o64 * g_o).sum() + (d64 * g_d).sum()).backward()
        assert float((o.double() - o64).detach().abs().max()) < 1e-5 and float((d.double() - d64).detach().abs().max()) < 1e-6
        for got, want in ((sp.xi[f].grad, xi64.grad), (sp.twist[f].grad, tw64.grad)):
            assert got is not None and float((got.double() - want).abs().max()) <= 1e-5 * float(want.abs().max()), (f, got, want)
        other = 1 - f
        assert sp.xi[other].grad is None and sp.twist[other].grad is None
    # a step moves xi and twist of the frame with a gradient by their own learning rates, and nothing else
    before = {f: (sp.xi[f].detach().clone(), sp.twist[f].detach().clone()) for f in (0, 1)}
    sp.lr_trans, sp.lr_rot, sp.lr_twist_trans, sp.lr_twist_rot = 1e-2, 1e-3, 1e-4, 1e-5
    sp.step()
    assert torch.equal(sp.xi[0], before[0][0]) and torch.equal(sp.twist[0], before[0][1])
    for x, b, lr in ((sp.xi[1], before[1][0], (1e-2, 1e-3)), (sp.twist[1], before[1][1], (1e-4, 1e-5))):
        step = (x.detach() - b).abs()
        assert torch.allclose(step[:3], torch.full((3,), lr[0]), rtol=2e-2, atol=2e-7) and torch.allclose(step[3:], torch.full((3,), lr[1]), rtol=2e-2, atol=2e-7), step


def test_sensor_poses_state_dicts_with_and_without_twists():
    rf, H, W = _sweep_frames()
    fixed = poses.SensorPoses(rf, [0, 1])                                                        # sweep rays, twists not refined
    assert not fixed.refine_twist and len(fixed.optimizer.param_groups) == 1 and not isinstance(fixed.twist[0], torch.nn.Parameter)
    o, d = fixed.get_range_rays(1)
    assert float((o[0, 0] - o[0, -1]).detach().norm()) > 0.1                                     # one origin per column
    with torch.no_grad():
        wo, wd = sw.sweep_rays(rf.pose_meta[1][1], rf.sweep_meta[1][0], H, W, list(sc.KITTI_INC), tau=rf.sweep_meta[1][1])
    assert torch.equal(o.detach(), wo) and torch.equal(d.detach(), wd) and torch.equal(wo, rf.rays[1][0])
    # a frames object without sweeps: exactly the old state dict, and refine_twist is refused
    plain = RangeFrames()
    for f in (0, 1):
        plain.add_range_image(f, torch.ones(H, W), torch.ones(H, W), torch.ones(H, W, dtype=torch.bool), sc.KITTI_INC, torch.eye(4))
    old = poses.SensorPoses(plain, [0, 1])
    (old.get_range_rays(0)[1] * torch.arange(3.0)).sum().backward()
    old.step()
    sd_old = old.state_dict()
    assert set(sd_old) == {"xi", "optimizer", "lr_trans", "lr_rot"} and old.twist == {}
    with pytest.raises(ValueError, match="refine_twist needs frames with sweep rays"):
        poses.SensorPoses(plain, [0], refine_twist=True)
    # an old state dict (no twists, one parameter group) loads into a model that refines twists
    new = poses.SensorPoses(rf, [0, 1], refine_twist=True, lr_twist_trans=3e-3)
    tw0 = new.twist[0].detach().clone()
    new.load_state_dict(sd_old)
    assert torch.equal(new.xi[0].detach(), sd_old["xi"][0]) and torch.equal(new.twist[0].detach(), tw0) and new.lr_twist_trans == 3e-3
    assert new.optimizer.state[new.xi[0]]["step"] == 1 and new.twist[0] not in new.optimizer.state
    # and its own state dict round-trips, twists and moments included
    (new.get_range_rays(1)[0].sum() + new.get_range_rays(1)[1][..., 2].sum()).backward()
    new.step()
    sd = new.state_dict()
    assert set(sd) == {"xi", "optimizer", "lr_trans", "lr_rot", "twist", "refine_twist", "lr_twist_trans", "lr_twist_rot"}
    again = poses.SensorPoses(rf, [0, 1], refine_twist=True)
    again.load_state_dict(sd)
    assert all(torch.equal(again.twist[f].detach(), new.twist[f].detach()) and torch.equal(again.xi[f].detach(), new.xi[f].detach()) for f in (0, 1))
    assert again.lr_twist_trans == 3e-3 and torch.equal(again.optimizer.state[again.twist[1]]["exp_avg"], new.optimizer.state[new.twist[1]]["exp_avg"])


def test_the_command_lines_refuse_what_cannot_work(tmp_path, capsys):
    from lidar_rt_amd import evaluate, ingest, train
    for argv, msg in ((["--refine-twist", "--sweep", "stored"], "--refine-twist needs --refine-poses"),
                      (["--refine-twist", "--refine-poses"], "--refine-twist needs a sweep"),
                      (["--refine-twist", "--refine-poses", "--sweep", "poses", "--gpus", "2"], "needs ray gradients"),
                      (["--sweep", "rolling"], "invalid choice")):
        with pytest.raises(SystemExit) as e:
            train.main(["--data", "unused"] + argv)
        assert e.value.code == 2 and msg in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--data", "unused", "--ckpt", "unused", "--sweep", "rolling"])
    assert e.value.code == 2 and "invalid choice" in capsys.readouterr().err
    # ingest --sweep stores the twists of the pose file; one frame has no neighbour
    rng = np.random.default_rng(0)
    xi = np.array([0.8, 0.0, 0.0, 0.0, 0.0, 0.03])
    os.makedirs(tmp_path / "pts")
    T = np.stack([np.linalg.matrix_power(_se3(xi).numpy(), k) for k in range(3)])
    for k in range(3):
        p = rng.normal(size=(500, 4)).astype(np.float32) * [10, 10, 0.5, 1]
        np.save(tmp_path / "pts" / f"{k}.npy", p.astype(np.float32))
    np.save(tmp_path / "poses.npy", T)
    common = ["--height", "8", "--width", "64", "--inclination", str(sc.KITTI_INC[0]), str(sc.KITTI_INC[1]), "--device", "cpu"]
    assert ingest.main(["--points", str(tmp_path / "pts"), "--poses", str(tmp_path / "poses.npy"), "--out", str(tmp_path / "seq"), "--sweep", "--sweep-fraction", "0.5"] + common) == 0
    for k in range(3):
        assert np.abs(np.load(tmp_path / "seq" / "frames" / f"{k:06d}.npz")["twist"] - 0.5 * xi).max() < 1e-6
    assert ingest.main(["--points", str(tmp_path / "pts"), "--poses", str(tmp_path / "poses.npy"), "--out", str(tmp_path / "plain")] + common) == 0
    assert "twist" not in np.load(tmp_path / "plain" / "frames" / "000000.npz").files
    os.makedirs(tmp_path / "one")
    np.save(tmp_path / "one" / "0.npy", np.load(tmp_path / "pts" / "0.npy"))
    np.save(tmp_path / "pose1.npy", T[:1])
    assert ingest.main(["--points", str(tmp_path / "one"), "--poses", str(tmp_path / "pose1.npy"), "--out", str(tmp_path / "refused"), "--sweep"] + common) == 2
    assert "at least two frames" in capsys.readouterr().err
