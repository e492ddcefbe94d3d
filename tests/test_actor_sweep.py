"""Actors that move within a sweep without a GPU: the thirteenth product library (`liblrt_actorsweep.so`: a source list and hash of its own,
exports, resource gate, argument errors before the device is touched), the rule's header compiled for the host against the float64 twin Gaussian
for Gaussian (plain and under the address and undefined-behaviour sanitizers), the search against the enumeration of all columns, a still actor
against `project_points_sweep_reference`, an actor that rides with the sensor, bit-for-bit pass-through, gradcheck of the twin, twists from
tracking boxes, and the sequence round trip of stored twists."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

from lidar_rt_amd import actor_sweep as asw, build as lrt_build, poses as lrt_poses, resources, sequence, sweep, sweep_project as sp
from tests import actor_sweep_cases as ac

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


# ---- 1. the library -------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def actorsweep_lib():
    return lrt_build.build_actorsweep()


def test_the_library_has_a_source_list_of_its_own(actorsweep_lib):
    assert lrt_build.ACTORSWEEP_SOURCES == ["lrt_actorsweep.hip"]
    assert {"lrt_actorsweep_math.h", "lrt_sweepproj_math.h", "lrt_project_math.h", "lrt_sweep_math.h", "lrt_device_guard.h"} <= set(lrt_build.ACTORSWEEP_HEADERS)
    lists = ("", "LOSS_", "GRIDCD_", "INIT_", "METRICS_", "ADAM_", "DENSIFY_", "PROJECT_", "SWEEP_", "REFINE_", "SWEEPPROJ_", "UNPROJECT_")
    others = sum((getattr(lrt_build, p + "SOURCES") + getattr(lrt_build, p + "HEADERS") for p in lists), [])
    assert not any("lrt_actorsweep" in f for f in others)
    assert os.path.basename(lrt_build.ACTORSWEEP_LIB) == "liblrt_actorsweep.so" and os.path.basename(lrt_build.ACTORSWEEP_STAMP) == "liblrt_actorsweep.srchash"
    src = open(lrt_build.__file__).read()
    product = src[src.index("def _build_product"):src.index("def _build_lib")]
    assert product.index("build_unproject(force, verbose)") < product.index("build_actorsweep(force, verbose)")
    assert "csrc/liblrt_actorsweep.so" in open(os.path.join(REPO, "setup.py")).read()
    body = src[src.index("def build_actorsweep"):src.index("EXT_SRC =")]
    assert "CODEGEN_FLAGS" in body and "resources.check(ACTORSWEEP_LIB)" in body
    assert os.path.exists(actorsweep_lib) and not lrt_build.actorsweep_is_stale()
    assert open(lrt_build.ACTORSWEEP_STAMP).read().strip() == lrt_build.actorsweep_source_hash()


def test_the_library_exports_what_its_header_declares(actorsweep_lib):
    hdr = open(os.path.join(REPO, "include", "lrt_actorsweep.h")).read()
    declared = set(re.findall(r"\b(lrt_actorsweep_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(asw.EXPORTS), declared ^ set(asw.EXPORTS)
    lib = asw.load()
    exported = set(re.findall(r"\blrt_actorsweep_[a-z_]+\b", subprocess.run(["nm", "-D", "--defined-only", actorsweep_lib], capture_output=True, text=True, check=True).stdout))
    assert exported == declared, exported ^ declared
    const = lambda name: int(re.search(r"#define\s+%s\s+\(?(\d+)" % name, hdr).group(1))
    assert lib.lrt_actorsweep_abi_version() == const("LRT_ACTORSWEEP_ABI_VERSION") == asw.ABI_VERSION
    assert const("LRT_ACTORSWEEP_N_COUNTS") == asw.N_COUNTS == len(asw.COUNT_NAMES) == 4 and const("LRT_ACTORSWEEP_BLOCK") == asw.BLOCK == 256
    assert const("LRT_ACTORSWEEP_MAX_EVAL") == asw.MAX_EVAL == sp.MAX_EVAL and const("LRT_ACTORSWEEP_TABLE") == asw.TABLE == 12
    assert const("LRT_ACTORSWEEP_MAX_POINTS") == asw.MAX_POINTS and const("LRT_ACTORSWEEP_MAX_ASSETS") == asw.MAX_ASSETS and const("LRT_ACTORSWEEP_MAX_COLUMNS") == asw.MAX_COLUMNS
    mh = open(os.path.join(REPO, "lidar_rt_amd", "csrc", "lrt_actorsweep_math.h")).read()
    for name, v in (("AS_MAX_EVAL", asw.MAX_EVAL), ("AS_TABLE", asw.TABLE), ("AS_CONVERGED", asw.CONVERGED), ("AS_UNCONVERGED", asw.UNCONVERGED), ("AS_INVALID", asw.INVALID)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, mh).group(1)) == v
    assert '#include "lrt_sweepproj_math.h"' in mh


def test_the_kernels_pass_the_resource_gate(actorsweep_lib):
    res = resources.kernel_resources(actorsweep_lib)
    own = sorted(n for n in res if resources.is_own_kernel(n))
    assert own == ["k_as_bwd", "k_as_finish", "k_as_fwd", "k_as_table"], own               # two launches forward, two backward
    assert resources.violations(res) == []
    for n in own:
        r = res[n]
        assert r["vgpr_spill"] == 0 and r["scratch_bytes"] == 0 and not r["dynamic_stack"], (n, r)
    resources.check(actorsweep_lib)


def test_argument_errors_come_before_the_device_and_launch_nothing(actorsweep_lib):
    lib = asw.load()
    buf = (C.c_char * 16384)()
    p = (C.addressof(buf) + 255) // 256 * 256
    err = lambda: lib.lrt_actorsweep_last_error()
    nodev = 1 << 20                                                                     # a device that does not exist: what passes the checks ends there
    wb = lib.lrt_actorsweep_work_bytes
    assert wb(-1, 1, 64) < 0 and wb(10, 0, 64) < 0 and wb(10, 1, 0) < 0 and wb(2 ** 30 + 1, 1, 64) < 0 and wb(10, 2 ** 20 + 1, 64) < 0 and wb(10, 1, 2 ** 20 + 1) < 0
    assert wb(0, 1, 1) == 256 + 256 and wb(1000, 4, 64) == 64 * 96 + 512 and wb(80_000, 10, 2048) == 2048 * 96 + (48 * (313 + 10) + 255) // 256 * 256

    def fwd(P=10, A=2, xyz=p, rot=p, seg=p, poses=p, twist=p, w2s=p, xi=None, tau=p, W=64, off=0.0, yaw=0.0, outs=(p, p, p, p), ws=p, ws_bytes=8192):
        return lib.lrt_actorsweep_forward(nodev, P, A, xyz, rot, seg, poses, twist, w2s, xi, tau, W, off, yaw, *outs, ws, ws_bytes, None)

    def bwd(P=10, A=2, xyz=p, rot=p, seg=p, poses=p, twist=p, tau=p, W=64, column=p, g=(p, p), outs=(p, p, p), ws=p, ws_bytes=8192):
        return lib.lrt_actorsweep_backward(nodev, P, A, xyz, rot, seg, poses, twist, tau, W, column, *g, *outs, ws, ws_bytes, None)
    for call in (fwd, bwd):
        assert call(P=-1) < 0 and b"-1 Gaussians" in err()
        assert call(A=0) < 0 and b"0 assets" in err()
        assert call(W=0) < 0 and b"0 columns" in err()
        assert call(W=-5) < 0 and b"-5 columns" in err()
        assert call(xyz=None) < 0 and b"null xyz / rot_raw" in err()
        assert call(rot=None) < 0 and b"null xyz / rot_raw" in err()
        for k in ("seg", "poses", "twist"):
            assert call(**{k: None}) < 0 and b"null seg_start / poses / actor_twist" in err()
        assert call(tau=None) < 0 and b"null tau" in err()
        assert call(rot=p + 8) < 0 and b"rot_raw must be 16-byte aligned" in err()
        assert call(ws=None) < 0 and b"256-byte aligned" in err()
        assert call(ws=p + 8) < 0 and b"256-byte aligned" in err()
        assert call(ws_bytes=64 * 96 + 255) < 0 and b"a workspace of 6399 bytes, 10 Gaussians in 2 assets and 64 columns need 6400" in err()
        assert call() < 0 and b"no HIP device" in err()
    assert fwd(w2s=None) < 0 and b"null world2sensor" in err()
    assert fwd(off=1.0) < 0 and b"pixel offset" in err()
    assert fwd(yaw=float("nan")) < 0 and b"yaw" in err()
    for k in range(4):
        assert fwd(outs=tuple(None if j == k else p for j in range(4))) < 0 and b"null xyz_s / rot_s / column / counts" in err()
    assert fwd(outs=(p, p + 4, p, p)) < 0 and b"rot_s must be 16-byte aligned" in err()
    assert bwd(g=(p, p + 8)) < 0 and b"g_rot_s and d_rot_raw must be 16-byte aligned" in err()
    assert bwd(outs=(p, p + 4, p)) < 0 and b"g_rot_s and d_rot_raw must be 16-byte aligned" in err()
    assert fwd(xi=p) < 0 and b"no HIP device" in err()
    assert fwd(P=0, xyz=None, rot=None, outs=(None, None, None, p)) < 0 and b"no HIP device" in err()
    assert bwd(column=None) < 0 and b"null column" in err()
    for k in range(2):
        assert bwd(g=tuple(None if j == k else p for j in range(2))) < 0 and b"null column / g_xyz_s" in err()
    assert bwd(outs=(p, p, None)) < 0 and b"null d_actor_twist" in err()
    assert bwd(outs=(None, p, p)) < 0 and b"d_xyz" in err()


def test_the_python_side_refuses_before_it_computes():
    c = ac.case(65, "mixed", 64)
    ok = ac.arguments(c)
    for fn in (asw.actor_sweep, asw.actor_sweep_reference):
        with pytest.raises(asw.ActorSweepError, match=r"xyz must be a \(N, 3\)"):
            fn(**{**ok, "xyz": c.xyz[:, :2]})
        with pytest.raises(asw.ActorSweepError, match="65 centres and 64 rotations"):
            fn(**{**ok, "rot_raw": c.rot[:64]})
        with pytest.raises(asw.ActorSweepError, match="twist rows"):
            fn(**{**ok, "actor_twist": c.twist[:3]})
        with pytest.raises(asw.ActorSweepError, match="int32"):
            fn(**{**ok, "seg_start": c.seg.long()})
        with pytest.raises(asw.ActorSweepError, match="int32"):
            fn(**{**ok, "seg_start": c.seg[:-1]})
        with pytest.raises(asw.ActorSweepError, match="columns"):
            fn(**{**ok, "W": 0})
        with pytest.raises(asw.ActorSweepError, match="tau must be"):
            fn(**{**ok, "tau": c.tau[:-1]})
        with pytest.raises(asw.ActorSweepError, match="sensor_twist must be"):
            fn(**{**ok, "sensor_twist": torch.zeros(5)})
        with pytest.raises(asw.ActorSweepError, match="sensor_pose must be"):
            fn(**{**ok, "sensor_pose": torch.eye(3)})
        with pytest.raises(asw.ActorSweepError, match="data_type"):
            fn(**{**ok, "data_type": "nuScenes"})
    with pytest.raises(asw.ActorSweepError, match="a workspace with Gaussians on cpu"):
        asw.actor_sweep(**ok, workspace=torch.zeros(8192, dtype=torch.uint8))


# ---- 2. the rule's header on the host -------------------------------------------------------------------------------------------------------------------

CHECK_SRC = os.path.join(HERE, "host_check", "actorsweep_check.cpp")


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("actorsweep_check") / "actorsweep_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, CHECK_SRC])
    return exe


@pytest.fixture(scope="module")
def host_check_sanitized(tmp_path_factory):
    """The same stand-alone program under the address and undefined-behaviour sanitizers; None where g++ cannot link their runtime."""
    d = tmp_path_factory.mktemp("actorsweep_check_san")
    probe = str(d / "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + flags + ["-o", str(d / "probe"), probe], capture_output=True).returncode != 0:
        return None
    exe = str(d / "actorsweep_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", exe, CHECK_SRC])
    return exe


def run_host(exe, c, tmp_path):
    off, yaw = sweep.convention(c.conv["data_type"], c.conv["sensor2ego"])
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    f64 = lambda t: np.ascontiguousarray(t.numpy(), np.float64).tobytes()
    f32 = lambda t: np.ascontiguousarray(t.numpy(), np.float32).tobytes()
    with open(inp, "wb") as f:
        f.write(struct.pack("<4i", c.P, c.A, c.W, int(c.sensor_twist is not None)))
        f.write(struct.pack("<2d", off, yaw))
        f.write(c.seg.numpy().astype(np.int32).tobytes()); f.write(f32(c.poses)); f.write(f32(c.twist)); f.write(f64(asw.world2sensor(c.sensor_pose)))
        if c.sensor_twist is not None:
            f.write(f64(c.sensor_twist))
        f.write(f64(c.tau)); f.write(f32(c.xyz)); f.write(f32(c.rot)); f.write(f32(c.g_xyz)); f.write(f32(c.g_rot))
    res = subprocess.run([exe, inp, out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "ACTORSWEEPCHECK ok" in res.stdout, res.stdout + res.stderr
    raw = open(out, "rb").read()
    P = c.P
    ints = np.frombuffer(raw, np.int32, 3 * P).reshape(P, 3)
    flt = np.frombuffer(raw, np.float32, 14 * P, 12 * P).reshape(P, 14)
    dbl = np.frombuffer(raw, np.float64, 6 * P, 12 * P + 56 * P).reshape(P, 6)
    return ints, torch.tensor(flt), torch.tensor(dbl)


def compare_host(exe, cases, tmp_path):
    states, most = set(), 0
    for c in cases:
        ints, flt, dbl = run_host(exe, c, tmp_path)
        r = c.ref
        assert np.array_equal(ints[:, 0], r.column.numpy()), c.key
        assert np.array_equal(ints[:, 1], r.state.numpy()), c.key
        assert np.array_equal(ints[:, 2], r.evals.numpy()), c.key
        assert ac.excess(flt[:, 0:3], r.xyz_s, r.A_xyz) <= 0.0 and ac.excess(flt[:, 3:7], r.rot_s, r.A_rot) <= 0.0, c.key
        assert ac.excess(flt[:, 7:10], r.d_xyz, r.A_dx) <= 0.0 and ac.excess(flt[:, 10:14], r.d_rot, r.A_dr) <= 0.0, c.key
        passing = ~r.moved
        assert torch.equal(flt[passing, 0:3].view(torch.int32), c.xyz[passing].view(torch.int32)), c.key       # bit for bit
        assert torch.equal(flt[passing, 3:7].view(torch.int32), c.rot[passing].view(torch.int32)), c.key
        assert float((dbl - r.contrib).abs().max()) <= 2.0 ** -34 * float(r.contrib.abs().max()) if c.P else True, c.key
        d_twist = torch.zeros(c.A, 6, dtype=torch.float64).index_add_(0, r.asset, dbl)
        assert ac.twist_excess(d_twist.float(), r.d_twist, r.A_tw) <= 0.0, c.key
        states |= set(ints[:, 1].tolist())
        most = max(most, int(ints[:, 2].max()))
    return states, most


def test_the_rule_header_on_the_host_against_the_twin(host_check, tmp_path):
    """Column, search state and evaluations of EVERY Gaussian of every small case equal the twin's; the float32 outputs and gradients are within
    half an ulp plus 2^-40 of the absolute terms of the un-rounded twin; the rows that pass are the inputs bit for bit."""
    cases = ac.all_cases_small()
    states, most = compare_host(host_check, cases, tmp_path)
    assert states == {asw.CONVERGED, asw.UNCONVERGED, asw.NOT_SEARCHED} and most == asw.MAX_EVAL and len(cases) >= 15
    assert {c.W for c in cases} == set(ac.COLUMNS) and {c.P for c in cases} == set(ac.SIZES)


def test_the_host_program_under_the_sanitizers(host_check_sanitized, tmp_path):
    """A stand-alone host program: nothing is loaded into Python, nothing is preloaded."""
    if host_check_sanitized is None:
        pytest.skip("g++ cannot link the sanitizer runtime here")
    states, most = compare_host(host_check_sanitized, ac.all_cases_small(), tmp_path)
    assert asw.UNCONVERGED in states and most == asw.MAX_EVAL


# ---- 3. the search ------------------------------------------------------------------------------------------------------------------------------------------

def enumerate_fixed_points(c):
    """(P, W) bool by independent vectorised numpy: does column w, at its own instant, see the centre in its own bin?"""
    off, yaw = sweep.convention(c.conv["data_type"], c.conv["sensor2ego"])
    W, P = c.W, c.P
    tau = c.tau.numpy()
    asset = np.repeat(np.arange(c.A), np.diff(c.seg.numpy()))
    S2W = c.sensor_pose.numpy()
    xi = np.zeros(6) if c.sensor_twist is None else c.sensor_twist.numpy()
    x = np.concatenate([c.xyz.numpy().astype(np.float64), np.ones((P, 1))], 1)
    fixed = np.zeros((P, W), bool)
    box = {}
    for a in range(c.A):
        box[a] = asw.box_pose((c.poses[a, :3], c.poses[a, 3:7]))
    for w in range(W):
        Tw = np.linalg.inv(S2W @ lrt_poses.se3_exp(torch.tensor(tau[w] * xi)).numpy())
        for a in range(c.A):
            sel = asset == a
            if not sel.any():
                continue
            Aw = box[a] @ lrt_poses.se3_exp(torch.tensor(tau[w] * c.twist[a].double().numpy())).numpy()
            q = x[sel] @ (Tw @ Aw).T
            u = (np.pi - (np.arctan2(q[:, 1], q[:, 0]) + yaw)) * W / (2.0 * np.pi) - off
            fixed[sel, w] = np.mod(np.rint(u), W) == w
    return fixed


@pytest.mark.parametrize("c", [ac.case(257, "three", 64), ac.case(255, "three", 64, "waymo_yaw", "ccw"), ac.case(257, "three", 1030, "waymo_yaw", "ccw")], ids=lambda c: str(c.key[:5]))
def test_the_search_against_the_enumeration_of_all_columns(c):
    fixed = enumerate_fixed_points(c)
    r = c.ref
    conv = (r.state == asw.CONVERGED).numpy()
    col = r.column.numpy()
    assert conv.sum() >= 0.95 * c.P
    assert fixed[np.flatnonzero(conv), col[conv]].all()                                   # a converged w* lies in S
    single = fixed.sum(1) == 1
    assert (single & conv).sum() > 0                                                      # the property below is tested on something
    assert np.array_equal(col[single & conv], fixed[single & conv].argmax(1))             # |S| = 1 and converged: that column
    unc = (r.state == asw.UNCONVERGED).numpy()
    assert ((col[unc] >= 0) & (col[unc] < c.W)).all() and (r.evals.numpy()[unc] == asw.MAX_EVAL).all()


def test_a_still_actor_under_a_sensor_twist_has_the_column_of_project_points_sweep():
    """eta -> 0 (a twist too small to move a float64 coordinate; an all-zero row is not searched at all): the column is the one the projection
    under the sweep model gives the world point A x.  A is the identity here so that A x is the float32 point itself."""
    for W, conv, direction in ((64, "kitti", "cw"), (1030, "waymo_yaw", "ccw")):
        base = ac.case(1000, "one", W, conv, direction, check=False)
        rng = np.random.default_rng(5)
        az, rr = rng.uniform(-np.pi, np.pi, 1000), rng.uniform(3.0, 60.0, 1000)
        s2w = base.sensor_pose.numpy()
        world = (s2w[:3, 3] + np.stack([rr * np.cos(az), rr * np.sin(az), rng.uniform(-1, 1, 1000)], 1)).astype(np.float32)
        poses = torch.tensor([[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]])
        tiny = torch.tensor([[1e-30, 0.0, 0.0, 0.0, 0.0, 0.0]])
        t = asw.actor_sweep_reference(torch.tensor(world), base.rot, base.seg, poses, tiny, base.sensor_pose, base.sensor_twist, base.tau, W, **base.conv)
        assert t.margin >= ac.MARGIN and torch.equal(t.xyz_s.float(), torch.tensor(world))
        pr = sp.project_points_sweep_reference(np.concatenate([world, np.zeros((1000, 1), np.float32)], 1), 8, W, [-1.5, 1.5], base.sensor_twist.numpy(),
                                               data_type=base.conv["data_type"], sensor2ego=base.conv["sensor2ego"],
                                               points2sensor=asw.world2sensor(base.sensor_pose).numpy()[None], tau=base.tau.numpy(), max_depth=1000.0)
        assert pr.margin >= ac.MARGIN
        kept = (pr.drop == sp.KEEP).numpy() & (t.state == asw.CONVERGED).numpy()
        assert kept.sum() >= 900
        assert np.array_equal(pr.pixel.numpy()[kept, 0], t.column.numpy()[kept])
        unseen = (pr.drop == sp.UNSEEN).numpy()
        assert np.array_equal(unseen, (t.state == asw.UNCONVERGED).numpy())
        assert np.array_equal(pr.evals.numpy(), t.evals.numpy())


def test_an_actor_that_rides_with_the_sensor_keeps_its_static_column():
    """A = P and eta = xi: (P Exp(s xi))^-1 A Exp(s eta) is the identity for every s, so every centre is seen where it stands in the sensor frame."""
    for W, conv in ((64, "kitti"), (1030, "waymo_yaw")):
        base = ac.case(1000, "one", W, conv, check=False)
        row = base.poses[:1].clone()
        Ra, ta, _ = asw._pose_table(row, torch.float64)
        P = torch.cat([Ra[0], ta[0][:, None]], 1)
        eta = torch.tensor([[1.5, 0.25, 0.0, 0.0, 0.0078125, 0.0625]])
        x = (base.xyz * 8.0 + torch.tensor([3.0, 0.0, 0.0])).contiguous()
        t = asw.actor_sweep_reference(x, base.rot, base.seg, row, eta, P, eta[0].double(), base.tau, W, **base.conv)
        off, yaw = sweep.convention(base.conv["data_type"], base.conv["sensor2ego"])
        u = asw._u_of(x.double(), W, off, yaw)
        assert float(((u - torch.round(u)).abs() - 0.5).abs().min()) >= 1e-9 and t.margin >= 1e-9
        assert torch.equal(t.column.long(), asw._column_of(torch.round(u), W)) and bool((t.state == asw.CONVERGED).all()) and int(t.evals.max()) == 1
        # the centre in its column's frame is the static one
        table = asw.column_table(asw.world2sensor(P), eta[0].double(), base.tau.double())[t.column.long()]
        q = asw._rigid(table[:, :, :3], table[:, :, 3], asw._rigid(Ra, ta, t.xyz_s))
        assert float((q - x.double()).abs().max()) <= 1e-12 * 30.0


# ---- 4. pass-through -----------------------------------------------------------------------------------------------------------------------------------------

def test_pass_through_is_bit_for_bit():
    c = ac.case(1000, "mixed", 64)
    xyz_s, rot_s, info = asw.actor_sweep(**ac.arguments(c))
    assert xyz_s.dtype == rot_s.dtype == torch.float32 and info.column.dtype == torch.int32 and info.counts.dtype == torch.int64
    asset = c.ref.asset
    unposed = asset == 1                                                                   # the unposed asset in the middle; asset 2 is empty
    assert int(unposed.sum()) == 300 and int((asset == 2).sum()) == 0 and int((asset == 3).sum()) == 300
    assert torch.equal(xyz_s[unposed].view(torch.int32), c.xyz[unposed].view(torch.int32)) and torch.equal(rot_s[unposed].view(torch.int32), c.rot[unposed].view(torch.int32))
    assert bool((info.column[unposed] == -1).all()) and bool((info.column[~unposed] >= 0).all())
    assert not torch.equal(xyz_s[~unposed], c.xyz[~unposed]) and info.counts.tolist() == c.ref.counts.tolist() and int(info.counts[0]) == 700
    # a zero twist row
    s = ac.case(256, "still", 64, "waymo_yaw")
    xs, rs, inf = asw.actor_sweep(**ac.arguments(s))
    assert torch.equal(xs[:128].view(torch.int32), s.xyz[:128].view(torch.int32)) and torch.equal(rs[:128].view(torch.int32), s.rot[:128].view(torch.int32))
    assert bool((inf.column[:128] == -1).all()) and inf.counts.tolist()[:2] == [128, 128]
    # all twists zero: nothing changes at all
    xz, rz, iz = asw.actor_sweep(**ac.arguments(c, actor_twist=torch.zeros_like(c.twist)))
    assert torch.equal(xz.view(torch.int32), c.xyz.view(torch.int32)) and torch.equal(rz.view(torch.int32), c.rot.view(torch.int32)) and iz.counts.tolist() == [0, 1000, 0, 0]
    # tau[w*] == 0: the Gaussian passes and still records its column
    tau = c.tau.clone()
    cols = c.ref.column.long()
    w0 = int(torch.mode(cols[cols >= 0]).values)
    tau[w0] = 0.0
    xt, rt, it = asw.actor_sweep(**ac.arguments(c, tau=tau))
    at = it.column == w0
    assert int(at.sum()) >= 1
    assert torch.equal(xt[at].view(torch.int32), c.xyz[at].view(torch.int32)) and torch.equal(rt[at].view(torch.int32), c.rot[at].view(torch.int32))
    assert int(it.counts[1]) == 300 + int(at.sum())
    # -0.0 and a NaN survive a pass
    odd = c.xyz.clone()
    odd[450] = torch.tensor([-0.0, float("nan"), 1.0])
    xo, _, _ = asw.actor_sweep(**ac.arguments(c, xyz=odd))
    assert torch.equal(xo[450].view(torch.int32), odd[450].view(torch.int32))


def test_a_centre_that_is_not_finite_or_on_the_sensor_axis_is_invalid_and_passes():
    c = ac.case(65, "one", 64, check=False)
    xyz = c.xyz.clone()
    xyz[3] = torch.tensor([float("nan"), 0.0, 0.0])
    xyz[7] = torch.tensor([float("inf"), 0.0, 0.0])
    t = asw.actor_sweep_reference(**ac.arguments(c, xyz=xyz))
    assert t.counts.tolist()[3] == 2 and t.column[3] == -1 and t.column[7] == -1 and not bool(t.moved[3]) and not bool(t.moved[7])
    assert int(t.counts[0] + t.counts[1]) == 65
    xs, rs, _ = asw.actor_sweep(**ac.arguments(c, xyz=xyz))
    assert torch.equal(xs[[3, 7]].view(torch.int32), xyz[[3, 7]].view(torch.int32)) and torch.equal(rs[[3, 7]], c.rot[[3, 7]])


# ---- 5. gradients -------------------------------------------------------------------------------------------------------------------------------------------

def test_gradcheck_of_the_twin_with_the_columns_frozen():
    """xyz, rot_raw and actor_twist, at the case's twists and at eight times them.  The row whose |rot_raw| lies below F.normalize's eps gets an ordinary
    quaternion here: a finite difference of 1e-6 would carry it across the clamp (the host program and the device compare that row with the twin)."""
    for c in (ac.case(63, "mixed", 64), ac.case(65, "mixed", 64, "waymo_yaw", "ccw", actor_scale=8.0, check=False)):
        column = c.ref.column
        kw = ac.arguments(c)

        def fn(x, r, eta):
            t = asw.actor_sweep_reference(**{**kw, "xyz": x, "rot_raw": r, "actor_twist": eta}, column=column)
            return t.xyz_s, t.rot_s
        r = c.rot.double()
        r[r.norm(dim=1) < 1e-6] = torch.tensor([0.3, -0.5, 0.7, 0.2], dtype=torch.float64)
        x, r, eta = c.xyz.double().requires_grad_(True), r.requires_grad_(True), c.twist.double().requires_grad_(True)
        assert torch.autograd.gradcheck(fn, (x, r, eta), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_the_closed_forms_of_the_exponential_and_of_the_quaternion_agree_with_se3_exp():
    """Twists large enough for |s phi|^2 >= 0.25 (sw_coef's closed forms) and |s phi|^2 / 4 >= 0.25 (as_half_coef's)."""
    c = ac.case(65, "one", 64, check=False)
    eta = torch.tensor([[0.5, -1.0, 0.2, 0.3, -0.4, 3.1]])
    s = torch.linspace(-0.5, 0.5, 65, dtype=torch.float64)
    xs, rs, moved, parts = asw.place(c.xyz.double(), c.rot.double(), eta.double().expand(65, 6), s, torch.ones(65, dtype=torch.bool))
    u = (s[:, None] * eta.double()[:, 3:]).pow(2).sum(1)
    assert float(u.max()) / 4 >= sweep.SERIES_TH2 > float(u.min())
    for k in range(65):
        T = lrt_poses.se3_exp((s[k] * eta[0].double()))
        assert float((parts.Re[k] - T[:3, :3]).abs().max()) <= 1e-14 and float((parts.te[k] - T[:3, 3]).abs().max()) <= 1e-14
        w, x, y, z = parts.qe[k].tolist()
        Rq = torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                           [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=torch.float64)
        assert float((Rq - parts.Re[k]).abs().max()) <= 1e-14 and abs(w * w + x * x + y * y + z * z - 1.0) <= 1e-14


# ---- 6. twists from tracking boxes -----------------------------------------------------------------------------------------------------------------------------

def _track(frames, eta, start, rng):
    """A TrackingBox whose poses at `frames` follow A_{f'} = A_f Exp(eta (f' - f))."""
    tb = sequence.TrackingBox([4.0, 2.0, 1.5], "cpu")
    T = start.copy()
    prev = None
    for f in frames:
        if prev is not None:
            T = T @ lrt_poses.se3_exp(torch.tensor(eta * (f - prev))).numpy()
        q = _quat(T[:3, :3]) * rng.uniform(0.5, 2.0)
        tb.frame[f] = (torch.tensor(T[:3, 3]), torch.tensor(q).reshape(1, 4), None, None)
        prev = f
    return tb


def _quat(R):
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])


def test_actor_twists_from_boxes():
    rng = np.random.default_rng(2)
    eta = np.array([1.2, -0.3, 0.05, 0.01, -0.02, 0.2])
    start = np.eye(4)
    start[:3, :3] = lrt_poses.se3_exp(torch.tensor([0.0, 0.0, 0.0, 0.1, -0.2, 0.7], dtype=torch.float64)).numpy()[:3, :3]
    start[:3, 3] = [10.0, -4.0, 0.5]
    boxes = [_track([0, 1, 2, 4, 5], eta, start, rng), _track([2], eta, start, rng), _track([1, 4], eta, start, rng)]
    tw = asw.actor_twists_from_boxes(boxes, range(6))
    assert sorted(tw[0]) == [0, 1, 2, 4, 5] and sorted(tw[1]) == [2] and sorted(tw[2]) == [1, 4]
    for f, nxt in ((0, 1), (1, 2), (2, 4), (4, 5)):
        assert np.allclose(tw[0][f], eta, atol=1e-12, rtol=0)
        A0, A1 = asw.box_pose(boxes[0].frame[f]), asw.box_pose(boxes[0].frame[nxt])
        assert np.abs(A0 @ lrt_poses.se3_exp(torch.tensor(tw[0][f] * (nxt - f))).numpy() - A1).max() <= 1e-12
    assert np.array_equal(tw[0][5], tw[0][4])                                              # the last frame takes the previous interval's
    assert np.array_equal(tw[1][2], np.zeros(6))                                           # seen once
    assert np.allclose(tw[2][1], eta, atol=1e-12, rtol=0) and np.array_equal(tw[2][4], tw[2][1])
    half = asw.actor_twists_from_boxes({"car": boxes[0]}, range(6), sweep_fraction=0.5)
    assert list(half) == ["car"] and np.allclose(half["car"][2], 0.5 * eta, atol=1e-12, rtol=0)
    only = asw.actor_twists_from_boxes(boxes[:1], [0, 2, 5])                               # the frames asked for decide the neighbours
    assert sorted(only[0]) == [0, 2, 5] and np.allclose(only[0][2], eta, atol=1e-12, rtol=0)
    with pytest.raises(asw.ActorSweepError, match="sweep_fraction"):
        asw.actor_twists_from_boxes(boxes, range(6), sweep_fraction=0.0)


# ---- 7. the sequence format --------------------------------------------------------------------------------------------------------------------------------------

def _write(root, with_twist):
    H, W = 4, 16
    frames = [dict(id=f, depth=np.ones((H, W), np.float32), intensity=np.zeros((H, W), np.float32), mask=np.ones((H, W), bool), inclination=[-0.3, 0.1],
                   sensor2world=np.eye(4)) for f in (0, 1, 2)]
    tr = np.zeros((2, 3, 3), np.float32)
    tr[0, :, 0] = [10.0, 11.0, 12.0]
    tr[1, :, 1] = [5.0, 5.0, 5.0]
    qu = np.tile(np.array([1.0, 0, 0, 0], np.float32), (2, 3, 1))
    boxes = dict(frames=[0, 1, 2], translation=tr, quaternion=qu, size=np.ones((2, 3), np.float32), valid=np.array([[1, 1, 1], [1, 0, 1]], bool))
    if with_twist:
        boxes["twist"] = np.arange(36, dtype=np.float32).reshape(2, 3, 6) / 10.0
    sequence.write_sequence(root, frames, boxes=boxes)
    return boxes


def test_stored_actor_twists_round_trip_and_a_file_without_them_loads_as_before(tmp_path):
    a, b = str(tmp_path / "with"), str(tmp_path / "without")
    boxes = _write(a, True)
    _write(b, False)
    assert "twist" in np.load(os.path.join(a, "boxes.npz")).files and "twist" not in np.load(os.path.join(b, "boxes.npz")).files
    assert open(os.path.join(a, "meta.json")).read() == open(os.path.join(b, "meta.json")).read()      # the format string is unchanged
    for root in (a, b):
        for mode in (None, "off"):
            s = sequence.load_sequence(root, device="cpu", actor_sweep=mode)
            assert s.actor_sweep is None and all(tb.twist == {} for tb in s.boxes) and sorted(s.boxes[1].frame) == [0, 2]
    s = sequence.load_sequence(a, device="cpu", actor_sweep="stored")
    assert sorted(s.boxes[0].twist) == [0, 1, 2] and sorted(s.boxes[1].twist) == [0, 2]
    assert torch.equal(s.boxes[1].twist[2], torch.tensor(boxes["twist"][1, 2])) and s.boxes[0].twist[1].dtype == torch.float32
    with pytest.raises(ValueError, match="no stored actor twists"):
        sequence.load_sequence(b, device="cpu", actor_sweep="stored")
    with pytest.raises(ValueError, match="actor_sweep"):
        sequence.load_sequence(b, device="cpu", actor_sweep="poses")
    d = sequence.load_sequence(b, device="cpu", actor_sweep="boxes", sweep_fraction=0.5)
    assert torch.allclose(d.boxes[0].twist[0], torch.tensor([0.5, 0, 0, 0, 0, 0])) and torch.equal(d.boxes[0].twist[2], d.boxes[0].twist[1])
    assert torch.equal(d.boxes[1].twist[0], torch.zeros(6)) and sorted(d.boxes[1].twist) == [0, 2]


# ---- 8. the simulator's edits ---------------------------------------------------------------------------------------------------------------------------------------

def test_apply_edits_keeps_the_body_twists():
    """--move-actor multiplies on the world side, A' = M A, so A' Exp(s eta) = M A Exp(s eta): eta, a motion in the actor's own frame, is unchanged."""
    from types import SimpleNamespace
    from lidar_rt_amd import simulate
    boxes = []
    for a in range(3):
        tb = sequence.TrackingBox([4.0, 2.0, 1.5], "cpu")
        for f in (0, 1):
            tb.frame[f] = (torch.tensor([10.0 + a, f, 0.0]), torch.tensor([[1.0, 0.0, 0.0, 0.0]]), None, None)
            tb.twist[f] = torch.tensor([1.0 + a, 0.5 * f, 0.0, 0.0, 0.0, 0.1])
        boxes.append(tb)
    assets = [SimpleNamespace(bounding_box=None)] + [SimpleNamespace(bounding_box=tb) for tb in boxes]
    out, _, rep = simulate.apply_edits(assets, remove_actor=[1], move_actor=[[2, 1.0, -2.0, 0.5, 30.0], [2, 0.0, 1.0, 0.0, 0.0]])
    assert len(out) == 3 and out[1].bounding_box is boxes[0] and rep["removed"] == [1]
    moved = out[2].bounding_box
    assert moved is not boxes[2] and torch.equal(moved.frame[1][0], torch.tensor([13.0, 0.0, 0.5]))
    assert sorted(moved.twist) == [0, 1] and all(torch.equal(moved.twist[f], boxes[2].twist[f]) for f in (0, 1))
    assert torch.equal(boxes[2].frame[1][0], torch.tensor([12.0, 1.0, 0.0]))                        # the given box is not changed
    plain = sequence.TrackingBox([1.0, 1.0, 1.0], "cpu")                                           # a box-like object without twists still moves
    plain.frame[0] = boxes[0].frame[0]
    del plain.twist
    out, _, _ = simulate.apply_edits([assets[0], SimpleNamespace(bounding_box=plain)], move_actor=[[0, 1.0, 0.0, 0.0, 0.0]])
    assert out[1].bounding_box.twist == {}
