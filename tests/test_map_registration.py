"""Scan-to-map registration on the CPU: the cases' margins, the rule header compiled for the host against the numpy twin bit for bit (and once
under the address and undefined-behaviour sanitizers over hostile inputs), the twin's gradient against the analytic normal of a sphere, the edge
cases of the rule, tracking against the odometry chain, the library's build entry, exports, resource gate and refused arguments, and the
``ingest --map-tracking`` command line."""
import json
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

from lidar_rt_amd import ingest, map_registration as mr, mesh, registration as rg
from tests import map_registration_cases as mc
from tests import registration_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_check", "mapreg_check.cpp")


# ---- 1. the cases ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", mc.LINEARIZE_KEYS)
def test_every_case_keeps_its_margin(key):
    c = mc.case(key)
    for at, _ in mc.linearize_points(c):
        margin = mc.linearize_reference(key, at)[3]
        print(key, at, margin)
        assert margin >= mc.MARGIN or key == "last_centre", (key, at, margin)
    if key in mc.ALIGN_KEYS:
        assert mc.reference(key).margin >= mc.MARGIN, mc.reference(key).margin
    if key == "last_centre":
        assert mc.linearize_reference(key, "start")[3] == 0.0                  # the points ARE the boundary; X is the identity, so q is exact


def test_the_cases_cover_the_workgroup_shapes_and_the_exclusions():
    shapes = {(mc.case(k).H, mc.case(k).W) for k in mc.ROOM_KEYS}
    assert shapes == {(5, 37), (9, 61), (16, 128)}
    assert [-(-h * w // mr.BLOCK) for h, w in sorted(shapes)] == [1, 3, 8] and 5 * 37 < mr.BLOCK and (9 * 61) % mr.BLOCK != 0
    c = mc.case("holes")
    ts, wt = mr._grid_np(c.grid)
    p = c.src[0][0].numpy().reshape(-1, 3).astype(np.float64)
    cell, D, g, _ = mr.sample_reference(ts, wt, c.grid.voxel, 1, p)
    dims = np.array(c.grid.dims)
    cen_lo, cen_hi = 0.5 * c.grid.voxel, (dims - 0.5) * c.grid.voxel
    inside = np.all((p >= np.float32(cen_lo)) & (p <= mesh.centres(c.grid.voxel, 1)[0] + (dims - 1) * c.grid.voxel - 1e-3), 1)
    idx = np.clip(np.floor(p / c.grid.voxel - 0.5).astype(int), 0, dims - 2)
    unknown, ones = np.zeros(len(p), bool), np.ones(len(p), bool)
    for n in range(8):
        i, j, k = idx[:, 0] + (n & 1), idx[:, 1] + (n >> 1 & 1), idx[:, 2] + (n >> 2 & 1)
        unknown |= wt[i, j, k] < 1
        ones &= ts[i, j, k] == 1.0
    assert (inside & unknown).sum() >= 5 and (inside & ones & ~unknown).sum() >= 5 and (~inside).sum() >= 10
    assert np.all(cell[inside & (unknown | ones)] == -1) and (cell >= 0).sum() >= 100


# ---- 2. the rule header on the host ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mapreg_check") / "mapreg_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, SRC])
    return exe


def run_host(exe, tmp_path, c, X, hostile=False):
    F, HW = c.F, c.H * c.W
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as fh:
        fh.write(struct.pack("<8i", *c.grid.dims, F, c.H, c.W, 1, int(hostile)))
        fh.write(struct.pack("<3d", c.grid.voxel, c.grid.trunc, c.huber))
        for a in (X.numpy().astype(np.float64), c.grid.tsdf.numpy(), c.grid.weight.numpy(), c.src[0].numpy(), c.src[1].numpy().astype(np.uint8)):
            fh.write(np.ascontiguousarray(a).tobytes())
    res = subprocess.run([exe, inp, out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "MAPREGCHECK ok" in res.stdout, res.stdout + res.stderr
    raw = np.fromfile(out, np.uint8)
    n = F * HW
    cell = raw[:8 * n].view(np.int64)
    en = raw[8 * n:40 * n].view(np.float64).reshape(n, 4)
    terms = raw[40 * n:280 * n].view(np.float64).reshape(n, 30)
    inv = raw[280 * n:].view(np.float64).reshape(F, 3, 4)
    return cell, en, terms, inv, res


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


@pytest.mark.parametrize("key", mc.LINEARIZE_KEYS)
def test_the_rule_header_is_the_twin_bit_for_bit(host_check, tmp_path, key):
    c = mc.case(key)
    ts, wt = mr._grid_np(c.grid)
    for at, X in mc.linearize_points(c):
        cell, en, terms, inv, _ = run_host(host_check, tmp_path, c, X)
        HW = c.H * c.W
        for f in range(c.F):
            o = mr.pixels_reference(ts, wt, c.grid.voxel, c.grid.trunc, 1, X[f].numpy(), c.src[0][f].numpy(), c.src[1][f].numpy(), c.huber)
            sl = slice(f * HW, (f + 1) * HW)
            assert np.array_equal(cell[sl], o.cell.astype(np.int64)), (key, at, f, int((cell[sl] != o.cell).sum()))
            assert same_bits(en[sl, 0], o.e) and same_bits(en[sl, 1:], o.n), (key, at, f)
            assert same_bits(terms[sl], o.terms), (key, at, f)
            assert same_bits(inv[f], mr.inverse_reference(X[f].numpy()))
        assert np.array_equal(cell.reshape(c.F, c.H, c.W), mc.linearize_reference(key, at)[1].numpy())


def test_the_rule_header_under_the_sanitizers_survives_hostile_inputs(tmp_path):
    """A stand-alone program, never a Python process: NaN, infinite and huge points, points on and one ulp beside every face of the domain, a pose
    with a NaN, and grids of 0, 1 and 2 voxels along an axis whose arrays hold exactly the voxels their dims name."""
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = str(tmp_path / "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    linked = subprocess.run(["g++"] + flags + ["-o", str(tmp_path / "probe"), probe], capture_output=True, text=True)
    if linked.returncode != 0:
        pytest.skip("the sanitizer runtime does not link here: " + (linked.stderr.strip().splitlines() or ["g++ failed"])[-1])
    exe = str(tmp_path / "mapreg_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", exe, SRC])
    c = mc.case("holes")
    cell, _, _, _, res = run_host(exe, tmp_path, c, c.X_start, hostile=True)
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
    m = re.search(r"hostile: (\d+) samples, (\d+) with a term", res.stdout)
    assert m and int(m.group(1)) >= 9 * 3 * 17 ** 3 and int(m.group(2)) > 0, res.stdout       # the hostile passes did sample, and some samples landed
    assert np.array_equal(cell.reshape(1, c.H, c.W), mc.linearize_reference("holes", "start")[1].numpy())


# ---- 3. the rule ----------------------------------------------------------------------------------------------------------------------------------------

def test_the_gradient_on_the_sphere_is_the_analytic_normal_within_the_voxel_bound():
    """Measured: the largest |n - n_true| over the 549 pixels is 0.1275 (the bound, 3 h / (r - h sqrt(3)) with h = 0.25 and r = 1.2, is 0.978)."""
    n, true, bound, has, total = mc.sphere_normals()
    err = float(np.linalg.norm(n - true, axis=1).max())
    print("sphere: max |n - n_true|", err, "bound", bound)
    assert has == total == 9 * 61
    assert err <= bound
    assert err <= 1.5 * mc.RECORDED_SPHERE, err
    assert float(np.sum(n * true, 1).min()) > 0.9                             # and it points outwards, towards positive distance


def test_the_jacobian_is_the_central_difference_of_the_twins_own_residual():
    c = mc.case("room3_16x128_kitti_bounds")
    ts, wt = mr._grid_np(c.grid)
    X = c.X_true[0].numpy()
    args = (ts, wt, c.grid.voxel, c.grid.trunc, 1)
    o = mr.pixels_reference(*args, X, c.src[0][0].numpy(), c.src[1][0].numpy(), 1e9)
    has = np.nonzero(o.cell >= 0)[0]
    J = np.stack([o.terms[has, 21 + i] / o.e[has] for i in range(6)], 1)      # huber is off: terms[21 + i] = J_i e
    h = 1e-6
    worst = 0.0
    for i in range(6):
        d = np.zeros(6)
        d[i] = h
        es = []
        for s in (1.0, -1.0):
            Re, te = rg.exp_reference(s * d)
            Y = np.concatenate([X[:, :3] @ Re, (X[:, :3] @ te + X[:, 3])[:, None]], 1)
            es.append(mr.pixels_reference(*args, Y, c.src[0][0].numpy(), c.src[1][0].numpy(), 1e9))
        same = (es[0].cell[has] == o.cell[has]) & (es[1].cell[has] == o.cell[has])          # the trilinear patch is smooth inside one cell only
        num = (es[0].e[has] - es[1].e[has]) / (2 * h)
        worst = max(worst, float(np.abs(num - J[:, i])[same].max()))
        assert same.sum() > 0.9 * has.size
    print("jacobian against the central difference:", worst)
    assert worst <= 1e-6                                                        # second order in h = 1e-6 on values of order 1, plus 2^-53 / h


def test_the_edges_of_the_rule():
    # a point exactly on the last voxel centre: cell n - 2, fraction 1 -- the value is the far corner's
    c = mc.case("last_centre")
    X, Y, Z = c.grid.dims
    ts, wt = mr._grid_np(c.grid)
    o = mr.pixels_reference(ts, wt, c.grid.voxel, c.grid.trunc, 1, c.X_start[0].numpy(), c.src[0][0].numpy(), c.src[1][0].numpy(), c.huber)
    for k in range(8):
        want = [(n - 2) if (k >> a) & 1 else 1 for a, n in enumerate((X, Y, Z))]
        assert o.cell[k] == (want[0] * Y + want[1]) * Z + want[2], (k, o.cell[k], want)
    assert o.e[7] == c.grid.trunc * float(ts[X - 1, Y - 1, Z - 1])             # all three fractions are 1: D is corner 7 exactly
    # an axis of 2 voxels has a domain (one cell thick), an axis of 1 voxel has none
    assert int(mc.linearize_reference("thin2", "start")[0][0, 29]) > 100
    assert np.all(mc.linearize_reference("thin2", "start")[1].numpy() % 2 == np.where(mc.linearize_reference("thin2", "start")[1].numpy() >= 0, 0, 1))
    s, cell, _, _ = mc.linearize_reference("thin1", "start")
    assert np.all(s.numpy() == 0.0) and np.all(cell.numpy() == -1)
    r = mc.reference("thin1")
    assert r.status.tolist() == [rg.FEW] and np.array_equal(r.X.numpy().view(np.uint64), mc.case("thin1").X_start.numpy().view(np.uint64))
    assert np.all(r.log[0, :, 5].numpy() == rg.FEW) and np.all(r.log[0, :, 3:5].numpy() == 0.0)
    # F = 3: an empty mask and a frame wholly outside the grid are FEW and keep their start; the first frame does not care
    b, one = mc.reference("batch3"), mc.reference("room3_16x128_kitti_bounds")
    c = mc.case("batch3")
    assert b.status.tolist()[1:] == [rg.FEW, rg.FEW] and b.status[0] == one.status[0]
    assert np.array_equal(b.X[1:].numpy().view(np.uint64), c.X_start[1:].numpy().view(np.uint64))
    assert np.array_equal(b.X[0].numpy().view(np.uint64), one.X[0].numpy().view(np.uint64))
    for f in range(3):
        assert np.abs(b.G[f].numpy() @ np.vstack([b.X[f].numpy(), [0, 0, 0, 1]]) - np.eye(4)[:3]).max() <= 1e-12 * max(1.0, float(np.abs(b.X[f].numpy()[:, 3]).max()))


@pytest.mark.parametrize("key", mc.ROOM_KEYS)
def test_the_twin_moves_towards_the_truth_as_recorded(key):
    c, r = mc.case(key), mc.reference(key)
    et, er = rc.pose_error(r.X[0].numpy(), c.X_true[0].numpy())
    e0 = rc.pose_error(c.X_start[0].numpy(), c.X_true[0].numpy())
    cond = float(np.linalg.cond(r.hessian[0].numpy()))
    print(key, et, er, cond, "from", e0)
    _, rt, rr = mc.RECORDED[key][0], mc.RECORDED[key][1], mc.RECORDED[key][2]
    assert et <= 1.5 * rt and er <= 1.5 * rr, (key, et, er)
    assert cond <= 1.5 * mc.RECORDED[key][0] and cond >= mc.RECORDED[key][0] / 1.5
    assert r.status[0] in (rg.OK, rg.CONVERGED) and np.array_equal(r.hessian[0].numpy(), r.hessian[0].numpy().T)


def test_the_python_side_refuses_before_it_computes():
    c = mc.case("thin2")
    with pytest.raises(mr.MapRegistrationError, match="TsdfGrid"):
        mr.align_to_grid(None, c.src, c.X_start)
    with pytest.raises(mr.MapRegistrationError, match="iterations"):
        mr.align_to_grid(c.grid, c.src, c.X_start, iters=33)
    with pytest.raises(mr.MapRegistrationError, match="min_weight"):
        mr.linearize_to_grid(c.grid, c.src, c.X_start, min_weight=0)
    with pytest.raises(mr.MapRegistrationError, match="huber"):
        mr.linearize_to_grid(c.grid, c.src, c.X_start, huber=0.0)
    with pytest.raises(mr.MapRegistrationError, match="float64"):
        mr.align_to_grid(c.grid, c.src, torch.eye(4)[None])
    with pytest.raises(mr.MapRegistrationError, match="workspace"):
        mr.align_to_grid(c.grid, c.src, c.X_start, workspace=torch.zeros(1 << 12, dtype=torch.uint8))
    with pytest.raises(mr.MapRegistrationError, match="no image"):
        mr.track_and_fuse(c.grid, {0: (c.src[0][0], c.src[1][0])}, {}, inclination=[-0.4, 0.1])
    sums, cell = mr.linearize_to_grid(c.grid, (c.src[0][0], c.src[1][0]), c.X_start[0])       # CPU tensors go to the twin; no frame axis in, none out
    assert sums.shape == (30,) and cell.shape == (c.H, c.W) and torch.equal(sums, mc.linearize_reference("thin2", "start")[0][0])


# ---- 4. tracking ----------------------------------------------------------------------------------------------------------------------------------------

def test_map_tracking_ends_nearer_the_truth_than_the_odometry_chain():
    """Twelve frames of 32 x 256, voxel 0.2 m, trunc 0.8 m, through the twins.  Measured for the last frame: map tracking 7.04 mm and 0.47 mrad,
    the odometry chain 29.1 mm and 4.62 mrad."""
    T = mc.tracking()
    (mt, mrot), (ct, crot) = T.map_error, T.chain_error
    print("map tracking", mt, mrot, "chain", ct, crot)
    for i in sorted(T.truth):
        print(i, "chain %.3e %.3e" % rc.pose_error(T.chain[i][:3], T.truth[i][:3]), "map %.3e %.3e" % rc.pose_error(T.tracked[i][:3], T.truth[i][:3]))
    assert mt < ct and mrot < crot
    rt, rr, rct, rcr = mc.RECORDED_TRACKING
    assert mt <= 1.5 * rt and mrot <= 1.5 * rr, (mt, mrot)
    assert rct / 1.5 <= ct <= 1.5 * rct and rcr / 1.5 <= crot <= 1.5 * rcr, (ct, crot)
    rep = T.report
    assert rep["failed"] == [] and rep["frames"][0] == {"id": 0, "status": None, "terms": None, "cond": None}
    assert all(r["status"] in (rg.OK, rg.CONVERGED) and r["terms"] > 5000 for r in rep["frames"][1:])
    assert np.array_equal(T.tracked[0], T.truth[0]) and int((T.grid.weight > 0).sum()) > 10000


def test_a_frame_that_cannot_be_tracked_keeps_its_start_and_is_fused_there():
    frames, images, truth, kw = mc.trajectory(3, 16, 128)
    steps = {i: np.linalg.inv(truth[i - 1]) @ truth[i] for i in (1, 2)}
    chain = {i: truth[i] for i in truth}
    broken = dict(frames)
    broken[1] = (frames[1][0], torch.zeros_like(frames[1][2]))             # no source pixel: FEW
    grid = mc.tracking_grid(frames, chain, 0.4, 1.2)
    est, rep = mr.track_and_fuse(grid, broken, images, steps=steps, **kw)
    assert rep["failed"] == [1] and rep["frames"][1]["status"] == rg.FEW and rep["frames"][2]["status"] in (rg.OK, rg.CONVERGED)
    assert np.abs(est[1] - truth[0] @ steps[1]).max() <= 1e-12                 # the start pose, through the grid frame and back
    assert int(grid.weight.max()) == 3                                          # and its image was fused all the same
    # without steps: constant velocity, the last step found once more
    grid2 = mc.tracking_grid(frames, chain, 0.4, 1.2)
    est2, rep2 = mr.track_and_fuse(grid2, frames, images, **kw)
    assert rep2["failed"] == [] and rc.pose_error(est2[2][:3], truth[2][:3])[0] < 0.1


# ---- 5. the library: its build entry, exports and resource gate, refused arguments -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def mapreg_lib():
    from lidar_rt_amd import build as lrt_build
    return lrt_build.build_mapreg()


def test_the_library_builds_and_exports_what_its_header_declares(mapreg_lib):
    from lidar_rt_amd import build as lrt_build
    assert os.path.exists(mapreg_lib) and not lrt_build.mapreg_is_stale()
    assert lrt_build.MAPREG_SOURCES == ["lrt_mapreg.hip"]
    assert {"lrt_mapreg_math.h", "lrt_raycast_math.h", "lrt_project_math.h", "lrt_sweep_math.h"} <= set(lrt_build.MAPREG_HEADERS)
    assert lrt_build.MAPREG_BORROWED == ["lrt_reg_math.h"]                     # hashed with the library, listed with liblrt_reg.so's files only
    before = lrt_build.mapreg_source_hash()
    try:
        lrt_build.MAPREG_BORROWED = []
        assert lrt_build.mapreg_source_hash() != before
    finally:
        lrt_build.MAPREG_BORROWED = ["lrt_reg_math.h"]
    assert "lrt_mapreg" not in " ".join(lrt_build.REG_SOURCES + lrt_build.REG_HEADERS + lrt_build.RAYCAST_SOURCES + lrt_build.RAYCAST_HEADERS
                                        + lrt_build.MESH_SOURCES + lrt_build.MESH_HEADERS)
    src = open(lrt_build.__file__).read()
    assert "build_mapreg(force, verbose)" in src[src.index("def _build_product"):src.index("def _build_lib")]
    assert "csrc/liblrt_mapreg.so" in open(os.path.join(REPO, "setup.py")).read()
    text = open(os.path.join(REPO, "lidar_rt_amd", "csrc", "lrt_mapreg_math.h")).read()
    for inc in ("lrt_raycast_math.h", "lrt_reg_math.h", "lrt_project_math.h"):
        assert f'#include "{inc}"' in text
    hdr = open(os.path.join(REPO, "include", "lrt_mapreg.h")).read()
    declared = set(re.findall(r"\b(lrt_mapreg_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(mr.EXPORTS), declared ^ set(mr.EXPORTS)
    exported = set(re.findall(r"\blrt_mapreg_[a-z_]+\b", subprocess.run(["nm", "-D", "--defined-only", mapreg_lib], capture_output=True, text=True, check=True).stdout))
    assert exported == declared, exported ^ declared
    lib = mr.load()
    assert lib.lrt_mapreg_abi_version() == int(re.search(r"#define\s+LRT_MAPREG_ABI_VERSION\s+(\d+)", hdr).group(1)) == mr.ABI_VERSION
    for name, val in (("BLOCK", mr.BLOCK), ("NSUM", mr.NSUM), ("NLOG", mr.NLOG), ("MAX_ITER", mr.MAX_ITER), ("MAX_FRAMES", mr.MAX_FRAMES), ("MAX_PIXELS", mr.MAX_PIXELS)):
        assert int(re.search(rf"#define\s+LRT_MAPREG_{name}\s+(\d+)", hdr).group(1)) == val, name
    assert (mr.BLOCK, mr.NSUM, mr.NLOG, mr.MAX_ITER) == (rg.BLOCK, rg.NSUM, rg.NLOG, rg.MAX_ITER)
    assert lib.lrt_mapreg_work_bytes(0, 8, 8) < 0 and lib.lrt_mapreg_work_bytes(1, 0, 8) < 0 and lib.lrt_mapreg_work_bytes(65536, 8, 8) < 0
    assert lib.lrt_mapreg_work_bytes(1, 5, 37) == 256 and lib.lrt_mapreg_work_bytes(3, 9, 61) == 2304 and mr.work_bytes(16, 64, 2048) == -(-8 * (30 * 16 * 512 + 16) // 256) * 256 == 1966336


def test_the_kernels_pass_the_resource_gate(mapreg_lib):
    from lidar_rt_amd import resources
    res = resources.kernel_resources(mapreg_lib)
    own = sorted(n for n in res if resources.is_own_kernel(n))
    assert own == ["k_mapreg_linearize", "k_mapreg_solve"], own
    assert all(any(re.search(g_, n) for g_ in resources.GATED) for n in own)
    assert resources.violations(res) == []
    assert all(res[n]["vgpr_spill"] == 0 and res[n]["scratch_bytes"] == 0 for n in own)


LIN_ARGS = ("device", "X", "Y", "Z", "voxel", "trunc", "tsdf", "weight", "min_weight", "F", "H", "W", "sp", "sm", "pose", "huber", "sums", "cell", "workspace",
            "work_bytes", "stream")
ALIGN_ARGS = ("device", "X", "Y", "Z", "voxel", "trunc", "tsdf", "weight", "min_weight", "F", "H", "W", "sp", "sm", "X_init", "K", "huber", "lam", "min_pairs",
              "tol_t", "tol_r", "X_out", "G_out", "log", "hessian", "status", "workspace", "work_bytes", "stream")


def test_argument_errors_come_before_the_device_and_launch_nothing(mapreg_lib):
    """Non-null dummy pointers and device 99: a refused argument is reported first; valid arguments reach the device check, which refuses too."""
    lib = mr.load()
    ok = dict(device=99, X=3, Y=3, Z=3, voxel=0.1, trunc=0.3, tsdf=8, weight=8, min_weight=1, F=1, H=4, W=8, sp=8, sm=8, pose=8, huber=0.1, sums=8, cell=None,
              workspace=256, work_bytes=256, stream=None, X_init=8, K=4, lam=1e-6, min_pairs=10, tol_t=1e-5, tol_r=1e-6, X_out=8, G_out=8, log=8, hessian=8, status=8)
    lin = lambda **kw: lib.lrt_mapreg_linearize(*[dict(ok, **kw)[k] for k in LIN_ARGS])
    ali = lambda **kw: lib.lrt_mapreg_align(*[dict(ok, **kw)[k] for k in ALIGN_ARGS])
    common = (({"X": 0}, "a grid of 0 x"), ({"X": 65536, "Y": 65536}, "a grid of 65536 x"), ({"voxel": 0.0}, "voxel 0"), ({"trunc": -1.0}, "trunc -1"),
              ({"min_weight": 0}, "min_weight 0"), ({"tsdf": None}, "null tsdf"), ({"F": 0}, "0 frames"), ({"F": mr.MAX_FRAMES + 1}, "65536 frames"),
              ({"H": 0}, "1 frames of 0 x 8"), ({"sm": None}, "null src_points"), ({"huber": 0.0}, "huber 0"), ({"huber": float("nan")}, "huber nan"),
              ({"workspace": None}, "256-byte aligned"), ({"workspace": 264}, "256-byte aligned"), ({"work_bytes": 255}, "a workspace of 255 bytes"),
              ({}, "no HIP device 99"))
    for call in (lin, ali):
        for kw, msg in common:
            assert call(**kw) == -1, kw
            assert msg in lib.lrt_mapreg_last_error().decode(), (kw, lib.lrt_mapreg_last_error())
    for kw, msg in (({"pose": None}, "null pose"), ({"sums": None}, "null pose / sums")):
        assert lin(**kw) == -1 and msg in lib.lrt_mapreg_last_error().decode(), kw
    for kw, msg in (({"K": 0}, "0 iterations"), ({"K": 33}, "33 iterations"), ({"lam": -1.0}, "lambda -1"), ({"min_pairs": 0}, "min_pairs 0"),
                    ({"tol_t": -1.0}, "tolerances"), ({"G_out": None}, "null X_init"), ({"status": None}, "null X_init")):
        assert ali(**kw) == -1 and msg in lib.lrt_mapreg_last_error().decode(), (kw, lib.lrt_mapreg_last_error())


# ---- 6. the command line ----------------------------------------------------------------------------------------------------------------------------------

def _write_clouds(folder, frames):
    os.makedirs(folder, exist_ok=True)
    for i, g in frames.items():
        p = g[0][g[-1]].numpy()
        np.save(os.path.join(folder, f"{i}.npy"), np.concatenate([p, np.full((p.shape[0], 1), 0.5, np.float32)], 1))


COMMON = ["--height", "16", "--width", "128", "--inclination", "-0.43", "0.12", "--device", "cpu", "--max-depth", "80"]


def _members(root):
    out = {}
    for d, _, files in os.walk(root):
        for fn in sorted(files):
            path = os.path.join(d, fn)
            rel = os.path.relpath(path, root)
            if fn.endswith(".npz"):
                z = np.load(path)
                out[rel] = {k: (str(z[k].dtype), z[k].shape, z[k].tobytes()) for k in z.files}
            else:
                out[rel] = open(path, "rb").read()
    return out


@pytest.fixture(scope="module")
def clouds(tmp_path_factory):
    frames, images, truth, kw = mc.trajectory(4, 16, 128)
    pts = str(tmp_path_factory.mktemp("clouds") / "pts")
    _write_clouds(pts, frames)
    return pts, frames, truth


def test_ingest_refuses_map_tracking_without_odometry_and_with_loop_closure(clouds, tmp_path, capsys):
    pts, frames, truth = clouds
    np.save(tmp_path / "poses.npy", np.stack([truth[i] for i in sorted(truth)]))
    out = str(tmp_path / "out")
    assert ingest.main(["--points", pts, "--out", out, "--poses", str(tmp_path / "poses.npy"), "--map-tracking"] + COMMON) == 2
    assert "--map-tracking goes with --odometry" in capsys.readouterr().err
    assert ingest.main(["--points", pts, "--out", out, "--odometry", "--map-tracking", "--loop-closure", "--sensor-height", "1.8"] + COMMON) == 2
    assert "--map-tracking does not go with --loop-closure" in capsys.readouterr().err
    assert not os.path.exists(out)
    with pytest.raises(ValueError, match="map_tracking does not go with loop_closure"):
        ingest.ingest_point_clouds(out, ((i, ingest.read_points(p), None) for i, p in ingest.list_points(pts)), 16, 128, [-0.43, 0.12], device="cpu",
                                   odometry={"map_tracking": {}, "loop_closure": {"sensor_height": 1.8}})


def test_ingest_with_map_tracking_writes_the_tracked_poses_and_without_it_the_same_bytes(clouds, tmp_path, capsys):
    """Four frames of 16 x 128 (coarser than map tracking wants: this checks the plumbing, not the accuracy), --map-voxel 0.4."""
    pts, frames, truth = clouds
    out, plain, direct = str(tmp_path / "tracked"), str(tmp_path / "plain"), str(tmp_path / "direct")
    assert ingest.main(["--points", pts, "--out", out, "--odometry", "--map-tracking", "--map-voxel", "0.4", "--map-trunc", "1.2"] + COMMON) == 0
    assert "map tracking moved the chain by up to" in capsys.readouterr().out
    rep = json.load(open(os.path.join(out, "ingest.json")))
    mt = rep["map_tracking"]
    assert mt["voxel"] == 0.4 and mt["trunc"] == 1.2 and mt["failed"] == [] and [r["id"] for r in mt["frames"]] == [0, 1, 2, 3] and mt["observed_voxels"] > 1000
    assert mt["frames"][0]["status"] is None and all(r["status"] in (rg.OK, rg.CONVERGED) for r in mt["frames"][1:])
    assert len(rep["odometry"]["pairs"]) == 3 and "map_tracking" not in rep["odometry"]
    # the written poses are the tracked ones: what track_and_fuse gives from the chain's steps on the same grid
    chain, orep = rg.odometry(frames, inclination=[-0.43, 0.12], return_steps=True)
    from lidar_rt_amd import sequence
    got = {i: np.load(sequence._frame_path(out, i))["sensor2world"].astype(np.float64) for i in sorted(frames)}
    assert mt["largest_correction"] > 0.0
    for i in sorted(frames):
        et, _ = rc.pose_error(got[i][:3], truth[i][:3])
        assert et < 0.05, (i, et)
    moved = max(float(np.linalg.norm(got[i][:3, 3] - chain[i][:3, 3])) for i in got)
    assert abs(moved - mt["largest_correction"]) <= 1e-5                        # float32 storage of the poses
    # off by default: --odometry alone writes what the call without the key writes, byte for byte
    assert ingest.main(["--points", pts, "--out", plain, "--odometry"] + COMMON) == 0
    ingest.ingest_point_clouds(direct, ((i, ingest.read_points(p), None) for i, p in ingest.list_points(pts)), 16, 128, [-0.43, 0.12], data_type="KITTI",
                               sensor2ego=None, max_depth=80.0, test_frames=[], device="cpu", batch=16, wrap=True, notes={"pose_taken_from": {}}, twists=None,
                               odometry={})
    ma, mb = _members(plain), _members(direct)
    assert sorted(ma) == sorted(mb) and "map_tracking" not in json.loads(ma["ingest.json"])
    for rel in ma:
        assert ma[rel] == mb[rel], rel
