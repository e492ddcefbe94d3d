"""Scan registration without a GPU: the twin's Jacobian and Exp, truth recovery in the analytic room, the rule's header compiled for the host
against the twin, the fifteenth product library (`liblrt_reg.so`), the odometry chain, and `ingest --odometry` on the CPU path."""
import ctypes as C
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

from lidar_rt_amd import build as lrt_build, ingest, poses, registration as rg, resources
from tests import registration_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
U = 2.0 ** -53


# ---- 1. the Jacobian and Exp ----------------------------------------------------------------------------------------------------------------------------------

def test_the_jacobian_is_the_central_difference_of_the_twins_own_residual():
    rng = np.random.default_rng(0)
    N = 40
    p, qt = rng.normal(0, 5, (N, 3)), rng.normal(0, 5, (N, 3))
    n = rng.normal(size=(N, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    X = rc.exp4(np.array([0.4, -1.0, 0.3, 0.2, -0.5, 0.9]))[:3]
    _, J = rg.residuals_reference(p, X, qt, n)
    h = 1e-6
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        ep, _ = rg.residuals_reference(p, (np.vstack([X, [0, 0, 0, 1]]) @ rc.exp4(d))[:3], qt, n)       # the right perturbation X Exp(delta)
        em, _ = rg.residuals_reference(p, (np.vstack([X, [0, 0, 0, 1]]) @ rc.exp4(-d))[:3], qt, n)
        assert np.abs((ep - em) / (2 * h) - J[:, k]).max() <= 1e-8 * max(1.0, np.abs(J[:, k]).max()), k


@pytest.mark.parametrize("xi", [[0.3, -0.2, 0.1, 0.0, 0.0, 0.0], [1.0, 2.0, -0.5, 0.01, -0.02, 0.03], [0.2, 0.1, 0.0, 0.3, -0.2, 0.35], [-1.0, 0.4, 0.2, 1.1, -0.7, 2.0]])
def test_exp_is_se3_exp(xi):
    Re, te = rg.exp_reference(xi)
    T = poses.se3_exp(torch.tensor(xi, dtype=torch.float64)).numpy()
    assert np.abs(Re - T[:3, :3]).max() <= 1e-14 and np.abs(te - T[:3, 3]).max() <= 1e-14 * max(1.0, np.abs(te).max())


# ---- 2. truth recovery ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", rc.KEYS)
def test_the_twin_recovers_the_truth(key):
    """From the identity, i.e. from the case's whole offset.  The bound is twice what the committed twin reached when the case was recorded
    (tests/registration_cases.py RECORDED), the remainder being partners across the room's creases and the estimated normals.  On the room cases
    the translation error is also under 1 % of the initial translation offset (recorded: 0.63 %, 0.24 %, 0.08 %).  The rotation error is not held
    to 1 % of the 2 to 4 degrees: the recorded 3.4e-4 to 8.3e-4 rad are 0.5 to 2.4 % of them, as the 4.9e-4 to 8.3e-4 rad of the numpy prototype
    this rule was drafted with were."""
    c, r = rc.case(key), rc.reference(key)
    assert int(r.status[0]) == rg.CONVERGED
    et, er = rc.pose_error(r.X[0].numpy(), c.X_true[0].numpy())
    t0, r0, _ = rc.RECORDED[key]
    print(key, et, er)
    assert et <= 2.0 * t0 and er <= 2.0 * r0, (et, er)
    if key in rc.ROOM_KEYS:
        assert float(np.linalg.norm(c.xi[0, :3])) == pytest.approx(rc.ROOM_OFFSETS[key][0]) and float(np.linalg.norm(c.xi[0, 3:])) == pytest.approx(np.radians(rc.ROOM_OFFSETS[key][1]))
        assert et < 0.01 * rc.ROOM_OFFSETS[key][0], et
    assert np.linalg.cond(r.hessian[0].numpy()) == pytest.approx(rc.RECORDED[key][2], rel=1e-2)


def test_status_log_and_frozen_poses_of_the_twin():
    c, r = rc.case("batch3"), rc.reference("batch3")
    assert r.status.tolist() == [rg.CONVERGED, rg.FEW, rg.FEW]
    eye = torch.eye(4, dtype=torch.float64)[:3]
    assert torch.equal(r.X[1], eye) and torch.equal(r.X[2], eye)                            # status 1: the start's bits
    assert not r.log[1, :, 0].any() and r.log[1, :, 5].eq(1).all() and not r.log[:, :, 6:].any()
    first = int((r.log[0, :, 5] == 3).nonzero()[0])                                          # the converging iteration and all after it: the same X
    short = rg.align_reference(c.src, c.tgt, None, c.schedule[:first], min_pairs=c.min_pairs, **c.kw)
    assert torch.equal(short.X[0], r.X[0]) and int(short.status[0]) == rg.OK
    assert float(r.log[0, first, 3]) < 1e-5 and float(r.log[0, first, 4]) < 1e-6 and not r.log[0, first + 1:, 3:5].any()
    tn = c.tgt[1].clone()
    tn[2] = float("nan")                                                                    # a system that is not a number: status 2 at the first pivot
    bad = rg.align_reference(c.src, (c.tgt[0], tn, c.tgt[2]), None, c.schedule[:2], min_pairs=c.min_pairs, **c.kw)
    assert bad.status.tolist() == [rg.OK, rg.FEW, rg.PIVOT] and torch.equal(bad.X[2], eye)
    one = rg.align_reference(tuple(t[0] for t in c.src), tuple(t[0] for t in c.tgt), None, c.schedule, min_pairs=c.min_pairs, **c.kw)     # without a pair axis
    assert one.X.shape == (3, 4) and torch.equal(one.X, r.X[0]) and torch.equal(one.log, r.log[0]) and one.status.shape == ()


def test_ties_go_to_the_lower_pixel_and_masked_pixels_have_no_partner():
    c = rc.case("tie")
    sums, assoc = rg.linearize(c.src, c.tgt, c.X_true, 1, 2, 5.0, **c.kw)                    # CPU tensors: the twin
    a = assoc[0].reshape(-1)
    lo, hi = 2 * c.W + 10, 2 * c.W + 11
    assert int((a == lo).sum()) >= 1 and int((a == hi).sum()) == 0                          # the doubled point is only ever reached through its lower pixel
    assert int(sums[0, 29]) == int((a >= 0).sum())
    sm = c.src[2].clone()
    sm[0, 1] = False
    _, a2 = rg.linearize((c.src[0], sm), c.tgt, c.X_true, 1, 2, 5.0, **c.kw)
    assert bool((a2[0, 1] == -1).all()) and torch.equal(a2[0, 0], assoc[0, 0])


# ---- 3. the rule's header on the host ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("reg_check") / "reg_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "host_check", "reg_check.cpp")])
    return exe


def run_host(exe, c, f, X, rh, rw, max_dist, tmp_path, huber=0.1, lam=1e-6, min_pairs=20.0, tol_t=1e-5, tol_r=1e-6):
    inc, off, yaw, lo, hi = rg._model(c.H, c.W, c.kw["inclination"], c.kw["data_type"], c.kw["sensor2ego"], 0.0, rg.FLT_MAX)
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as fh:
        fh.write(struct.pack("<8i", c.H, c.W, inc.size, rh, rw, 0, 0, 0))
        fh.write(struct.pack("<10d", off, yaw, lo, hi, max_dist, huber, lam, min_pairs, tol_t, tol_r))
        fh.write(inc.tobytes()); fh.write(np.ascontiguousarray(X, np.float64).tobytes())
        fh.write(c.src[0][f].numpy().tobytes()); fh.write(c.src[2][f].numpy().astype(np.uint8).tobytes())
        fh.write(c.tgt[0][f].numpy().tobytes()); fh.write(c.tgt[1][f].numpy().tobytes()); fh.write(c.tgt[2][f].numpy().astype(np.uint8).tobytes())
    res = subprocess.run([exe, inp, out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "REGCHECK ok" in res.stdout, res.stdout + res.stderr
    raw = open(out, "rb").read()
    HW = c.H * c.W
    assoc = np.frombuffer(raw, np.int32, HW)
    sums = np.frombuffer(raw, np.float64, rg.NSUM, 4 * HW)
    status = int(np.frombuffer(raw, np.int32, 1, 4 * HW + 8 * rg.NSUM)[0])
    rest = np.frombuffer(raw, np.float64, 14, 4 * HW + 8 * rg.NSUM + 8)
    return assoc, sums, status, rest[:12].reshape(3, 4), rest[12:]


@pytest.mark.parametrize("key", rc.KEYS)
def test_the_rule_header_on_the_host_against_the_twin(host_check, key, tmp_path):
    """assoc equal on every pixel; every sum within N 2^-53 sum |term| of the twin's (N the valid source pixels: both add the same terms, in
    different orders); and one solve step within 1e-12 of the twin's."""
    c = rc.case(key)
    rh, rw, md = (4, 16, 3.0) if key == "wide" else (int(c.schedule[0][0]), int(c.schedule[0][1]), float(c.schedule[0][2]))
    for name, X in rc.linearize_points(c):
        sums, assoc, ab = rg.linearize_reference(c.src, c.tgt, X, rh, rw, md, return_abs=True, **c.kw)
        for f in range(c.F):
            h_assoc, h_sums, h_st, h_X, h_norms = run_host(host_check, c, f, X[f].numpy(), rh, rw, md, tmp_path)
            assert np.array_equal(h_assoc, assoc[f].numpy().reshape(-1)), (key, name, f)
            assert np.all(np.abs(h_sums - sums[f].numpy()) <= max(c.n_valid[f], 1) * U * ab[f].numpy()), (key, name, f)
            assert h_sums[29] == float((h_assoc >= 0).sum())
            st, Xn, nr, nf = rg.solve_reference(sums[f].numpy(), 1e-6, 20.0, 1e-5, 1e-6, X[f].numpy())
            assert h_st == st and np.abs(h_X - Xn).max() <= 1e-12 * max(1.0, np.abs(Xn).max()) and abs(h_norms[0] - nr) <= 1e-12 and abs(h_norms[1] - nf) <= 1e-12


# ---- 4. the library ------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def reg_lib():
    return lrt_build.build_reg()


def test_the_library_has_a_source_list_of_its_own_and_leaves_the_borrowed_headers_alone():
    assert lrt_build.REG_SOURCES == ["lrt_reg.hip"]
    assert {os.path.basename(h) for h in lrt_build.REG_HEADERS} == {"lrt_reg_math.h", "lrt_project_math.h", "lrt_sweep_math.h", "lrt_device_guard.h", "lrt_reg.h"}
    others = [getattr(lrt_build, n) for n in dir(lrt_build) if n.endswith(("SOURCES", "HEADERS")) and not n.startswith("REG_")]
    assert len(others) >= 28 and not any("lrt_reg" in f for lst in others for f in lst)
    assert os.path.basename(lrt_build.REG_LIB) == "liblrt_reg.so" and os.path.basename(lrt_build.REG_STAMP) == "liblrt_reg.srchash"
    assert re.fullmatch(r"[0-9a-f]{16}", lrt_build.reg_source_hash())
    src = open(lrt_build.__file__).read()
    assert "build_reg(force, verbose)" in src[src.index("def _build_product"):src.index("def _build_lib")]
    assert "csrc/liblrt_reg.so" in open(os.path.join(REPO, "setup.py")).read()
    body = src[src.index("def build_reg"):src.index("EXT_SRC =")]
    assert "CODEGEN_FLAGS" in body and "resources.check(REG_LIB)" in body
    mh = open(os.path.join(REPO, "lidar_rt_amd", "csrc", "lrt_reg_math.h")).read()
    assert '#include "lrt_project_math.h"' in mh and '#include "lrt_sweep_math.h"' in mh
    # the two borrowed rule headers are byte for byte what they were before this library read them
    import hashlib
    for hdr, want in (("lrt_project_math.h", "cf3f97d820b9cdb3acd5c41202d19c9938c3057a72a5e7f8a23bb06e350d7b0c"),
                      ("lrt_sweep_math.h", "143796d2b4c11a794fdc7911f614fbc2561cb884c07e521b335c67f6466f52a1")):
        assert hashlib.sha256(open(os.path.join(REPO, "lidar_rt_amd", "csrc", hdr), "rb").read()).hexdigest() == want, hdr


def test_the_library_builds_and_exports_what_its_header_declares(reg_lib):
    assert os.path.exists(reg_lib) and not lrt_build.reg_is_stale()
    hdr = open(os.path.join(REPO, "include", "lrt_reg.h")).read()
    declared = set(re.findall(r"\b(lrt_reg_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(rg.EXPORTS), declared ^ set(rg.EXPORTS)
    lib = rg.load()
    exported = set(re.findall(r"\blrt_reg_[a-z_]+\b", subprocess.run(["nm", "-D", "--defined-only", reg_lib], capture_output=True, text=True, check=True).stdout))
    assert exported == declared, exported ^ declared
    assert lib.lrt_reg_abi_version() == int(re.search(r"#define\s+LRT_REG_ABI_VERSION\s+(\d+)", hdr).group(1)) == rg.ABI_VERSION
    for name, val in (("BLOCK", rg.BLOCK), ("NSUM", rg.NSUM), ("NLOG", rg.NLOG), ("MAX_ITER", rg.MAX_ITER), ("MAX_RH", rg.MAX_RH), ("MAX_RW", rg.MAX_RW),
                      ("MAX_PAIRS", rg.MAX_PAIRS), ("MAX_PIXELS", rg.MAX_PIXELS)):
        assert int(re.search(rf"#define\s+LRT_REG_{name}\s+(\d+)", hdr).group(1)) == val, name
    assert float(re.search(r"#define\s+LRT_REG_EPS\s+(\S+)", hdr).group(1)) == rg.EPS


def test_the_kernels_pass_the_resource_gate(reg_lib):
    res = resources.kernel_resources(reg_lib)
    own = sorted(n for n in res if resources.is_own_kernel(n))
    assert own == ["k_reg_linearize", "k_reg_solve"], own                                   # an iteration: these two launches
    assert all(any(re.search(g_, n) for g_ in resources.GATED) for n in own)
    assert resources.violations(res) == []
    for n in own:
        r = res[n]
        assert r["vgpr_spill"] == 0 and r["scratch_bytes"] == 0 and not r["dynamic_stack"], (n, r)
    assert res["k_reg_linearize"]["max_workgroup"] == 256 and res["k_reg_solve"]["max_workgroup"] == 64
    resources.check(reg_lib)


def test_argument_errors_come_before_the_device_and_launch_nothing(reg_lib):
    lib = rg.load()
    buf = (C.c_char * 8192)()
    p = (C.addressof(buf) + 255) // 256 * 256
    err = lambda: lib.lrt_reg_last_error()
    nodev = 1 << 20                                                                     # a device that does not exist: what passes the checks ends there
    wb = lib.lrt_reg_work_bytes
    assert wb(0, 8, 64) < 0 and wb(1, 0, 64) < 0 and wb(1, 8, 0) < 0 and wb(3, 30000, 30000) < 0 and wb(65536, 1, 1) < 0
    assert wb(3, 5, 37) == (8 * (30 * 3 * 1 + 3) + 255) // 256 * 256 and wb(1, 16, 128) == (8 * (30 * 8 + 1) + 255) // 256 * 256
    need = wb(1, 8, 64)
    sched = (C.c_double * 6)(2, 8, 2.0, 1, 2, 0.5)

    def lin(F=1, H=8, W=64, inc=p, n_inc=2, off=0.0, yaw=0.0, lo=0.0, hi=80.0, sp=p, sm=p, tp=p, tn=p, tm=p, X=p, rh=1, rw=2, md=1.0, huber=0.1, sums=p, ws=p,
            ws_bytes=need):
        return lib.lrt_reg_linearize(nodev, F, H, W, inc, n_inc, off, yaw, lo, hi, sp, sm, tp, tn, tm, X, rh, rw, md, huber, sums, None, ws, ws_bytes, None)

    def ali(F=1, H=8, W=64, inc=p, n_inc=2, off=0.0, yaw=0.0, lo=0.0, hi=80.0, sp=p, sm=p, tp=p, tn=p, tm=p, X=p, schedule=sched, K=2, huber=0.1, lam=1e-6,
            min_pairs=50, tol_t=1e-5, tol_r=1e-6, outs=(p, p, p, p), ws=p, ws_bytes=need):
        return lib.lrt_reg_align(nodev, F, H, W, inc, n_inc, off, yaw, lo, hi, sp, sm, tp, tn, tm, X, schedule, K, huber, lam, min_pairs, tol_t, tol_r, *outs,
                                 ws, ws_bytes, None)
    for call in (lin, ali):
        assert call(F=0) < 0 and b"0 pairs of 8 x 64" in err()
        assert call(F=70000, H=1, W=1, ws_bytes=1 << 30) < 0 and b"70000 pairs" in err()
        assert call(n_inc=3) < 0 and b"3 inclinations" in err()
        assert call(off=1.0) < 0 and b"pixel offset" in err()
        assert call(yaw=float("nan")) < 0 and b"yaw" in err()
        assert call(lo=5.0, hi=5.0) < 0 and b"depths" in err()
        assert call(inc=None) < 0 and b"null inclination" in err()
        assert call(sm=None) < 0 and b"null src_points / src_mask" in err()
        assert call(tn=None) < 0 and b"null tgt_points / tgt_normals / tgt_mask" in err()
        assert call(huber=0.0) < 0 and b"huber" in err()
        assert call(ws=p + 8) < 0 and b"256-byte aligned" in err()
        assert call(ws_bytes=need - 1) < 0 and (b"a workspace of %d bytes, 1 pairs of 8 x 64 need %d" % (need - 1, need)) in err()
        assert call() < 0 and b"no HIP device" in err()
    assert lin(rh=5) < 0 and b"a window of 5 rows" in err()
    assert lin(rw=17) < 0 and b"a window of 1 rows and 17 columns" in err()
    assert lin(md=0.0) < 0 and b"max_dist" in err()
    assert lin(X=None) < 0 and b"null X / sums" in err()
    assert ali(schedule=None) < 0 and b"null schedule" in err()
    assert ali(K=0) < 0 and ali(K=33) < 0 and b"33 iterations" in err()
    assert ali(schedule=(C.c_double * 6)(2, 8, 2.0, 1.5, 2, 0.5)) < 0 and b"a window of 1.5 rows" in err()
    assert ali(schedule=(C.c_double * 6)(2, 8, 2.0, 1, 2, -1.0)) < 0 and b"max_dist" in err()
    assert ali(lam=-1.0) < 0 and b"lambda" in err()
    assert ali(min_pairs=0) < 0 and b"min_pairs" in err()
    assert ali(tol_t=float("nan")) < 0 and b"tolerances" in err()
    assert ali(outs=(p, None, p, p)) < 0 and b"null X_init / X_out / log / hessian / status" in err()


def test_the_python_side_refuses_before_it_computes():
    c = rc.case("odd")
    src, tgt = tuple(t[0] for t in c.src), tuple(t[0] for t in c.tgt)
    with pytest.raises(rg.RegistrationError, match="inclination is required"):
        rg.align(src, tgt)
    with pytest.raises(rg.RegistrationError, match="normals must be"):
        rg.align(src, (tgt[0], None, tgt[2]), **c.kw)
    with pytest.raises(rg.RegistrationError, match="differ"):
        rg.align(src, c.tgt, **c.kw)
    with pytest.raises(rg.RegistrationError, match=r"schedule must be \(K, 3\)"):
        rg.align(src, tgt, schedule=[(1, 2, 0.5)] * 33, **c.kw)
    with pytest.raises(rg.RegistrationError, match="a window of 5"):
        rg.align(src, tgt, schedule=[(5, 2, 0.5)], **c.kw)
    with pytest.raises(rg.RegistrationError, match="float64"):
        rg.align(src, tgt, init=torch.eye(4), **c.kw)
    with pytest.raises(rg.RegistrationError, match="huber"):
        rg.linearize(src, tgt, torch.eye(4, dtype=torch.float64), 1, 2, 1.0, huber=-1.0, **c.kw)
    with pytest.raises(rg.RegistrationError, match="strictly monotonic"):
        rg.align(src, tgt, inclination=[0.1, 0.0, 0.2, 0.3, 0.4], data_type="KITTI")


# ---- 5. odometry ---------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chain():
    frames, truth, kw = rc.odometry_frames(3)
    est, rep = rg.odometry(frames, **kw)
    return frames, truth, kw, est, rep


def test_odometry_chains_three_frames_to_the_true_trajectory(chain):
    frames, truth, kw, est, rep = chain
    assert sorted(est) == [10, 12, 14] and np.array_equal(est[10], np.eye(4)) and rep["failed"] == []
    assert [(p["source"], p["target"], p["status"]) for p in rep["pairs"]] == [(12, 10, 3), (14, 12, 3)] and all(p["partners"] > 1000 for p in rep["pairs"])
    for i in (12, 14):
        et, er = rc.pose_error(est[i][:3], truth[i][:3])
        print(i, et, er)
        assert et <= 2.0 * rc.RECORDED_ODOMETRY[i][0] and er <= 2.0 * rc.RECORDED_ODOMETRY[i][1], (i, et, er)
    # the second pair starts from the first pair's result (the constant-velocity guess), not from the identity
    second = rg.align(frames[14], frames[12], torch.from_numpy(np.linalg.inv(est[10]) @ est[12])[:3].contiguous(), **kw)
    assert np.array_equal((est[12] @ np.vstack([second.X.numpy(), [0, 0, 0, 1]])), est[14])
    first = np.array([[0.0, -1.0, 0.0, 4.0], [1.0, 0.0, 0.0, -2.0], [0.0, 0.0, 1.0, 0.5], [0.0, 0.0, 0.0, 1.0]])
    moved, _ = rg.odometry(frames, first_pose=first, **kw)
    assert np.allclose(moved[14], first @ est[14], atol=1e-12)
    # a pair that cannot be aligned keeps the guess and is named
    broken = dict(frames)
    broken[14] = (frames[14][0], frames[14][1], torch.zeros_like(frames[14][2]))
    est2, rep2 = rg.odometry(broken, **kw)
    assert rep2["failed"] == [14] and rep2["pairs"][1]["status"] == rg.FEW
    assert np.array_equal(est2[14], est2[12] @ (np.linalg.inv(est2[10]) @ est2[12]))


# ---- 6. ingest ---------------------------------------------------------------------------------------------------------------------------------------------------

def _write_clouds(folder, frames):
    os.makedirs(folder, exist_ok=True)
    for i, (pts, _, mask) in frames.items():
        p = pts[mask].numpy()
        np.save(os.path.join(folder, f"{i}.npy"), np.concatenate([p, np.full((p.shape[0], 1), 0.5, np.float32)], 1))


COMMON = ["--height", "16", "--width", "128", "--inclination", "-0.43", "0.12", "--device", "cpu", "--max-depth", "80"]


def test_ingest_wants_exactly_one_source_of_poses(chain, tmp_path, capsys):
    frames = chain[0]
    pts = str(tmp_path / "pts")
    _write_clouds(pts, frames)
    np.save(tmp_path / "poses.npy", np.stack([chain[1][i] for i in sorted(frames)]))
    out = str(tmp_path / "out")
    assert ingest.main(["--points", pts, "--out", out] + COMMON) == 2 and "exactly one of --poses FILE and --odometry (neither" in capsys.readouterr().err
    assert ingest.main(["--points", pts, "--out", out, "--odometry", "--poses", str(tmp_path / "poses.npy")] + COMMON) == 2
    assert "exactly one of --poses FILE and --odometry (both" in capsys.readouterr().err
    assert ingest.main(["--points", pts, "--out", out, "--odometry", "--sweep", "--compensated"] + COMMON) == 2
    assert "--odometry does not go with --compensated" in capsys.readouterr().err
    assert ingest.main(["--points", pts, "--out", out, "--poses", str(tmp_path / "poses.npy"), "--first-pose", str(tmp_path / "poses.npy")] + COMMON) == 2
    assert not os.path.exists(out)
    with pytest.raises(ValueError, match="odometry finds the poses after the projection"):
        ingest.ingest_point_clouds(out, [], 16, 128, [-0.43, 0.12], odometry={}, twists={})


def test_ingest_with_odometry_writes_the_true_trajectory(chain, tmp_path, capsys):
    frames, truth, kw, est, _ = chain
    pts, out = str(tmp_path / "pts"), str(tmp_path / "out")
    _write_clouds(pts, frames)
    assert ingest.main(["--points", pts, "--out", out, "--odometry", "--sweep"] + COMMON) == 0
    assert "0 of 2 pairs kept the constant-velocity guess" in capsys.readouterr().out
    rep = json.load(open(os.path.join(out, "ingest.json")))
    odo = rep["odometry"]
    assert odo["schedule"] == [list(map(float, r)) for r in rg.DEFAULT_SCHEDULE] and odo["failed"] == [] and rep["pose_taken_from"] == {}
    assert [(p["source"], p["target"], p["status"]) for p in odo["pairs"]] == [(12, 10, 3), (14, 12, 3)] and all(p["partners"] > 1000 for p in odo["pairs"])
    from lidar_rt_amd import sequence, sweep
    got = {}
    for i in sorted(frames):
        z = np.load(sequence._frame_path(out, i))
        got[i] = z["sensor2world"].astype(np.float64)
        assert z["sensor2world"].dtype == np.float32 and "twist" in z.files
    for i in (12, 14):
        et, er = rc.pose_error(got[i][:3], truth[i][:3])
        assert et <= 2.0 * rc.RECORDED_ODOMETRY[i][0] + 1e-6 and er <= 2.0 * rc.RECORDED_ODOMETRY[i][1] + 1e-6, (i, et, er)
    want = sweep.twists_from_poses(got, 1.0)                                                # from the poses as stored, in float32
    assert np.abs(np.load(sequence._frame_path(out, 12))["twist"] - want[12]).max() <= 1e-5
    # --first-pose moves the whole trajectory
    first = np.array([[0.0, -1.0, 0.0, 4.0], [1.0, 0.0, 0.0, -2.0], [0.0, 0.0, 1.0, 0.5], [0.0, 0.0, 0.0, 1.0]])
    np.savetxt(tmp_path / "first.txt", first)
    out2 = str(tmp_path / "out2")
    assert ingest.main(["--points", pts, "--out", out2, "--odometry", "--first-pose", str(tmp_path / "first.txt")] + COMMON) == 0
    z = np.load(sequence._frame_path(out2, 14))
    assert np.abs(z["sensor2world"] - first @ got[14]).max() <= 1e-5 and "twist" not in z.files
    assert json.load(open(os.path.join(out2, "ingest.json")))["odometry"]["first_pose"] == first.tolist()


def _members(root):
    """{relative path: bytes of a text file, or {member: (dtype, shape, bytes)} of an .npz} -- the zip container stamps the time of writing, its members do not."""
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


def test_ingest_with_poses_writes_what_it_wrote_before(chain, tmp_path):
    """The command line with --poses against the call it made before --odometry existed (ingest_point_clouds with the poses read from the file, no
    odometry argument): every written file equal, ingest.json byte for byte."""
    frames, truth = chain[0], chain[1]
    pts = str(tmp_path / "pts")
    _write_clouds(pts, frames)
    ids = sorted(frames)
    np.save(tmp_path / "poses.npy", np.stack([truth[i] for i in ids]))
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    assert ingest.main(["--points", pts, "--poses", str(tmp_path / "poses.npy"), "--out", a, "--sweep", "--test-frames", "14"] + COMMON) == 0
    from lidar_rt_amd import sweep
    files = ingest.list_points(pts)
    use = ingest.read_poses(str(tmp_path / "poses.npy"), ids)
    ingest.ingest_point_clouds(b, ((i, ingest.read_points(p), use[i]) for i, p in files), 16, 128, [-0.43, 0.12], data_type="KITTI", sensor2ego=None, max_depth=80.0,
                               test_frames=[14], device="cpu", batch=16, wrap=True, notes={"pose_taken_from": {}, "sweep_fraction": 1.0},
                               twists=sweep.twists_from_poses(use, 1.0))
    ma, mb = _members(a), _members(b)
    assert sorted(ma) == sorted(mb) and "ingest.json" in ma and "odometry" not in json.loads(ma["ingest.json"])
    for rel in ma:
        assert ma[rel] == mb[rel], rel
