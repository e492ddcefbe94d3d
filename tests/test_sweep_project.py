"""Range images of a moving sensor without a GPU: the eleventh product library (`liblrt_sweepproj.so`: a source list and hash of its own that moves
no other hash, exports, resource gate, argument errors before the device is touched), the rule's header compiled for the host against the float64
twin point for point (plain and under the address and undefined-behaviour sanitizers), zero motion against the static projection bit for bit, the
round trip on the sweep-ray grid, agreement with that grid for any cloud, the unseen class, ties and occlusion, and the ingest of motion-compensated
clouds (function and command line) on the CPU path."""
import ctypes as C
import json
import math
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from lidar_rt_amd import build as lrt_build, ingest, range_image as ri, resources, sequence, sweep, sweep_project as sp
from tests import range_image_cases as rc, sweep_project_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


# ---- 1. the library -------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sweepproj_lib():
    return lrt_build.build_sweepproj()


def test_the_library_has_a_source_list_of_its_own_and_moves_no_other_hash():
    assert lrt_build.SWEEPPROJ_SOURCES == ["lrt_sweepproj.hip"]
    assert {"lrt_sweepproj_math.h", "lrt_project_math.h", "lrt_sweep_math.h", "lrt_device_guard.h"} <= set(lrt_build.SWEEPPROJ_HEADERS)
    lists = ("", "LOSS_", "GRIDCD_", "INIT_", "METRICS_", "ADAM_", "DENSIFY_", "PROJECT_", "SWEEP_", "REFINE_")
    others = sum((getattr(lrt_build, p + "SOURCES") + getattr(lrt_build, p + "HEADERS") for p in lists), [])
    assert not any("lrt_sweepproj" in f for f in others)
    # the other libraries' hashes at the commit this library was added on: the values the earlier tests pin
    pinned = {"source_hash": "2c98b54882a7ff74", "loss_source_hash": "cc56b0c83f72d5ca", "gridcd_source_hash": "fd279d9f7ff67722", "init_source_hash": "0fd7105f5d08ab22",
              "metrics_source_hash": "9e8267ef6335030b", "adam_source_hash": "1b4949dcebd155a4", "densify_source_hash": "223b0fc546560708",
              "project_source_hash": "974b6f2b8535fc99", "sweep_source_hash": "9d47a4b445577aef", "refine_source_hash": "8408e92aef295221"}
    for fn, want in pinned.items():
        assert getattr(lrt_build, fn)() == want, fn
    assert lrt_build.CODEGEN_FLAGS == ["-O3", "-munsafe-fp-atomics", "-fno-slp-vectorize"]
    assert "lrt_sweepproj" not in open(lrt_build.EXT_SRC).read()
    assert lrt_build.sweepproj_source_hash() not in pinned.values()
    assert os.path.basename(lrt_build.SWEEPPROJ_LIB) == "liblrt_sweepproj.so" and os.path.basename(lrt_build.SWEEPPROJ_STAMP) == "liblrt_sweepproj.srchash"
    src = open(lrt_build.__file__).read()
    product = src[src.index("def _build_product"):src.index("def _build_lib")]
    assert product.index("build_refine(force, verbose)") < product.index("build_sweepproj(force, verbose)")
    assert "csrc/liblrt_sweepproj.so" in open(os.path.join(REPO, "setup.py")).read()
    body = src[src.index("def build_sweepproj"):src.index("EXT_SRC =")]
    assert "CODEGEN_FLAGS" in body and "resources.check(SWEEPPROJ_LIB)" in body and "correctly-rounded" not in src and "fast-math" not in src


def test_the_library_builds_and_exports_what_its_header_declares(sweepproj_lib):
    assert os.path.exists(sweepproj_lib) and not lrt_build.sweepproj_is_stale()
    assert open(lrt_build.SWEEPPROJ_STAMP).read().strip() == lrt_build.sweepproj_source_hash()
    hdr = open(os.path.join(REPO, "include", "lrt_sweepproj.h")).read()
    declared = set(re.findall(r"\b(lrt_sweepproj_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(sp.EXPORTS), declared ^ set(sp.EXPORTS)
    lib = sp.load()
    for n in declared:
        assert hasattr(lib, n), n
    exported = set(re.findall(r"\blrt_sweepproj_[a-z_]+\b", subprocess.run(["nm", "-D", "--defined-only", sweepproj_lib], capture_output=True, text=True, check=True).stdout))
    assert exported == declared, exported ^ declared
    const = lambda name: int(re.search(r"#define\s+%s\s+\(?(\d+)" % name, hdr).group(1))
    assert lib.lrt_sweepproj_abi_version() == const("LRT_SWEEPPROJ_ABI_VERSION") == sp.ABI_VERSION
    assert const("LRT_SWEEPPROJ_N_COUNTS") == sp.N_COUNTS == len(sp.COUNT_NAMES) == 7 and const("LRT_SWEEPPROJ_BLOCK") == sp.BLOCK
    assert const("LRT_SWEEPPROJ_MAX_EVAL") == sp.MAX_EVAL == 8 and const("LRT_SWEEPPROJ_TABLE") == sp.TABLE == 12
    assert const("LRT_SWEEPPROJ_MAX_POINTS") == sp.MAX_POINTS and const("LRT_SWEEPPROJ_MAX_PIXELS") == sp.MAX_PIXELS
    mh = open(os.path.join(REPO, "lidar_rt_amd", "csrc", "lrt_sweepproj_math.h")).read()
    for name, v in (("SP_UNSEEN", sp.UNSEEN), ("SP_MAX_EVAL", sp.MAX_EVAL), ("SP_TABLE", sp.TABLE), ("SP_CONVERGED", sp.CONVERGED), ("SP_EDGE", sp.EDGE), ("SP_CYCLE", sp.CYCLE)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, mh).group(1)) == v
    assert sp.COUNT_NAMES == ri.COUNT_NAMES[:4] + ("unseen",) + ri.COUNT_NAMES[4:]
    assert '#include "lrt_project_math.h"' in mh and '#include "lrt_sweep_math.h"' in mh and mh.count("#pragma clang fp contract(off)") >= 6


def test_the_kernels_pass_the_resource_gate(sweepproj_lib):
    res = resources.kernel_resources(sweepproj_lib)
    own = sorted(n for n in res if resources.is_own_kernel(n))
    assert own == ["k_swproj_fill", "k_swproj_resolve", "k_swproj_scatter", "k_swproj_table"], own       # a call: at most these four launches
    assert all(any(re.search(g_, n) for g_ in resources.GATED) for n in own)
    assert resources.violations(res) == []
    for n in own:
        r = res[n]
        assert r["vgpr_spill"] == 0 and r["scratch_bytes"] == 0 and not r["dynamic_stack"], (n, r)
    resources.check(sweepproj_lib)


def test_argument_errors_come_before_the_device_and_launch_nothing(sweepproj_lib):
    lib = sp.load()
    buf = (C.c_char * 16384)()
    p = (C.addressof(buf) + 255) // 256 * 256
    err = lambda: lib.lrt_sweepproj_last_error()
    nodev = 1 << 20                                                                     # a device that does not exist: what passes the checks ends there
    wb = lib.lrt_sweepproj_work_bytes
    assert wb(0, 8, 64) < 0 and wb(1, 0, 64) < 0 and wb(1, 8, 0) < 0 and wb(3, 30000, 30000) < 0 and wb(1 << 40, 1, 1) < 0
    assert wb(1, 1, 1) == 256 and wb(3, 5, 37) == (3 * 5 * 37 * 8 + 3 * 37 * 96 + 255) // 256 * 256
    assert wb(1, 8, 64) == 8 * 64 * 8 + 64 * 96 == 10240 and wb(16, 66, 1030) == (16 * 66 * 1030 * 8 + 16 * 1030 * 96 + 255) // 256 * 256

    def call(N=10, points=p, F=1, offsets=p, T=None, twist=None, tau=None, H=8, W=64, inc=p, n_inc=2, off=0.0, yaw=0.0, lo=0.0, hi=80.0, wrap=1, outs=(p,) * 5, ws=p,
             ws_bytes=10240):
        return lib.lrt_sweepproj_points(nodev, N, points, F, offsets, T, twist, tau, H, W, inc, n_inc, off, yaw, lo, hi, wrap, *outs, ws, ws_bytes, None)
    assert call(N=-1) < 0 and b"-1 points" in err()
    assert call(N=1 << 31) < 0 and b"2147483648 points" in err()
    assert call(F=0) < 0 and b"0 frames of 8 x 64" in err()
    assert call(F=3, H=30000, W=30000) < 0 and b"3 frames of 30000 x 30000" in err()
    assert call(n_inc=3) < 0 and b"3 inclinations" in err()
    assert call(H=1, W=4, n_inc=1) < 0 and b"1 inclinations" in err()
    assert call(off=1.0) < 0 and b"pixel offset" in err()
    assert call(yaw=float("nan")) < 0 and b"yaw" in err()
    assert call(lo=-1.0) < 0 and b"depths" in err()
    assert call(lo=5.0, hi=5.0) < 0 and b"depths" in err()
    assert call(hi=float("inf")) < 0 and b"depths" in err()
    assert call(wrap=2) < 0 and b"wrap 2" in err()
    assert call(points=None) < 0 and b"null points" in err()
    assert call(offsets=None) < 0 and b"null offsets / inclination" in err()
    assert call(inc=None) < 0 and b"null offsets / inclination" in err()
    assert call(twist=p, tau=None) < 0 and b"null tau pointer with a twist" in err()
    for k in range(5):
        assert call(outs=tuple(None if j == k else p for j in range(5))) < 0 and b"null depth / intensity / mask / index / counts" in err()
    assert call(ws=p + 8) < 0 and b"256-byte aligned" in err()
    assert call(ws=None) < 0 and b"256-byte aligned" in err()
    assert call(ws_bytes=10239) < 0 and b"a workspace of 10239 bytes, 1 frames of 8 x 64 need 10240" in err()
    assert call() < 0 and b"no HIP device" in err()
    assert call(twist=p, tau=p) < 0 and b"no HIP device" in err()
    assert call(tau=p) < 0 and b"no HIP device" in err()                                # column times without a twist are not read
    assert call(N=0, points=None, H=8, W=8, n_inc=8) < 0 and b"no HIP device" in err()


def test_the_python_side_refuses_before_it_computes():
    pts = np.zeros((10, 4), np.float32)
    ok = dict(H=8, W=64, inclination=list(rc.KITTI_INC))
    tw = np.array(sc.MODERATE)
    for fn in (sp.project_points_sweep_reference, lambda p_, *a, **kw: sp.project_points_sweep(torch.as_tensor(p_), *a, **kw)):
        with pytest.raises(ri.ProjectionError, match=r"\(N, 4\)"):
            fn(np.zeros((10, 5), np.float32), twist=tw, **ok)
        with pytest.raises(ri.ProjectionError, match="offsets must ascend from 0 to 10"):
            fn(pts, twist=tw, **ok, offsets=[0, 7, 5, 10])
        with pytest.raises(ri.ProjectionError, match="offsets must ascend from 0 to 10"):
            fn(pts, twist=tw, **ok, offsets=[0, 5, 9])
        with pytest.raises(ri.ProjectionError, match="inclination holds 2 bounds or one angle per row"):
            fn(pts, 8, 64, [0.1] * 7, tw)
        with pytest.raises(ri.ProjectionError, match="strictly monotonic"):
            fn(pts, 8, 64, [-0.3, -0.2, -0.1, -0.15, 0.0, 0.01, 0.02, 0.03], tw)
        with pytest.raises(ri.ProjectionError, match="the two bounds differ"):
            fn(pts, 8, 64, [0.1, 0.1], tw)
        with pytest.raises(ri.ProjectionError, match="3 frames of 30000 x 30000"):
            fn(pts, 30000, 30000, list(rc.KITTI_INC), tw, offsets=[0, 3, 6, 10])
        with pytest.raises(ri.ProjectionError, match=r"points2sensor must be \(2, 3, 4\)"):
            fn(pts, twist=tw, **ok, offsets=[0, 5, 10], points2sensor=np.zeros((3, 3, 4)))
        with pytest.raises(ri.ProjectionError, match="depths"):
            fn(pts, twist=tw, **ok, max_depth=float("inf"))
        with pytest.raises(ri.ProjectionError, match="data_type"):
            fn(pts, twist=tw, **ok, data_type="nuScenes")
        with pytest.raises(ri.ProjectionError, match=r"twist must be \(6,\) or \(2, 6\)"):
            fn(pts, twist=np.zeros((3, 6)), **ok, offsets=[0, 5, 10])
        with pytest.raises(ri.ProjectionError, match=r"twist must be \(6,\) or \(1, 6\)"):
            fn(pts, twist=np.zeros(5), **ok)
        with pytest.raises(ri.ProjectionError, match="a non-finite twist"):
            fn(pts, twist=[1.0, 0, 0, 0, float("nan"), 0], **ok)
        with pytest.raises(ri.ProjectionError, match="a non-finite twist"):
            fn(pts, twist=[float("inf"), 0, 0, 0, 0, 0], **ok)
        with pytest.raises(ri.ProjectionError, match="a non-finite tau"):
            fn(pts, twist=tw, **ok, tau=[float("nan")] + [0.0] * 63)
        with pytest.raises(ri.ProjectionError, match="tau must hold 64 column times"):
            fn(pts, twist=tw, **ok, tau=np.zeros(63))
        with pytest.raises(ri.ProjectionError, match="direction"):
            fn(pts, twist=tw, **ok, direction="up")
    huge = torch.zeros((1, 4)).expand(2 ** 31, 4)                                         # no memory behind it
    with pytest.raises(ri.ProjectionError, match="2147483648 points"):
        sp.project_points_sweep(huge, twist=tw, **ok)


# ---- 2. the rule's header on the host -------------------------------------------------------------------------------------------------------------------

CHECK_SRC = os.path.join(HERE, "host_check", "sweepproj_check.cpp")


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sweepproj_check") / "sweepproj_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, CHECK_SRC])
    return exe


@pytest.fixture(scope="module")
def host_check_sanitized(tmp_path_factory):
    """The same stand-alone program under the address and undefined-behaviour sanitizers; None where g++ cannot link their runtime."""
    d = tmp_path_factory.mktemp("sweepproj_check_san")
    probe = str(d / "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + flags + ["-o", str(d / "probe"), probe], capture_output=True).returncode != 0:
        return None
    exe = str(d / "sweepproj_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", exe, CHECK_SRC])
    return exe


def run_host(exe, c, tmp_path):
    kw = c.kw
    N = c.points.shape[0]
    off_arr = np.array([0, N], np.int64) if kw["offsets"] is None else kw["offsets"]
    F = off_arr.size - 1
    inc = np.asarray(kw["inclination"], np.float64)
    off, yaw = ri.convention(kw["data_type"], kw["sensor2ego"])
    T = kw["points2sensor"]
    xi = None if kw["twist"] is None else np.ascontiguousarray(np.broadcast_to(np.asarray(kw["twist"], np.float64), (F, 6)))
    tau = sc.column_times(kw, kw["W"])
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<8i", N, F, kw["H"], kw["W"], inc.size, int(kw["wrap"]), int(T is not None), int(xi is not None)))
        f.write(struct.pack("<4d", off, yaw, kw["min_depth"], kw["max_depth"]))
        f.write(off_arr.astype(np.int64).tobytes()); f.write(inc.tobytes())
        if T is not None:
            f.write(np.ascontiguousarray(np.asarray(T, np.float64).reshape(F, -1, 4)[:, :3, :]).tobytes())
        if xi is not None:
            f.write(xi.tobytes()); f.write(np.ascontiguousarray(tau, np.float64).tobytes())
        f.write(c.points.tobytes())
    res = subprocess.run([exe, inp, out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "SWEEPPROJCHECK ok" in res.stdout, res.stdout + res.stderr
    return np.fromfile(out, np.int32).reshape(N, 5)


def compare_host(exe, cases, tmp_path):
    classes, most = set(), 0
    for c in cases:
        got = run_host(exe, c, tmp_path)
        t = c.twin
        assert np.array_equal(got[:, 3], t.drop.numpy().astype(np.int32)), c.key
        assert np.array_equal(got[:, :2], t.pixel.numpy()), c.key
        assert np.array_equal(got[:, 2].view(np.uint32), t.range_bits), c.key
        assert np.array_equal(got[:, 4], t.evals.numpy()), c.key
        classes |= set(got[:, 3].tolist())
        most = max(most, int(got[:, 4].max()))
    return classes, most


def test_the_rule_header_on_the_host_against_the_twin(host_check, tmp_path):
    """Drop class, pixel, range bits and evaluations of EVERY point of every small case equal the twin's, the sizes 1 x 1 and 2 x 3 included; so do
    those of the static cases with no twist at all."""
    cases = sc.all_cases_small()
    classes, most = compare_host(host_check, cases, tmp_path)
    assert classes == {ri.KEEP, ri.INVALID, ri.OUT_OF_RANGE, ri.OUT_OF_VIEW, sp.UNSEEN} and most == sp.MAX_EVAL and len(cases) >= 50
    assert {(c.kw["H"], c.kw["W"]) for c in cases} >= {(1, 1), (2, 3), (8, 64), (5, 37)}
    static = [sc.finish(("static",) + tuple(map(str, c.key)), c.points, c.kw["H"], c.kw["W"],
                        dict(inclination=c.kw["inclination"], data_type=c.kw["data_type"], sensor2ego=c.kw["sensor2ego"]),
                        dict(twist=None, tau=None, t_ref=0.5, direction="cw"), offsets=c.kw["offsets"], points2sensor=c.kw["points2sensor"],
                        max_depth=c.kw["max_depth"], min_depth=c.kw["min_depth"], wrap=c.kw["wrap"]) for c in rc.all_cases_small()[::5]]
    classes, most = compare_host(host_check, static, tmp_path)
    assert sp.UNSEEN not in classes and most == 1


def test_the_host_program_under_the_sanitizers(host_check_sanitized, tmp_path):
    """A stand-alone host program: nothing is loaded into Python, nothing is preloaded."""
    if host_check_sanitized is None:
        pytest.skip("g++ cannot link the sanitizer runtime here")
    classes, most = compare_host(host_check_sanitized, sc.all_cases_small(), tmp_path)
    assert sp.UNSEEN in classes and most == sp.MAX_EVAL


# ---- 3. zero motion is the static projection ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("twist", [None, sc.ZERO], ids=["no_twist", "zero_twist"])
def test_zero_motion_is_the_static_projection_bit_for_bit(twist):
    cases = rc.all_cases_small()
    for c in cases:
        got = sp.project_points_sweep_reference(c.points, twist=twist, **c.kw)
        want = c.twin
        for k in ("depth", "intensity"):
            assert torch.equal(getattr(got, k).view(torch.int32), getattr(want, k).view(torch.int32)), (c.key, k)
        assert torch.equal(got.mask, want.mask) and torch.equal(got.index, want.index), c.key
        cnt = got.counts.reshape(-1, sp.N_COUNTS)
        assert torch.equal(cnt[:, [0, 1, 2, 3, 5, 6]], want.counts.reshape(-1, ri.N_COUNTS)) and int(cnt[:, 4].sum()) == 0, c.key
        assert torch.equal(got.drop, want.drop) and torch.equal(got.pixel, want.pixel) and np.array_equal(got.range_bits, want.range_bits), c.key
        assert int(got.evals.max()) <= 1
    assert len(cases) >= 30
    # a twist is not looked at where the column time is zero: (-2, -0.0, 0) keeps the sign of its zero there too
    c = rc.constructed("bounds", False)
    got = sp.project_points_sweep_reference(c.points, twist=sc.STRONG, tau=np.zeros(64), **c.kw)
    assert torch.equal(got.drop, c.twin.drop) and torch.equal(got.pixel, c.twin.pixel)


# ---- 4. it inverts the sweep rays -----------------------------------------------------------------------------------------------------------------------------

def check_round_trip(c, H, W):
    t = c.twin
    assert torch.equal(t.index.reshape(-1), torch.arange(H * W, dtype=torch.int32)) and bool(t.mask.all())
    assert t.counts.tolist() == [H * W, 0, 0, 0, 0, 0, H * W]
    r = torch.from_numpy(c.ranges)
    assert float(((t.depth.reshape(-1).double() - r).abs() / r).max()) <= 1e-6                # float32 points and a float32 depth
    assert torch.equal(t.intensity.reshape(-1), torch.tensor(c.points[:, 3]))


@pytest.mark.parametrize("posed", [False, True], ids=["sensor_frame", "posed"])
@pytest.mark.parametrize("mo", ["moderate_cw", "moderate_ccw"])
@pytest.mark.parametrize("conv", sc.CONVENTIONS)
@pytest.mark.parametrize("H,W", sc.SIZES)
def test_every_sweep_rays_point_comes_back_to_its_own_pixel(H, W, conv, mo, posed):
    check_round_trip(sc.grid(H, W, conv, sc.GRID_SEED, mo, posed=posed), H, W)


@pytest.mark.parametrize("mo", ["strong_cw", "minus_strong_ccw"])
@pytest.mark.parametrize("H,W", sc.SIZES)
def test_the_strong_turn_in_the_direction_whose_seam_has_a_gap(H, W, mo):
    """Turning with the column order (+0.3 rad with cw, -0.3 rad with ccw) overlaps adjacent bins and leaves the gap at the seam: every ray is a
    fixed point that the search reaches."""
    for conv in sc.CONVENTIONS:
        c = sc.grid(H, W, conv, sc.GRID_SEED, mo)
        check_round_trip(c, H, W)
        assert int(c.twin.evals.max()) > 1


@pytest.mark.parametrize("mo", ["strong_ccw", "minus_strong_cw"])
@pytest.mark.parametrize("H,W", sc.SIZES)
def test_the_strong_turn_in_the_direction_whose_seam_overlaps(H, W, mo):
    """Turning against the column order closes the seam: the first and the last columns, a sweep apart, see the same points.  Every point is
    kept, and one that is not on its own pixel has been seen by the columns across the seam: both columns lie within the overlap's width of it
    (the turn's share of the circle, and one column for the parallax of the 3 m the sensor moves)."""
    c = sc.grid(H, W, "kitti_bounds", sc.GRID_SEED, mo, own_pixel=False)
    t = c.twin
    assert bool((t.drop == ri.KEEP).all()) and int(t.counts[4]) == 0
    width = abs(sc.STRONG[5]) * W / (2.0 * math.pi) + 1.0
    own = np.arange(H * W) % W
    found = t.pixel[:, 0].numpy()
    moved = np.flatnonzero(found != own)
    assert moved.size > 0
    near = lambda w: np.minimum(w + 0.5, W - 0.5 - w) <= width                              # columns from the seam, which lies at u = -0.5 = W - 0.5
    assert bool(near(own[moved]).all()) and bool(near(found[moved]).all())
    assert bool((np.abs(found[moved] - own[moved]) > W / 2).all())                           # across the seam, not to a neighbour


# ---- 5. agreement with the ray grid, for any cloud --------------------------------------------------------------------------------------------------------------

def half_diagonals(kw):
    """(H,) the largest angle between a pixel's centre ray and a direction inside the pixel: half a column and half a row (bounds), or the larger
    half gap to a neighbouring beam (table); sin^2(t / 2) <= sin^2(a / 2) + sin^2(b / 2) for azimuth and elevation differences a and b."""
    H, W = kw["H"], kw["W"]
    inc = np.asarray(kw["inclination"], np.float64)
    a = math.pi / W
    if inc.size == 2:
        b = np.full(H, 0.5 * abs(inc[1] - inc[0]) / H)
    else:
        beams = inc[::-1]                                                                # row h has inclination[H - 1 - h]
        gap = np.abs(np.diff(beams))
        b = 0.5 * np.maximum(np.concatenate([[gap[0]], gap]), np.concatenate([gap, [gap[-1]]]))
    return 2.0 * np.arcsin(np.sqrt(np.sin(a / 2) ** 2 + np.sin(b / 2) ** 2))


CLOUDS = [(H, W, cn, mo, wrap, tr) for H, W in sc.SIZES for cn in sc.CONVENTIONS
          for mo, wrap, tr in (("moderate_cw", True, False), ("strong_ccw", False, True), ("table", True, True))]


@pytest.mark.parametrize("H,W,conv,mo,wrap,transform", CLOUDS)
def test_every_kept_pixel_agrees_with_the_ray_grid(H, W, conv, mo, wrap, transform):
    """For any cloud: the winner of pixel (h, w) lies within the pixel's half diagonal of the sweep ray d[h, w] as seen from that column's
    origin, and its distance from that origin rounds to the stored depth -- direction, t_ref, off, yaw and the table's order are sweep_rays'."""
    c = sc.random_cloud(1000, 3, H, W, conv, 11, mo, wrap=wrap, transform=transform)
    kw, t = c.kw, c.twin
    conv_ = rc.convention(conv, H)
    s2e = None if conv_["sensor2ego"] is None else torch.tensor(conv_["sensor2ego"])
    tau = torch.tensor(sc.column_times(kw, W))
    off_arr = kw["offsets"]
    frame = np.repeat(np.arange(3), np.diff(off_arr))
    p = c.points[:, :3].astype(np.float64)
    if kw["points2sensor"] is not None:
        T = np.asarray(kw["points2sensor"])[frame]
        with np.errstate(all="ignore"):
            p = np.einsum("nij,nj->ni", T[:, :3, :3], p) + T[:, :3, 3]
    half = half_diagonals(kw)
    eye = torch.eye(4, dtype=torch.float64)
    checked = 0
    for f in range(3):
        xi = torch.tensor(np.asarray(kw["twist"], np.float64).reshape(-1, 6)[f if np.ndim(kw["twist"]) == 2 else 0])
        _, d = sweep.sweep_rays_reference(eye, xi, H, W, kw["inclination"], kw["data_type"], s2e, tau=tau)
        _, o = sweep.column_poses_reference(eye[None, :3], xi[None], tau)                    # the columns' origins at float64 column times
        d, o = d.numpy(), o[0].numpy()
        hs, ws = np.nonzero(t.mask[f].numpy())
        rows = off_arr[f] + t.index[f].numpy()[hs, ws]
        v = p[rows] - o[ws]
        dist = np.sqrt((v * v).sum(1))
        cosang = np.clip((v * d[hs, ws]).sum(1) / dist, -1.0, 1.0)
        ang = np.arctan2(np.linalg.norm(np.cross(v, d[hs, ws]), axis=1), (v * d[hs, ws]).sum(1))
        assert bool((ang <= half[hs] + 1e-9).all()), (f, float((ang - half[hs]).max()), cosang.min())
        assert np.array_equal(dist.astype(np.float32).view(np.uint32), t.depth[f].numpy()[hs, ws].view(np.uint32)), f
        checked += hs.size
    assert checked == int(t.counts[:, 6].sum()) > 100


# ---- 6. the unseen class ------------------------------------------------------------------------------------------------------------------------------------------

def test_the_unseen_class_is_exercised_and_bounded():
    for H, W in sc.SIZES + [(66, 1030)]:
        m = sc.random_cloud(1000, 1, H, W, "kitti_bounds", 11, "moderate_cw").twin
        assert 0 < int(m.counts[4]) <= 30 and int((m.drop == sp.UNSEEN).sum()) == int(m.counts[4]), (H, W, m.counts.tolist())
        assert bool((m.evals[m.drop == sp.UNSEEN] == sp.MAX_EVAL).all())
        for mo in ("strong_cw", "strong_ccw"):
            s = sc.random_cloud(1000, 1, H, W, "kitti_bounds", 11, mo).twin
            assert 0 < int(s.counts[4]) <= 100, (H, W, mo, s.counts.tolist())
        print(f"SWEEPPROJ|unseen of 1000|{H} x {W}|moderate {int(m.counts[4])}|strong cw {int(s.counts[4])}")


def test_points_between_two_columns_are_unseen_and_a_point_beyond_the_edge_is_out_of_view():
    c = sc.between_columns()
    t = c.twin
    assert t.drop.tolist() == [sp.UNSEEN, sp.UNSEEN, ri.KEEP] and t.evals.tolist()[:2] == [sp.MAX_EVAL] * 2
    assert t.counts.tolist() == [3, 0, 0, 0, 2, 0, 1] and t.pixel.tolist()[:2] == [[-1, -1]] * 2 and t.pixel.tolist()[2] == [20, 3]
    # the same points under the static rule are ordinary returns: it is the motion that hides them
    st = ri.project_points_reference(c.points, **sc.static_kw(c.kw))
    assert st.drop.tolist() == [ri.KEEP] * 3
    e = sc.beyond_the_edge().twin
    assert e.drop.tolist() == [ri.OUT_OF_VIEW, ri.KEEP] and e.counts.tolist() == [2, 0, 0, 1, 0, 0, 1] and int(e.evals[0]) < sp.MAX_EVAL


# ---- 7. ties, occlusion and contention on one pixel under motion -----------------------------------------------------------------------------------------------

def test_a_thousand_points_on_one_sweep_ray_leave_one_pixel():
    c = sc.one_ray(1000)
    t = c.twin
    assert t.counts.tolist() == [1000, 0, 0, 0, 0, 999, 1] and int(t.mask.sum()) == 1 and bool(t.mask[3, 20])
    k = int(np.argmin(c.ranges))
    assert int(t.index[3, 20]) == k and abs(float(t.depth[3, 20]) - c.ranges[k]) <= 1e-6 * c.ranges[k]
    assert float(t.intensity[3, 20]) == float(c.points[k, 3])
    # the static rule spreads the same points over other pixels: the sensor moved
    st = ri.project_points_reference(c.points, **sc.static_kw(c.kw))
    assert int(st.mask.sum()) > 1


def test_equal_ranges_go_to_the_lower_index_and_a_nearer_point_wins():
    c = sc.one_ray(300, equal=True)
    t = c.twin
    assert t.counts.tolist() == [300, 0, 0, 0, 0, 299, 1] and int(t.index[3, 20]) == 0 and float(t.intensity[3, 20]) == float(c.points[0, 3])
    assert len(set(t.range_bits.tolist())) == 1
    near = sc.one_ray(1000)
    k = int(np.argmin(near.ranges))
    pts = np.concatenate([c.points, near.points[k:k + 1]])                                   # a nearer point that comes last
    t2 = sp.project_points_sweep_reference(pts, **c.kw)
    assert int(t2.index[3, 20]) == 300 and int(t2.counts[5]) == 300


def test_a_permuted_order_gives_the_same_image_with_the_index_following():
    c = sc.random_cloud(1000, 1, 8, 64, "kitti_bounds", 11, "moderate_cw")
    perm = np.random.default_rng(4).permutation(1000)
    t = sp.project_points_sweep_reference(np.ascontiguousarray(c.points[perm]), **c.kw)
    assert torch.equal(t.depth.view(torch.int32), c.twin.depth.view(torch.int32)) and torch.equal(t.counts, c.twin.counts) and torch.equal(t.mask, c.twin.mask)
    m = c.twin.mask.numpy()
    assert np.array_equal(perm[t.index.numpy()[m]], c.twin.index.numpy()[m])


def test_the_counts_add_up_on_every_case():
    for c in sc.all_cases_small():
        cnt = c.twin.counts.reshape(-1, sp.N_COUNTS)
        assert torch.equal(cnt[:, 0], cnt[:, 1:].sum(1)), c.key
        assert int(cnt[:, 6].sum()) == int(c.twin.mask.sum()) and int(cnt[:, 0].sum()) == c.points.shape[0]
        assert bool((c.twin.index[~c.twin.mask] == -1).all()) and bool((c.twin.depth[~c.twin.mask] == 0).all())
        if c.kw["offsets"] is not None and c.kw["offsets"].size == 4:
            assert cnt[1].tolist() == [0] * 7                                             # the empty middle frame


# ---- 8. ingest ----------------------------------------------------------------------------------------------------------------------------------------------------

def ingest_compensated(root, ic, **kw):
    return ingest.ingest_point_clouds(root, ((f.id, f.points, f.sensor2world) for f in ic.frames), ic.H, ic.W, ic.inclination, twists={f.id: f.twist for f in ic.frames},
                                      compensated=True, sweep_ref=ic.t_ref, sweep_direction=ic.direction, test_frames=[7], **kw)


def check_compensated(root, ic):
    seq = sequence.load_sequence(root, device="cpu", sweep="stored")
    rep = json.load(open(os.path.join(root, "ingest.json")))
    tau = sweep.column_times(ic.W, ic.t_ref, ic.direction)
    assert rep["compensated"] is True and rep["sweep_ref"] == ic.t_ref and rep["sweep_direction"] == ic.direction
    assert [f["id"] for f in rep["frames"]] == [f.id for f in ic.frames]
    for f, r in zip(ic.frames, rep["frames"]):
        z = np.load(os.path.join(root, "frames", f"{f.id:06d}.npz"))
        assert np.array_equal(z["mask"], f.mask), f.id
        want = f.depth.astype(np.float64)
        assert bool((np.abs(z["depth"].astype(np.float64) - want) <= 1e-6 * want).all()), f.id
        assert np.array_equal(z["intensity"].view(np.uint32), f.intensity.view(np.uint32)), f.id
        twin = sp.project_points_sweep_reference(f.points, ic.H, ic.W, ic.inclination, f.twist, t_ref=ic.t_ref, direction=ic.direction)
        assert twin.margin >= sc.MARGIN and twin.range_margin >= sc.RANGE_MARGIN
        assert np.array_equal(z["depth"].view(np.uint32), twin.depth.numpy().view(np.uint32)), f.id      # the depth bits are the twin's
        assert set(r) == {"id"} | set(sp.COUNT_NAMES)
        assert r["hidden"] == f.n_extra and r["out_of_view"] + r["unseen"] == f.n_out and r["invalid"] == 0 and r["out_of_range"] == 0
        assert r["pixels"] == int(f.mask.sum()) and r["points"] == f.points.shape[0] == sum(r[n] for n in sp.COUNT_NAMES[1:])
        assert np.allclose(z["twist"], f.twist.astype(np.float32)) and np.allclose(z["tau"], tau.numpy().astype(np.float32)) and z["tau"].shape == (ic.W,)
    assert rep["total"] == {n: sum(fr[n] for fr in rep["frames"]) for n in sp.COUNT_NAMES}
    return seq, rep


@pytest.mark.parametrize("direction,t_ref", [("cw", 0.5), ("ccw", 0.0)])
def test_ingest_of_compensated_clouds_on_the_cpu(tmp_path, direction, t_ref):
    ic = sc.ingest_clouds(direction=direction, t_ref=t_ref)
    root = str(tmp_path / "seq")
    rep = ingest_compensated(root, ic, device="cpu", batch=3)
    seq, on_disk = check_compensated(root, ic)
    assert rep == on_disk and rep["device"] == "cpu"
    assert sum(f.n_extra for f in ic.frames) > 100
    # load_sequence(..., sweep="stored") trains with the column times the images were built with
    tau = sweep.column_times(ic.W, t_ref, direction).to(torch.float32)
    other = sequence.load_sequence(root, device="cpu", sweep="stored", sweep_ref=0.25, sweep_direction="cw" if direction == "ccw" else "ccw")
    for s in (seq, other):                                                                   # the stored times win over the loader's defaults
        assert sorted(s.frames.sweep_meta) == [f.id for f in ic.frames]
        for f in ic.frames:
            twist, stored = s.frames.sweep_meta[f.id]
            assert torch.equal(stored.cpu(), tau) and torch.equal(twist.cpu(), torch.as_tensor(f.twist.astype(np.float32)))
    # the batch size does not show in the files
    root1 = str(tmp_path / "seq1")
    ingest_compensated(root1, ic, device="cpu", batch=1)
    for f in ic.frames:
        za, zb = (np.load(os.path.join(r, "frames", f"{f.id:06d}.npz")) for r in (root, root1))
        assert sorted(za.files) == sorted(zb.files) and all(za[k].tobytes() == zb[k].tobytes() for k in za.files)


def test_the_uncompensated_path_does_not_give_that_mask_and_writes_what_it_wrote(tmp_path):
    ic = sc.ingest_clouds()
    root = str(tmp_path / "raw")
    rep = ingest.ingest_point_clouds(root, ((f.id, f.points, f.sensor2world) for f in ic.frames), ic.H, ic.W, ic.inclination, twists={f.id: f.twist for f in ic.frames},
                                     device="cpu", batch=3)
    differing = 0
    for f in ic.frames:
        z = np.load(os.path.join(root, "frames", f"{f.id:06d}.npz"))
        assert "tau" not in z.files and "twist" in z.files
        differing += int((z["mask"] != f.mask).sum())
    assert differing >= 1, "the static projection of compensated clouds gave the moving sensor's mask"
    assert "compensated" not in rep and "sweep_ref" not in rep and set(rep["total"]) == set(ri.COUNT_NAMES)
    with pytest.raises(ValueError, match="compensated clouds need the twists"):
        ingest.ingest_point_clouds(str(tmp_path / "x"), iter(()), ic.H, ic.W, ic.inclination, compensated=True, device="cpu")
    with pytest.raises(ValueError, match="has no twist"):
        ingest.ingest_point_clouds(str(tmp_path / "y"), ((f.id, f.points, f.sensor2world) for f in ic.frames), ic.H, ic.W, ic.inclination, twists={3: ic.frames[0].twist},
                                   compensated=True, device="cpu")


def test_the_command_line_with_compensated_clouds(tmp_path):
    ic = sc.ingest_clouds()
    pts = tmp_path / "pts"
    pts.mkdir()
    for f in ic.frames:
        np.save(str(pts / f"{f.id}.npy"), f.points)
    np.save(str(tmp_path / "poses.npy"), np.stack([f.sensor2world for f in ic.frames]))
    common = ["--points", str(pts), "--poses", str(tmp_path / "poses.npy"), "--height", str(ic.H), "--width", str(ic.W), "--inclination", repr(ic.inclination[0]),
              repr(ic.inclination[1]), "--device", "cpu"]
    out = str(tmp_path / "out")
    res = subprocess.run([sys.executable, "-m", "lidar_rt_amd.ingest", "--out", out, "--sweep", "--compensated", "--sweep-ref", "0.0", "--sweep-direction", "ccw"] + common,
                         capture_output=True, text=True, cwd=REPO, timeout=300)
    assert res.returncode == 0 and re.search(r"\d+ unseen", res.stdout), res.stdout + res.stderr
    rep = json.load(open(os.path.join(out, "ingest.json")))
    assert rep["compensated"] is True and rep["sweep_ref"] == 0.0 and rep["sweep_direction"] == "ccw" and rep["sweep_fraction"] == 1.0
    assert set(rep["total"]) == set(sp.COUNT_NAMES) and f"{rep['total']['unseen']} unseen" in res.stdout
    twists = sweep.twists_from_poses({f.id: f.sensor2world for f in ic.frames}, 1.0)
    tau = sweep.column_times(ic.W, 0.0, "ccw").numpy()
    for f in ic.frames:
        z = np.load(os.path.join(out, "frames", f"{f.id:06d}.npz"))
        twin = sp.project_points_sweep_reference(f.points, ic.H, ic.W, ic.inclination, twists[f.id], tau=tau)
        assert np.array_equal(z["depth"].view(np.uint32), twin.depth.numpy().view(np.uint32)) and np.array_equal(z["mask"], twin.mask.numpy())
        assert np.allclose(z["tau"], tau.astype(np.float32))
    # without --sweep the flag is refused before anything is read or written
    refused = str(tmp_path / "refused")
    assert ingest.main(["--out", refused, "--compensated"] + common) == 2 and not os.path.exists(refused)
    # the uncompensated command line names no unseen points
    raw = str(tmp_path / "raw")
    res = subprocess.run([sys.executable, "-m", "lidar_rt_amd.ingest", "--out", raw, "--sweep"] + common, capture_output=True, text=True, cwd=REPO, timeout=300)
    assert res.returncode == 0 and "unseen" not in res.stdout and "compensated" not in json.load(open(os.path.join(raw, "ingest.json")))
