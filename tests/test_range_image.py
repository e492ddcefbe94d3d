"""Range images from point clouds without a GPU: the eighth product library (`liblrt_project.so`: a source list and hash of its own that moves no
other hash, exports, resource gate, argument errors before the device is touched), the rule's header compiled for the host against the float64
twin point for point, the round trip on this repository's ray grid, the reference's lost column under `wrap=False`, constructed points, ties and
occlusion, and the ingest of point clouds into a sequence directory (function and command line) on the CPU path."""
import ctypes as C
import json
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from lidar_rt_amd import build as lrt_build, ingest, range_image as ri, resources, sequence
from tests import range_image_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


# ---- build ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def project_lib():
    return lrt_build.build_project()


def test_the_library_has_a_source_list_of_its_own_and_moves_no_other_hash():
    assert lrt_build.PROJECT_SOURCES == ["lrt_project.hip"] and "lrt_project_math.h" in lrt_build.PROJECT_HEADERS
    others = (lrt_build.SOURCES + lrt_build.HEADERS + lrt_build.LOSS_SOURCES + lrt_build.LOSS_HEADERS + lrt_build.GRIDCD_SOURCES + lrt_build.GRIDCD_HEADERS
              + lrt_build.INIT_SOURCES + lrt_build.INIT_HEADERS + lrt_build.METRICS_SOURCES + lrt_build.METRICS_HEADERS + lrt_build.ADAM_SOURCES + lrt_build.ADAM_HEADERS
              + lrt_build.DENSIFY_SOURCES + lrt_build.DENSIFY_HEADERS)
    assert not any("lrt_project" in f for f in others)
    # the other libraries' hashes at the commit this library was added on: committed profiles are keyed by them
    assert lrt_build.source_hash() == "2c98b54882a7ff74"          # moved twice since: the non-finite-input fixes in lrt_chamfer.hip; a comment of include/lrt.h (lrt_xchg_apply, zero_only on an overflowed block)
    assert lrt_build.loss_source_hash() == "cc56b0c83f72d5ca"
    assert lrt_build.gridcd_source_hash() == "fd279d9f7ff67722"
    assert lrt_build.init_source_hash() == "0fd7105f5d08ab22"
    assert lrt_build.metrics_source_hash() == "9e8267ef6335030b"
    assert lrt_build.adam_source_hash() == "1b4949dcebd155a4"
    assert lrt_build.densify_source_hash() == "223b0fc546560708"
    assert "lrt_project" not in open(lrt_build.EXT_SRC).read()
    mine = lrt_build.project_source_hash()
    assert mine not in (lrt_build.source_hash(), lrt_build.loss_source_hash(), lrt_build.gridcd_source_hash(), lrt_build.init_source_hash(),
                        lrt_build.metrics_source_hash(), lrt_build.adam_source_hash(), lrt_build.densify_source_hash())
    assert os.path.basename(lrt_build.PROJECT_LIB) == "liblrt_project.so"
    assert lrt_build.PROJECT_LIB not in (lrt_build.LIB, lrt_build.LOSS_LIB, lrt_build.GRIDCD_LIB, lrt_build.INIT_LIB, lrt_build.METRICS_LIB, lrt_build.ADAM_LIB,
                                         lrt_build.DENSIFY_LIB)
    src = open(lrt_build.__file__).read()
    assert "build_project(force, verbose)" in src                                        # _build_product builds it
    assert "csrc/liblrt_project.so" in open(os.path.join(REPO, "setup.py")).read()
    body = src[src.index("def build_project"):src.index("EXT_SRC =")]
    assert "CODEGEN_FLAGS" in body and "resources.check(PROJECT_LIB)" in body and "correctly-rounded" not in src and "fast-math" not in src


def test_the_library_builds_and_exports_what_its_header_declares(project_lib):
    assert os.path.exists(project_lib) and not lrt_build.project_is_stale()
    assert open(lrt_build.PROJECT_STAMP).read().strip() == lrt_build.project_source_hash()
    hdr = open(os.path.join(REPO, "include", "lrt_project.h")).read()
    declared = set(re.findall(r"\b(lrt_project_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(ri.EXPORTS), declared ^ set(ri.EXPORTS)
    lib = ri.load()
    for n in declared:
        assert hasattr(lib, n), n
    exported = set(re.findall(r"\blrt_project_[a-z_]+\b", subprocess.run(["nm", "-D", "--defined-only", project_lib], capture_output=True, text=True, check=True).stdout))
    assert exported == declared, exported ^ declared
    const = lambda name: int(re.search(r"#define\s+%s\s+\(?(\d+)" % name, hdr).group(1))
    assert lib.lrt_project_abi_version() == const("LRT_PROJECT_ABI_VERSION") == ri.ABI_VERSION
    assert const("LRT_PROJECT_N_COUNTS") == ri.N_COUNTS == len(ri.COUNT_NAMES) and const("LRT_PROJECT_BLOCK") == ri.BLOCK
    assert const("LRT_PROJECT_MAX_POINTS") == ri.MAX_POINTS and const("LRT_PROJECT_MAX_PIXELS") == ri.MAX_PIXELS
    mh = open(os.path.join(REPO, "lidar_rt_amd", "csrc", "lrt_project_math.h")).read()
    for name, v in (("PJ_KEEP", ri.KEEP), ("PJ_INVALID", ri.INVALID), ("PJ_OUT_OF_RANGE", ri.OUT_OF_RANGE), ("PJ_OUT_OF_VIEW", ri.OUT_OF_VIEW)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, mh).group(1)) == v


def test_the_kernels_pass_the_resource_gate(project_lib):
    res = resources.kernel_resources(project_lib)
    own = sorted(n for n in res if resources.is_own_kernel(n))
    assert own == ["k_project_fill", "k_project_resolve", "k_project_scatter"], own       # a call: at most these three launches
    assert all(any(re.search(g_, n) for g_ in resources.GATED) for n in own)
    assert resources.violations(res) == []
    for n in own:
        r = res[n]
        assert r["vgpr_spill"] == 0 and r["scratch_bytes"] == 0 and not r["dynamic_stack"], (n, r)
    resources.check(project_lib)


def test_argument_errors_come_before_the_device_and_launch_nothing(project_lib):
    lib = ri.load()
    buf = (C.c_char * 8192)()
    p = (C.addressof(buf) + 255) // 256 * 256
    err = lambda: lib.lrt_project_last_error()
    nodev = 1 << 20                                                                     # a device that does not exist: what passes the checks ends there
    assert lib.lrt_project_work_bytes(0, 8, 64) < 0 and lib.lrt_project_work_bytes(1, 0, 64) < 0 and lib.lrt_project_work_bytes(1, 8, 0) < 0
    assert lib.lrt_project_work_bytes(3, 30000, 30000) < 0 and lib.lrt_project_work_bytes(1 << 40, 1, 1) < 0
    assert lib.lrt_project_work_bytes(1, 1, 1) == 256 and lib.lrt_project_work_bytes(3, 5, 37) == (3 * 5 * 37 * 8 + 255) // 256 * 256
    assert lib.lrt_project_work_bytes(16, 66, 1030) == 16 * 66 * 1030 * 8

    def call(N=10, points=p, F=1, offsets=p, T=None, H=8, W=64, inc=p, n_inc=2, off=0.0, yaw=0.0, lo=0.0, hi=80.0, wrap=1, outs=(p,) * 5, ws=p, ws_bytes=4096):
        return lib.lrt_project_points(nodev, N, points, F, offsets, T, H, W, inc, n_inc, off, yaw, lo, hi, wrap, *outs, ws, ws_bytes, None)
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
    for k in range(5):
        assert call(outs=tuple(None if j == k else p for j in range(5))) < 0 and b"null depth / intensity / mask / index / counts" in err()
    assert call(ws=p + 8) < 0 and b"256-byte aligned" in err()
    assert call(ws=None) < 0 and b"256-byte aligned" in err()
    assert call(ws_bytes=4095) < 0 and b"a workspace of 4095 bytes, 1 frames of 8 x 64 need 4096" in err()
    assert call() < 0 and b"no HIP device" in err()
    assert call(N=0, points=None, H=8, W=8, n_inc=8) < 0 and b"no HIP device" in err()


def test_the_python_side_refuses_before_it_computes():
    pts = np.zeros((10, 4), np.float32)
    ok = dict(H=8, W=64, inclination=list(rc.KITTI_INC))
    for fn in (ri.project_points_reference, lambda p_, *a, **kw: ri.project_points(torch.as_tensor(p_), *a, **kw)):
        with pytest.raises(ri.ProjectionError, match=r"\(N, 4\)"):
            fn(np.zeros((10, 5), np.float32), **ok)
        with pytest.raises(ri.ProjectionError, match="offsets must ascend from 0 to 10"):
            fn(pts, **ok, offsets=[0, 7, 5, 10])
        with pytest.raises(ri.ProjectionError, match="offsets must ascend from 0 to 10"):
            fn(pts, **ok, offsets=[0, 5, 9])
        with pytest.raises(ri.ProjectionError, match="inclination holds 2 bounds or one angle per row"):
            fn(pts, 8, 64, [0.1] * 7)
        with pytest.raises(ri.ProjectionError, match="strictly monotonic"):
            fn(pts, 8, 64, [-0.3, -0.2, -0.1, -0.15, 0.0, 0.01, 0.02, 0.03])
        with pytest.raises(ri.ProjectionError, match="strictly monotonic"):
            fn(pts, 8, 64, [-0.3, -0.2, -0.1, -0.1, 0.0, 0.01, 0.02, 0.03])
        with pytest.raises(ri.ProjectionError, match="the two bounds differ"):
            fn(pts, 8, 64, [0.1, 0.1])
        with pytest.raises(ri.ProjectionError, match="3 frames of 30000 x 30000"):
            fn(pts, 30000, 30000, list(rc.KITTI_INC), offsets=[0, 3, 6, 10])
        with pytest.raises(ri.ProjectionError, match=r"points2sensor must be \(2, 3, 4\)"):
            fn(pts, **ok, offsets=[0, 5, 10], points2sensor=np.zeros((3, 3, 4)))
        with pytest.raises(ri.ProjectionError, match="depths"):
            fn(pts, **ok, max_depth=float("inf"))
        with pytest.raises(ri.ProjectionError, match="data_type"):
            fn(pts, **ok, data_type="nuScenes")
    huge = torch.zeros((1, 4)).expand(2 ** 31, 4)                                         # no memory behind it
    with pytest.raises(ri.ProjectionError, match="2147483648 points"):
        ri.project_points(huge, **ok)


# ---- the rule's header on the host ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("project_check") / "project_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "host_check", "project_check.cpp")])
    return exe


def run_host(exe, c, tmp_path):
    kw = c.kw
    N = c.points.shape[0]
    off_arr = np.array([0, N], np.int64) if kw["offsets"] is None else kw["offsets"]
    F = off_arr.size - 1
    inc = np.asarray(kw["inclination"], np.float64)
    off, yaw = ri.convention(kw["data_type"], kw["sensor2ego"])
    T = kw["points2sensor"]
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<8i", N, F, kw["H"], kw["W"], inc.size, int(kw["wrap"]), int(T is not None), 0))
        f.write(struct.pack("<4d", off, yaw, kw["min_depth"], kw["max_depth"]))
        f.write(off_arr.astype(np.int64).tobytes()); f.write(inc.tobytes())
        if T is not None:
            f.write(np.ascontiguousarray(np.asarray(T, np.float64).reshape(F, -1, 4)[:, :3, :]).tobytes())
        f.write(c.points.tobytes())
    res = subprocess.run([exe, inp, out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "PROJECTCHECK ok" in res.stdout, res.stdout + res.stderr
    return np.fromfile(out, np.int32).reshape(N, 4)


def test_the_rule_header_on_the_host_against_the_twin(host_check, tmp_path):
    """Pixel, range bits and drop class of EVERY point of every case equal the twin's (the cases keep u and v off the rounding boundaries)."""
    cases = rc.all_cases_small()
    classes = set()
    for c in cases:
        got = run_host(host_check, c, tmp_path)
        t = c.twin
        assert np.array_equal(got[:, 3], t.drop.numpy().astype(np.int32)), c.key
        assert np.array_equal(got[:, :2], t.pixel.numpy()), c.key
        assert np.array_equal(got[:, 2].view(np.uint32), t.range_bits), c.key
        classes |= set(got[:, 3].tolist())
    assert classes == {ri.KEEP, ri.INVALID, ri.OUT_OF_RANGE, ri.OUT_OF_VIEW} and len(cases) >= 30


# ---- the round trip on this repository's ray grid ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("posed", [False, True], ids=["sensor_frame", "posed"])
@pytest.mark.parametrize("conv", rc.CONVENTIONS)
@pytest.mark.parametrize("H,W", rc.SIZES)
def test_every_pixels_own_point_comes_back_to_its_own_pixel(H, W, conv, posed):
    c = rc.grid(H, W, conv, 13, posed=posed)
    got = ri.project_points(torch.tensor(c.points), **c.kw)                                # CPU tensors: the twin
    assert got.depth.shape == (H, W) and got.depth.dtype == torch.float32 and got.mask.dtype == torch.bool and got.index.dtype == torch.int32
    assert torch.equal(got.index.reshape(-1), torch.arange(H * W, dtype=torch.int32))
    assert bool(got.mask.all())
    assert got.counts.tolist() == [H * W, 0, 0, 0, 0, H * W]
    r = torch.from_numpy(c.ranges).double()
    rel = float(((got.depth.reshape(-1).double() - r).abs() / r).max())
    print(f"RANGEIMAGE|round trip|{H} x {W}|{conv}|{'posed' if posed else 'sensor frame'}|margin {got.margin:.4f}|depth error {rel:.2e} of r")
    assert rel <= 1e-6
    assert torch.equal(got.intensity.reshape(-1), torch.tensor(c.points[:, 3]))


def test_the_round_trip_at_66_x_1030():
    c = rc.grid(66, 1030, "kitti_bounds", 13)
    assert torch.equal(c.twin.index.reshape(-1), torch.arange(66 * 1030, dtype=torch.int32)) and bool(c.twin.mask.all())
    r = torch.from_numpy(c.ranges).double()
    assert float(((c.twin.depth.reshape(-1).double() - r).abs() / r).max()) <= 1e-6


def test_without_wrap_the_kitti_grid_loses_exactly_column_0():
    for H, W in rc.SIZES:
        c = rc.grid(H, W, "kitti_bounds", 13, wrap=False)
        t = c.twin
        assert not bool(t.mask[:, 0].any()) and bool(t.mask[:, 1:].all())
        assert t.counts.tolist() == [H * W, 0, 0, H, 0, H * W - H]
        assert (t.drop.reshape(H, W)[:, 0] == ri.OUT_OF_VIEW).all() and (t.drop.reshape(H, W)[:, 1:] == ri.KEEP).all()
        w = rc.grid(H, W, "kitti_bounds", 13).twin                                        # the same points with the wrap
        assert torch.equal(w.depth[:, 1:], t.depth[:, 1:]) and bool(w.mask[:, 0].all())
    # the Waymo convention with a 0.3 rad sensor yaw loses three columns
    t = rc.grid(8, 64, "waymo_bounds_yaw", 13, wrap=False).twin
    assert (~t.mask).all(0).nonzero().reshape(-1).tolist() == [61, 62, 63] and int(t.counts[3]) == 24


# ---- constructed points -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wrap", [True, False], ids=["wrap", "no_wrap"])
@pytest.mark.parametrize("mode", ["bounds", "table"])
def test_constructed_points(mode, wrap):
    c = rc.constructed(mode, wrap)
    t = c.twin
    for k, (cls, col) in enumerate(c.expect):
        assert int(t.drop[k]) == cls, (k, c.points[k], cls, int(t.drop[k]))
        if col is not None:
            assert int(t.pixel[k, 0]) == col, (k, c.points[k])
    for k, row in c.edge_rows.items():
        assert int(t.pixel[k, 1]) == row, (k, c.points[k])
    n = lambda cls: sum(1 for e in c.expect if e[0] == cls)
    assert t.counts[:4].tolist() == [len(c.expect), n(ri.INVALID), n(ri.OUT_OF_RANGE), n(ri.OUT_OF_VIEW)]
    assert int(t.counts[0]) == int(t.counts[1:].sum())
    # (-2, 0, 0) and (-2, -0.0, 0) share column 0 under the wrap: the lower index wins the tie of equal ranges
    if wrap:
        hit = (t.index == 1).nonzero()
        assert hit.shape[0] == 1 and int(hit[0, 1]) == 0 and not bool((t.index == 2).any())


# ---- ties and occlusion ---------------------------------------------------------------------------------------------------------------------------------------

def test_a_thousand_points_on_one_ray_leave_one_pixel():
    c = rc.one_ray(1000)
    t = c.twin
    assert t.counts.tolist() == [1000, 0, 0, 0, 999, 1] and int(t.mask.sum()) == 1 and bool(t.mask[3, 20])
    k = int(np.argmin(c.ranges))
    assert int(t.index[3, 20]) == k and float(t.depth[3, 20]) == float(np.float32(np.sqrt((c.points[k, :3].astype(np.float64) ** 2).sum())))
    assert float(t.intensity[3, 20]) == float(c.points[k, 3])


def test_equal_ranges_go_to_the_lower_index():
    c = rc.one_ray(300, equal=True)
    t = c.twin
    assert t.counts.tolist() == [300, 0, 0, 0, 299, 1] and int(t.index[3, 20]) == 0 and float(t.intensity[3, 20]) == float(c.points[0, 3])
    assert len(set(t.range_bits.tolist())) == 1
    # the same points behind a nearer one that comes last
    pts = np.concatenate([c.points, c.points[:1] * np.float32(0.5)])
    t2 = ri.project_points_reference(pts, **c.kw)
    assert int(t2.index[3, 20]) == 300 and int(t2.counts[4]) == 300


def test_the_counts_add_up_on_every_case():
    for c in rc.all_cases_small() + [rc.random_cloud(N, F, 8, 64, "kitti_bounds", 11) for N in (1, 63, 64, 65, 255, 256, 257) for F in (1, 3)]:
        cnt = c.twin.counts.reshape(-1, ri.N_COUNTS)
        assert torch.equal(cnt[:, 0], cnt[:, 1:].sum(1)), c.key
        assert int(cnt[:, 5].sum()) == int(c.twin.mask.sum()) and int(cnt[:, 0].sum()) == c.points.shape[0]
        assert bool((c.twin.index[~c.twin.mask] == -1).all()) and bool((c.twin.depth[~c.twin.mask] == 0).all()) and bool((c.twin.intensity[~c.twin.mask] == 0).all())
        if c.kw["offsets"] is not None and c.kw["offsets"].size == 4:
            assert cnt[1].tolist() == [0] * 6                                             # the empty middle frame


def test_the_measured_margins_of_random_clouds():
    """The condition the comparisons rest on, on the clouds the issue names: 1 k and 200 k seeded points."""
    small = rc.random_cloud(1000, 1, 8, 64, "kitti_bounds", 11)
    large = rc.random_cloud(200_000, 1, 66, 1030, "kitti_bounds", 11)
    print(f"RANGEIMAGE|margin|1 k points 8 x 64: {small.twin.margin:.2e}|200 k points 66 x 1030: {large.twin.margin:.2e}")
    assert small.twin.margin >= rc.MARGIN and large.twin.margin >= rc.MARGIN


# ---- ingest ---------------------------------------------------------------------------------------------------------------------------------------------------

def check_sequence(root, ic):
    seq = sequence.load_sequence(root, device="cpu")
    rep = json.load(open(os.path.join(root, "ingest.json")))
    assert seq.meta["frames"] == [f.id for f in ic.frames] and (seq.meta["height"], seq.meta["width"]) == (ic.H, ic.W)
    assert [f["id"] for f in rep["frames"]] == [f.id for f in ic.frames]
    for f, r in zip(ic.frames, rep["frames"]):
        d, it, m = seq.frames.get_depth(f.id), seq.frames.get_intensity(f.id), seq.frames.get_mask(f.id)
        assert torch.equal(m, torch.from_numpy(f.mask)), f.id
        want = torch.from_numpy(f.depth).double()
        assert bool(((d.double() - want).abs() <= 1e-6 * want).all()), f.id
        assert torch.equal(it.view(torch.int32), torch.from_numpy(f.intensity).view(torch.int32)), f.id
        assert r["hidden"] == f.n_extra and r["out_of_view"] == f.n_out and r["invalid"] == 0 and r["out_of_range"] == 0
        assert r["pixels"] == int(f.mask.sum()) and r["points"] == f.points.shape[0] == sum(r[n] for n in ri.COUNT_NAMES[1:])
        z = np.load(os.path.join(root, "frames", f"{f.id:06d}.npz"))
        assert np.allclose(z["sensor2world"], f.sensor2world.astype(np.float32)) and z["inclination"].shape == (2,)
    assert rep["total"] == {n: sum(fr[n] for fr in rep["frames"]) for n in ri.COUNT_NAMES}
    assert (rep["height"], rep["width"], rep["data_type"], rep["max_depth"], rep["wrap"]) == (ic.H, ic.W, "KITTI", 80.0, True)
    assert rep["extent"] == seq.meta["extent"] == pytest.approx(max(float(f.depth.max()) for f in ic.frames), rel=1e-6)
    return seq, rep


def test_ingest_on_the_cpu(tmp_path):
    ic = rc.ingest_clouds()
    root = str(tmp_path / "seq")
    rep = ingest.ingest_point_clouds(root, ((f.id, f.points, f.sensor2world) for f in ic.frames), ic.H, ic.W, ic.inclination, device="cpu", batch=3, test_frames=[7])
    seq, on_disk = check_sequence(root, ic)
    assert rep == on_disk and rep["device"] == "cpu" and rep["batch"] == 3
    assert seq.test_frames == [7] and seq.train_frames == [3, 4, 5]
    assert rep["frames"][2] == {"id": 5, **{n: 0 for n in ri.COUNT_NAMES}}                # the empty frame
    assert sum(f.n_extra for f in ic.frames) > 100
    # the batch size does not show in the files
    root1 = str(tmp_path / "seq1")
    ingest.ingest_point_clouds(root1, ((f.id, f.points, f.sensor2world) for f in ic.frames), ic.H, ic.W, ic.inclination, device="cpu", batch=1, test_frames=[7])
    same_frames(root, root1, ic)


def same_frames(a, b, ic):
    for f in ic.frames:
        za, zb = (np.load(os.path.join(r, "frames", f"{f.id:06d}.npz")) for r in (a, b))
        assert sorted(za.files) == sorted(zb.files)
        for k in za.files:
            assert za[k].dtype == zb[k].dtype and za[k].tobytes() == zb[k].tobytes(), (f.id, k)
    assert json.load(open(os.path.join(a, "meta.json"))) == json.load(open(os.path.join(b, "meta.json")))


def test_the_command_line_on_bin_and_npy_inputs(tmp_path):
    ic = rc.ingest_clouds()
    as_bin, as_npy = tmp_path / "bin", tmp_path / "npy"
    as_bin.mkdir(); as_npy.mkdir()
    for f in ic.frames:
        f.points.tofile(str(as_bin / f"{f.id:06d}.bin"))
        np.save(str(as_npy / f"{f.id}.npy"), f.points)
    # text poses: frame 4 as 16 numbers, frame 5 without a row (it takes frame 4's), the others as 12
    with open(tmp_path / "poses.txt", "w") as fh:
        fh.write("# id, then the matrix row by row\n")
        for f in ic.frames:
            if f.id != 5:
                m = f.sensor2world if f.id == 4 else f.sensor2world[:3]
                fh.write(f"{f.id} " + " ".join(repr(float(x)) for x in m.reshape(-1)) + "\n")
    by4 = {f.id: f for f in ic.frames}
    np.save(str(tmp_path / "poses.npy"), np.stack([(by4[4] if f.id == 5 else f).sensor2world for f in ic.frames]))
    common = ["--height", str(ic.H), "--width", str(ic.W), "--inclination", repr(ic.inclination[0]), repr(ic.inclination[1]), "--device", "cpu", "--test-frames", "7"]
    out_bin, out_npy = str(tmp_path / "out_bin"), str(tmp_path / "out_npy")
    res = subprocess.run([sys.executable, "-m", "lidar_rt_amd.ingest", "--points", str(as_bin), "--poses", str(tmp_path / "poses.txt"), "--out", out_bin] + common,
                         capture_output=True, text=True, cwd=REPO, timeout=300)
    assert res.returncode == 0 and "1 frames took an earlier pose" in res.stdout, res.stdout + res.stderr
    assert ingest.main(["--points", str(as_npy), "--poses", str(tmp_path / "poses.npy"), "--out", out_npy, "--batch", "2"] + common) == 0
    same_frames(out_bin, out_npy, ic)
    ic.frames[2].sensor2world = by4[4].sensor2world                                          # what frame 5 was written with
    check_sequence(out_bin, ic)
    rep_bin, rep_npy = (json.load(open(os.path.join(r, "ingest.json"))) for r in (out_bin, out_npy))
    assert rep_bin["pose_taken_from"] == {"5": 4} and rep_npy["pose_taken_from"] == {}
    assert rep_bin["frames"] == rep_npy["frames"]
    assert ingest.main(["--points", str(as_bin), "--poses", str(tmp_path / "poses.txt"), "--out", str(tmp_path / "refused"), "--missing-pose", "error"] + common) == 2
    assert not os.path.exists(tmp_path / "refused")
