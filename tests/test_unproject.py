"""CPU tests of the point clouds of range images (lidar_rt_amd/unproject.py, include/lrt_unproject.h) and of the host half of
``python -m lidar_rt_amd.simulate``: the library's place in the build, the numpy twin against first principles, the round trip through the
projection twins as the independent yardstick, the rule header compiled by g++ against the twin bit for bit (also under the sanitizers),
and the edits, transform tables and files of simulate."""
import os
import re
import struct
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lidar_rt_amd import build as lrt_build, ingest, range_image as ri, sequence, simulate, sweep, sweep_project as sp, unproject as up
from lidar_rt_amd.training import RangeFrames
from tests import unproject_cases as uc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


# ---- 1. the library -------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def unproject_lib():
    return lrt_build.build_unproject()


def test_the_library_has_a_source_list_of_its_own():
    assert lrt_build.UNPROJECT_SOURCES == ["lrt_unproject.hip"]
    assert {"lrt_unproject_math.h", "lrt_device_guard.h"} <= set(lrt_build.UNPROJECT_HEADERS)
    lists = ("", "LOSS_", "GRIDCD_", "INIT_", "METRICS_", "ADAM_", "DENSIFY_", "PROJECT_", "SWEEP_", "REFINE_", "SWEEPPROJ_")
    others = sum((getattr(lrt_build, p + "SOURCES") + getattr(lrt_build, p + "HEADERS") for p in lists), [])
    assert not any("lrt_unproject" in f for f in others)
    hashes = {getattr(lrt_build, n)() for n in ("source_hash", "loss_source_hash", "gridcd_source_hash", "init_source_hash", "metrics_source_hash", "adam_source_hash",
                                                "densify_source_hash", "project_source_hash", "sweep_source_hash", "refine_source_hash", "sweepproj_source_hash")}
    assert lrt_build.unproject_source_hash() not in hashes
    assert os.path.basename(lrt_build.UNPROJECT_LIB) == "liblrt_unproject.so" and os.path.basename(lrt_build.UNPROJECT_STAMP) == "liblrt_unproject.srchash"
    src = open(lrt_build.__file__).read()
    product = src[src.index("def _build_product"):src.index("def _build_lib")]
    assert product.index("build_sweepproj(force, verbose)") < product.index("build_unproject(force, verbose)")
    assert "csrc/liblrt_unproject.so" in open(os.path.join(REPO, "setup.py")).read()
    body = src[src.index("def build_unproject"):src.index("EXT_SRC =")]
    assert "CODEGEN_FLAGS" in body and "resources.check(UNPROJECT_LIB)" in body
    assert "lrt_unproject" not in open(lrt_build.EXT_SRC).read()


def test_the_library_builds_and_exports_what_its_header_declares(unproject_lib):
    assert os.path.exists(unproject_lib) and not lrt_build.unproject_is_stale()
    assert open(lrt_build.UNPROJECT_STAMP).read().strip() == lrt_build.unproject_source_hash()
    hdr = open(os.path.join(REPO, "include", "lrt_unproject.h")).read()
    declared = set(re.findall(r"\b(lrt_unproject_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(up.EXPORTS), declared ^ set(up.EXPORTS)
    lib = up.load()
    exported = set(re.findall(r"\blrt_unproject_[a-z_]+\b", subprocess.run(["nm", "-D", "--defined-only", unproject_lib], capture_output=True, text=True, check=True).stdout))
    assert exported == declared, exported ^ declared
    const = lambda name: int(re.search(r"#define\s+%s\s+\(?(\d+)" % name, hdr).group(1))
    assert lib.lrt_unproject_abi_version() == const("LRT_UNPROJECT_ABI_VERSION") == up.ABI_VERSION
    assert const("LRT_UNPROJECT_N_COUNTS") == up.N_COUNTS == len(up.COUNT_NAMES) == 5 and const("LRT_UNPROJECT_BLOCK") == up.BLOCK == 256
    assert const("LRT_UNPROJECT_MAX_PIXELS") == up.MAX_PIXELS and const("LRT_UNPROJECT_MAX_WORKGROUPS") == up.MAX_WORKGROUPS == 2 ** 32 // 256 - 1
    mh = open(os.path.join(REPO, "lidar_rt_amd", "csrc", "lrt_unproject_math.h")).read()
    for name, v in (("UP_KEEP", up.KEEP), ("UP_INVALID", up.INVALID), ("UP_MASKED", up.MASKED), ("UP_OUT_OF_RANGE", up.OUT_OF_RANGE)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, mh).group(1)) == v
    # the workspace: 16 + 8 bytes per workgroup of 256 pixels of one frame and 32 per frame, each part rounded to 256; refused sizes are negative
    r256 = lambda x: (x + 255) // 256 * 256
    for F, H, W in ((1, 1, 1), (3, 5, 37), (3, 64, 2048), (16, 66, 1030)):
        G = F * ((H * W + 255) // 256)
        assert lib.lrt_unproject_work_bytes(F, H, W) == r256(16 * G) + r256(8 * G) + r256(32 * F)
    assert lib.lrt_unproject_work_bytes(0, 8, 64) < 0 and lib.lrt_unproject_work_bytes(2, 2 ** 15, 2 ** 15) < 0
    # the grid of a launch stays below 2^32 threads: at most 2^24 - 1 workgroups
    assert lib.lrt_unproject_work_bytes(2 ** 24 - 1, 1, 1) > 0 and lib.lrt_unproject_work_bytes(2 ** 24, 1, 1) < 0 and lib.lrt_unproject_work_bytes(2 ** 31 - 1, 1, 1) < 0
    assert lib.lrt_unproject_work_bytes(2 ** 24 - 1, 1, 100) > 0 and lib.lrt_unproject_work_bytes(2 ** 24, 1, 100) < 0     # fewer than 2^31 pixels, one workgroup too many
    assert lib.lrt_unproject_work_bytes(2 ** 15 - 1, 2 ** 8, 2 ** 8) > 0


def test_the_resource_gate_passes_on_the_three_kernels(unproject_lib):
    from lidar_rt_amd import resources
    res = resources.check(unproject_lib)
    own = {n for n in res if resources.is_own_kernel(n)}
    assert {n.split("(")[0] for n in own} == {"k_up_count", "k_up_scan", "k_up_write"}, own


# ---- 2. the twin against first principles ---------------------------------------------------------------------------------------------------------------

def _frames_of(c, F):
    rf = RangeFrames()
    for f in range(F):
        rf.add_frame(f, torch.tensor(c.o[f]), torch.tensor(c.d[f]), torch.tensor(c.depth[f]), torch.tensor(c.kw["intensity"][f]), torch.ones(c.H, c.W, dtype=torch.bool))
    return rf


@pytest.mark.parametrize("H,W", [(5, 37), (8, 64)])
def test_world_mode_is_inverse_projection_with_range_bit_for_bit(H, W):
    c = uc.random_frames(3, H, W, "random", "keep", "none", empty_middle=False)
    rf = _frames_of(c, 3)
    kept = c.twin.cls == up.KEEP
    off = c.twin.offsets.tolist()
    for f in range(3):
        want = rf.inverse_projection_with_range(f, torch.tensor(c.depth[f]), kept[f])
        got = c.twin.points[off[f]:off[f + 1]]
        assert got[:, :3].numpy().tobytes() == want.numpy().tobytes()
        assert torch.equal(got[:, 3], torch.tensor(c.kw["intensity"][f]).reshape(-1)[kept[f].reshape(-1)])
        assert torch.equal(c.twin.pixel[off[f]:off[f + 1]].long(), torch.nonzero(kept[f].reshape(-1)).squeeze(1))
    assert off[-1] > 0 and not c.twin.points[off[-1]:].any()


def test_the_precedence_of_the_classes_on_constructed_pixels():
    nan, inf = float("nan"), float("inf")
    #           depth  keep  raydrop  class
    rows = [(nan, 0, 0.1, up.INVALID),             # invalid before masked
            (inf, 1, 0.1, up.INVALID),
            (0.0, 1, 0.1, up.OUT_OF_RANGE),        # "no return"
            (10.0, 1, nan, up.MASKED),             # a NaN ray-drop is masked
            (10.0, 1, 0.4, up.MASKED),             # raydrop == ratio
            (10.0, 1, float(np.nextafter(np.float32(0.4), np.float32(0))), up.KEEP),
            (0.0, 0, 0.1, up.MASKED),              # masked before out_of_range
            (90.0, 1, 0.9, up.MASKED),
            (90.0, 1, 0.1, up.OUT_OF_RANGE),
            (80.0, 1, 0.1, up.KEEP),               # min < depth <= max
            (0.5, 1, 0.1, up.OUT_OF_RANGE),
            (-3.0, 1, 0.1, up.OUT_OF_RANGE)]
    n = len(rows)
    depth = torch.tensor([r[0] for r in rows]).reshape(1, n)
    keep = torch.tensor([r[1] for r in rows], dtype=torch.uint8).reshape(1, n)
    drop = torch.tensor([r[2] for r in rows]).reshape(1, n)
    o = torch.zeros(1, n, 3)
    d = torch.tensor([0.0, 0.6, 0.8]).expand(1, n, 3).contiguous()
    pc = up.points_from_range_images(depth, o, d, keep=keep, raydrop=drop, raydrop_ratio=0.4, min_depth=0.5, max_depth=80.0)     # CPU tensors: the twin
    ref = up.points_from_range_images_reference(depth, o, d, keep=keep, raydrop=drop, raydrop_ratio=0.4, min_depth=0.5, max_depth=80.0)
    assert ref.cls.reshape(-1).tolist() == [r[3] for r in rows]
    assert pc.counts.tolist() == ref.counts.tolist() == [n, 2, 4, 4, 2] and pc.counts.dim() == 1
    assert pc.pixel[:2].tolist() == [5, 9] and pc.offsets.tolist() == [0, 2]
    one = pc.trim()
    assert one.points.shape == (2, 4) and one.points[1].tolist() == [0.0, float(np.float32(0.6) * np.float32(80.0)), float(np.float32(0.8) * np.float32(80.0)), 0.0]
    # a non-finite origin or direction is invalid whatever else holds
    o2 = o.clone(); o2[0, 5, 1] = nan
    d2 = d.clone(); d2[0, 9, 0] = inf
    assert up.points_from_range_images_reference(depth, o2, d2, keep=keep, raydrop=drop, min_depth=0.5, max_depth=80.0).counts.tolist() == [n, 4, 4, 4, 0]


@pytest.mark.parametrize("pattern", uc.PATTERNS)
@pytest.mark.parametrize("use", uc.USES)
def test_offsets_and_counts_are_consistent(pattern, use):
    c = uc.random_frames(3, 8, 64, pattern, use, "frame")
    t = c.twin
    cnt = t.counts.numpy()
    assert (cnt[:, 0] == 8 * 64).all() and (cnt[:, 1:].sum(1) == cnt[:, 0]).all()
    assert t.offsets.tolist() == [0] + np.cumsum(cnt[:, 4]).tolist()
    assert cnt[1, 4] == 0                                                     # the empty frame between two others
    finite = np.isfinite(c.depth) & np.isfinite(c.o).all(-1) & np.isfinite(c.d).all(-1)
    in_range = (c.depth > 0.5) & (c.depth <= 80.0)
    assert np.array_equal(t.cls.numpy() == up.KEEP, finite & c.want & in_range)
    assert cnt[:, 1].tolist() == (~finite).reshape(3, -1).sum(1).tolist() == [4, 4, 4]
    if pattern == "none":
        assert cnt[:, 4].tolist() == [0, 0, 0] and cnt[:, 3].tolist() == [0, 0, 0]
    if pattern == "all":
        assert cnt[0, 4] == 8 * 64 - 4 - 4 and cnt[0, 2] == 0 and cnt[0, 3] == 4     # 0, 85, 0.25 and -1 m
    if pattern == "last":
        assert cnt[:, 4].tolist() == [1, 0, 1] and t.pixel[:2].tolist() == [511, 511]
    per = [SimpleNamespace(points=t.points[a:b], pixel=t.pixel[a:b]) for a, b in zip(t.offsets[:-1].tolist(), t.offsets[1:].tolist())]
    for f, (got, want) in enumerate(zip(t.trim(), per)):
        assert torch.equal(got.points, want.points) and torch.equal(got.pixel, want.pixel)
        assert (got.pixel[1:] > got.pixel[:-1]).all()                         # row-major within a frame


def test_refused_arguments():
    c = uc.random_frames(3, 5, 37)
    dep, o, d = (torch.tensor(x) for x in (c.depth, c.o, c.d))
    E = up.UnprojectError
    for kw in (dict(world2out=np.zeros((2, 3, 4))), dict(world2out=np.zeros((3, 36, 3, 4))), dict(world2out=np.zeros((3, 3, 3))), dict(keep=torch.ones(3, 5, 36)),
               dict(intensity=torch.ones(5, 37)), dict(min_depth=-1.0), dict(min_depth=5.0, max_depth=5.0), dict(max_depth=float("inf")),
               dict(raydrop=dep, raydrop_ratio=float("nan")), dict(workspace=torch.zeros(1 << 16, dtype=torch.uint8))):
        with pytest.raises(E):
            up.points_from_range_images(dep, o, d, **kw)
    with pytest.raises(E):
        up.points_from_range_images(dep, o[..., :2], d)
    with pytest.raises(E):
        up.points_from_range_images(c.depth, o, d)                            # numpy goes to the twin by name
    with pytest.raises(E, match="int32"):
        up.points_from_range_images_reference(torch.zeros(1).expand(2 ** 31, 1, 1), torch.zeros(1).expand(2 ** 31, 1, 1, 3), torch.zeros(1).expand(2 ** 31, 1, 1, 3))


# ---- 3. the round trip: the independent yardstick ----------------------------------------------------------------------------------------------------------

def _back(g, points, twist=None):
    kw = dict(data_type=g.conv["data_type"], sensor2ego=g.conv["sensor2ego"], max_depth=100.0)
    if twist is None:
        return ri.project_points_reference(points, g.H, g.W, g.conv["inclination"], **kw), None
    img = sp.project_points_sweep_reference(points, g.H, g.W, g.conv["inclination"], twist, tau=g.tau, **kw)
    return img, int(img.counts[sp.COUNT_NAMES.index("unseen")])


def _own_pixels(img, g, names):
    n = g.H * g.W
    assert bool(img.mask.all()) and int(img.counts[names.index("hidden")]) == 0 and int(img.counts[names.index("pixels")]) == n
    assert torch.equal(img.index.reshape(-1), torch.arange(n, dtype=torch.int32))


@pytest.mark.parametrize("H,W", uc.ROUND_TRIP_SIZES)
def test_sensor_frame_points_return_to_their_pixels_and_depths(H, W):
    """|depth' - depth| <= 8 * 2^-24 * depth: d is unit to within its normalisation's three roundings, the point and the range are rounded once
    each.  Measured maximum over these grids: 2.90 (66 x 1030, Waymo bounds).  The float32 world route at this pose does NOT meet it (measured
    9 at 1 x 1, 35 at 2 x 3, 350 .. 1030 from 5 x 37 on): that is why the float64 rule exists."""
    for cn in uc.conventions(H):
        g = uc.static_grid(H, W, cn)
        pc = up.points_from_range_images_reference(g.depth, g.o, g.d, world2out=uc.sensor_table(g, "sensor"))
        assert pc.counts.tolist() == [H * W, 0, 0, 0, H * W]
        img, _ = _back(g, pc.points)
        _own_pixels(img, g, ri.COUNT_NAMES)
        e = uc.round_trip_error(img.depth, g.depth)
        print(f"round trip {H} x {W} {cn}: {e:.2f} x 2^-24 depth")
        assert e <= uc.BOUND, (cn, e)
        world = up.points_from_range_images_reference(g.depth, g.o, g.d)
        back = ri.project_points_reference(world.points, H, W, g.conv["inclination"], points2sensor=np.linalg.inv(g.pose)[None], data_type=g.conv["data_type"],
                                           sensor2ego=g.conv["sensor2ego"], max_depth=100.0)
        ew = uc.round_trip_error(back.depth, g.depth)
        print(f"float32 world route {H} x {W} {cn}: {ew:.1f} x 2^-24 depth")
        assert bool(back.mask.all()) and ew > uc.BOUND, (cn, ew)


@pytest.mark.parametrize("frame", ["raw", "sensor"])
@pytest.mark.parametrize("H,W", uc.ROUND_TRIP_SIZES)
def test_the_round_trip_under_a_twist(H, W, frame):
    """The sweep-ray twin's grid under uc.TWIST, its rays rounded to float32 as the operator's are.  ``raw`` points are in their own column's frame:
    the static projection brings them back; ``sensor`` points are motion compensated: the sweep projection does, with nothing unseen.  Measured
    maximum: 2.0.  The column tables take the rays' float32 origins (``column_transforms(origins=)``): with the exact column origins instead,
    the 0.1 mm by which float32 misplaces an origin 1.6 km out shows as 100 .. 1030 x 2^-24 depth."""
    for cn in uc.conventions(H):
        g = uc.sweep_grid(H, W, cn)
        pc = up.points_from_range_images_reference(g.depth, g.o, g.d, world2out=uc.sensor_table(g, frame))
        assert pc.counts.tolist() == [H * W, 0, 0, 0, H * W]
        img, unseen = _back(g, pc.points, g.twist if frame == "sensor" else np.zeros(6))
        assert unseen == 0
        _own_pixels(img, g, sp.COUNT_NAMES)
        e = uc.round_trip_error(img.depth, g.depth)
        print(f"round trip under a twist {H} x {W} {cn} {frame}: {e:.2f} x 2^-24 depth")
        assert e <= uc.BOUND, (cn, e)


def test_column_transforms_invert_the_column_poses():
    g = uc.sweep_grid(8, 64, "kitti_bounds")
    Rc, tc = sweep.column_poses_reference(torch.tensor(g.pose[:3])[None], torch.tensor(g.twist)[None], torch.tensor(g.tau))
    Tc = np.tile(np.eye(4), (64, 1, 1))
    Tc[:, :3, :3], Tc[:, :3, 3] = Rc[0].numpy(), tc[0].numpy()
    raw = simulate.column_transforms("raw", g.pose, g.twist, g.tau)
    assert raw.shape == (64, 3, 4) and raw.dtype == np.float64
    full = np.tile(np.eye(4), (64, 1, 1)); full[:, :3] = raw
    assert np.abs(full @ Tc - np.eye(4)).max() <= 1e-12
    # independent of column_poses_reference: P Exp(tau xi) by scipy-free series of the 4 x 4 matrix exponential
    def expm(A):
        out, term = np.eye(4), np.eye(4)
        for k in range(1, 30):
            term = term @ A / k
            out = out + term
        return out
    P = np.eye(4); P[:3] = g.pose[:3]
    for w in range(64):
        X = np.zeros((4, 4)); r, p = g.twist[:3], g.twist[3:]
        X[:3, :3] = [[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]]; X[:3, 3] = r
        assert np.abs(full[w] @ (P @ expm(g.tau[w] * X)) - np.eye(4)).max() <= 1e-12
    sensor = simulate.column_transforms("sensor", g.pose)
    assert sensor.shape == (3, 4) and np.abs(sensor @ P - np.eye(4)[:3]).max() <= 1e-12
    assert simulate.column_transforms("world", g.pose) is None
    # with the rays' origins: every column's own origin maps to the exact origin's place
    for frame in ("raw", "sensor"):
        T = simulate.column_transforms(frame, g.pose, g.twist, g.tau, origins=g.o[0])
        o = g.o[0].double().numpy()
        at = np.einsum("wij,wj->wi", T[:, :, :3], o) + T[:, :, 3]
        exact = np.zeros((64, 3)) if frame == "raw" else (sensor[None, :, :3] @ tc[0].numpy()[..., None])[..., 0] + sensor[:, 3]
        assert np.abs(at - exact).max() <= 1e-12
    with pytest.raises(simulate.SimulateError, match="raw"):
        simulate.column_transforms("raw", g.pose)
    with pytest.raises(simulate.SimulateError):
        simulate.column_transforms("ego", g.pose)


# ---- 4. the rule's header on the host ----------------------------------------------------------------------------------------------------------------------

CHECK_SRC = os.path.join(HERE, "host_check", "unproject_check.cpp")


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("unproject_check") / "unproject_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, CHECK_SRC])
    return exe


@pytest.fixture(scope="module")
def host_check_sanitized(tmp_path_factory):
    """The same stand-alone program under the address and undefined-behaviour sanitizers; None where g++ cannot link their runtime."""
    d = tmp_path_factory.mktemp("unproject_check_san")
    probe = str(d / "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + flags + ["-o", str(d / "probe"), probe], capture_output=True).returncode != 0:
        return None
    exe = str(d / "unproject_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", exe, CHECK_SRC])
    return exe


def run_host(exe, c, tmp_path):
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    T = c.kw["world2out"]
    tmode = 0 if T is None else (1 if T.ndim == 3 else 2)
    with open(inp, "wb") as f:
        f.write(struct.pack("<6i", c.F, c.H, c.W, int(c.kw["keep"] is not None), int(c.kw["raydrop"] is not None), tmode))
        f.write(struct.pack("<3d", c.kw["raydrop_ratio"], c.kw["min_depth"], c.kw["max_depth"]))
        f.write(c.depth.tobytes()); f.write(c.o.tobytes()); f.write(c.d.tobytes())
        if c.kw["keep"] is not None:
            f.write(np.ascontiguousarray(c.kw["keep"], np.uint8).tobytes())
        if c.kw["raydrop"] is not None:
            f.write(c.kw["raydrop"].tobytes())
        if T is not None:
            f.write(np.ascontiguousarray(T[..., :3, :], np.float64).tobytes())
    res = subprocess.run([exe, inp, out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "UNPROJECTCHECK ok" in res.stdout, res.stdout + res.stderr
    return np.fromfile(out, np.int32).reshape(c.F * c.H * c.W, 4)


def compare_host(exe, cases, tmp_path):
    classes = set()
    for c in cases:
        got = run_host(exe, c, tmp_path)
        cls = c.twin.cls.numpy().reshape(-1)
        assert np.array_equal(got[:, 0], cls), c.key
        n = int(c.twin.offsets[-1])
        kept = got[got[:, 0] == up.KEEP]
        assert kept[:, 1:].astype(np.int32).tobytes() == np.ascontiguousarray(c.twin.points[:n, :3].numpy()).view(np.int32).tobytes(), c.key
        assert not got[got[:, 0] != up.KEEP][:, 1:].any()
        classes |= set(cls.tolist())
    return classes


def test_the_rule_header_on_the_host_against_the_twin(host_check, tmp_path):
    """Class and point bits of EVERY pixel of every small case equal the twin's: g++ -ffp-contract=off and numpy round alike."""
    cases = uc.small_cases()
    assert compare_host(host_check, cases, tmp_path) == {up.KEEP, up.INVALID, up.MASKED, up.OUT_OF_RANGE} and len(cases) >= 100
    assert {(c.H, c.W) for c in cases} >= {(1, 1), (2, 3), (5, 37), (8, 64)}
    assert {None if c.kw["world2out"] is None else c.kw["world2out"].ndim for c in cases} == {None, 3, 4}
    # the far grids too: the float64 rule where it matters
    for H, W in ((5, 37), (8, 64)):
        g = uc.sweep_grid(H, W, "kitti_bounds")
        for frame in ("raw", "sensor"):
            T = uc.sensor_table(g, frame)[None]
            depth, o, d = (x[None].numpy() for x in (g.depth, g.o, g.d))
            kw = dict(intensity=None, keep=None, raydrop=None, raydrop_ratio=0.4, world2out=T, min_depth=0.0, max_depth=100.0)
            twin = up.points_from_range_images_reference(depth, o, d, **kw)
            compare_host(host_check, [SimpleNamespace(key=("far", H, W, frame), F=1, H=H, W=W, depth=depth, o=o, d=d, kw=kw, twin=twin)], tmp_path)


def test_the_host_program_under_the_sanitizers(host_check_sanitized, tmp_path):
    """A stand-alone host program: nothing is loaded into Python, nothing is preloaded."""
    if host_check_sanitized is None:
        pytest.skip("g++ cannot link the sanitizer runtime here")
    assert compare_host(host_check_sanitized, uc.small_cases(), tmp_path) == {up.KEEP, up.INVALID, up.MASKED, up.OUT_OF_RANGE}


# ---- 5. the host half of simulate ----------------------------------------------------------------------------------------------------------------------------

def _scene(n_actors=3, frames=(0, 1, 2)):
    rng = np.random.default_rng(4)
    assets = [SimpleNamespace(name="background", bounding_box=None)]
    for a in range(n_actors):
        tb = sequence.TrackingBox([4.6, 2.1, 1.8], "cpu")
        for f in frames:
            q = rng.standard_normal(4).astype(np.float32); q /= np.linalg.norm(q)
            tb.frame[f] = (torch.tensor(rng.uniform(-20, 20, 3).astype(np.float32)), torch.tensor(q).reshape(1, 4), None, None)
        assets.append(SimpleNamespace(name=f"actor_{a:02d}", bounding_box=tb))
    return assets


def _rot(q):
    w, x, y, z = (float(v) for v in q.reshape(4))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def test_apply_edits_removes_and_moves_actors():
    assets = _scene()
    before = {a: dict(g.bounding_box.frame) for a, g in enumerate(assets[1:])}
    out, decomp, rep = simulate.apply_edits(assets, remove_actor=[1])
    assert [g.name for g in out] == ["background", "actor_00", "actor_02"] and decomp is False and rep["removed"] == [1] and len(assets) == 4
    out, decomp, rep = simulate.apply_edits(assets, move_actor=[[2, 1.0, -2.0, 0.5, 30.0]], only="actors")
    assert decomp == "object" and [g.name for g in out] == [g.name for g in assets] and out[3] is not assets[3] and out[1] is assets[1]
    th = np.radians(30.0)
    Rz = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    for f in (0, 1, 2):
        t0, q0 = before[2][f][:2]
        t1, q1 = out[3].bounding_box.frame[f][:2]
        assert q1.shape == (1, 4) and np.allclose(t1.numpy(), t0.numpy() + np.array([1.0, -2.0, 0.5], np.float32), atol=0, rtol=1e-7)
        assert np.abs(_rot(q1) - Rz @ _rot(q0)).max() < 1e-6                  # a rotation about world z, composed on the left
        assert torch.equal(assets[3].bounding_box.frame[f][0], t0) and torch.equal(assets[3].bounding_box.frame[f][1], q0)     # the scene's own table is not written to
    assert torch.equal(out[3].bounding_box.max_xyz, assets[3].bounding_box.max_xyz)
    # the identity move leaves every number as it is
    out, _, _ = simulate.apply_edits(assets, move_actor=[[0, 0.0, 0.0, 0.0, 0.0]])
    for f in (0, 1, 2):
        assert torch.equal(out[1].bounding_box.frame[f][0], before[0][f][0]) and torch.equal(out[1].bounding_box.frame[f][1], before[0][f][1])
    assert simulate.apply_edits(assets, only="background")[1] == "background"
    for kw in (dict(remove_actor=[3]), dict(remove_actor=[-1]), dict(move_actor=[[7, 0, 0, 0, 0]]), dict(move_actor=[[0.5, 0, 0, 0, 0]])):
        with pytest.raises(simulate.SimulateError, match=r"0 \.\. 2"):
            simulate.apply_edits(assets, **kw)
    for kw in (dict(remove_actor=[1], move_actor=[[1, 0, 0, 0, 0]]), dict(move_actor=[[1, 0, 0, 0]]), dict(move_actor=[[1, float("nan"), 0, 0, 0]]), dict(only="object"),
               dict(remove_actor=[0, 1, 2], only="actors")):
        with pytest.raises(simulate.SimulateError):
            simulate.apply_edits(assets, **kw)
    with pytest.raises(simulate.SimulateError, match="no actors"):
        simulate.apply_edits(assets[:1], remove_actor=[0])


def _clouds():
    c = uc.random_frames(3, 8, 64, "random", "both", "frame")
    return c, c.twin


@pytest.mark.parametrize("fmt", ["bin", "npy"])
def test_written_clouds_and_poses_read_back_through_ingest(fmt, tmp_path):
    c, pc = _clouds()
    ids = [4, 9, 17]
    poses = {i: uc.far_pose(seed=i) for i in ids}
    out = str(tmp_path / "out")
    paths = simulate.write_clouds(out, ids, pc, 64, poses, fmt=fmt)
    assert [os.path.basename(p) for p in paths] == [f"{i:06d}.{fmt}" for i in ids]
    found = ingest.list_points(out)
    assert [i for i, _ in found] == ids
    off = pc.offsets.tolist()
    for k, (i, p) in enumerate(found):
        assert np.array_equal(ingest.read_points(p), pc.points[off[k]:off[k + 1]].numpy())
    back = ingest.read_poses(os.path.join(out, "poses.txt"), ids)
    assert sorted(back) == ids and all(np.array_equal(back[i], poses[i]) for i in ids)
    # the six-field rows: ring and the column's firing time
    tau = {i: sweep.column_times(64).numpy() + 0.001 * i for i in ids}
    six = str(tmp_path / "six")
    paths = simulate.write_clouds(six, ids, pc, 64, None, fmt=fmt, fields="xyzirt", tau=tau)
    assert not os.path.exists(os.path.join(six, "poses.txt"))
    for k, p in enumerate(paths):
        a = np.load(p) if fmt == "npy" else np.fromfile(p, np.float32).reshape(-1, 6)
        px = pc.pixel[off[k]:off[k + 1]].numpy()
        assert np.array_equal(a[:, :4], pc.points[off[k]:off[k + 1]].numpy()) and np.array_equal(a[:, 4], px // 64)
        assert np.array_equal(a[:, 5], tau[ids[k]].astype(np.float32)[px % 64])
    for kw in (dict(fmt="pcd"), dict(fields="xyz")):
        with pytest.raises(simulate.SimulateError):
            simulate.write_clouds(six, ids, pc, 64, **kw)
    with pytest.raises(simulate.SimulateError):
        simulate.write_clouds(six, ids[:2], pc, 64)


def test_clouds_from_renders_on_cpu_tensors_and_the_torch_expression_agree():
    c = uc.random_frames(3, 8, 64, "random", "raydrop", "none", empty_middle=False)
    rf = _frames_of(c, 3)
    renders = {f: {"depth": torch.tensor(c.depth[f])[..., None], "intensity": torch.tensor(c.kw["intensity"][f])[..., None], "raydrop": torch.tensor(c.kw["raydrop"][f])[..., None]}
               for f in range(3)}
    a = simulate.clouds_from_renders(renders, rf, [0, 1, 2], uc.RATIO, None, 0.5, 80.0)
    b = simulate.clouds_from_renders(renders, rf, [0, 1, 2], uc.RATIO, None, 0.5, 80.0, backend="torch")
    n = int(c.twin.offsets[-1])
    for pc in (a, b):
        assert torch.equal(pc.offsets, c.twin.offsets) and torch.equal(pc.counts, c.twin.counts)
        assert pc.points[:n].numpy().tobytes() == c.twin.points[:n].numpy().tobytes() and torch.equal(pc.pixel[:n], c.twin.pixel[:n])
    T = uc.transforms("column", 3, 64, 2)
    t = simulate.clouds_from_renders(renders, rf, [2, 0], uc.RATIO, [T[0], T[1]], 0.5, 80.0)
    ref = up.points_from_range_images_reference(c.depth[[2, 0]], c.o[[2, 0]], c.d[[2, 0]], intensity=c.kw["intensity"][[2, 0]], raydrop=c.kw["raydrop"][[2, 0]],
                                                raydrop_ratio=uc.RATIO, world2out=T[:2], min_depth=0.5, max_depth=80.0)
    assert torch.equal(t.points, ref.points) and torch.equal(t.offsets, ref.offsets)
    with pytest.raises(simulate.SimulateError):
        simulate.clouds_from_renders(renders, rf, [0], uc.RATIO, [T[0]], backend="torch")


def _cpu_sequence(tmp_path, n=4, H=8, W=64):
    """A sequence directory of n empty frames on a gentle curve, loaded on the CPU."""
    from lidar_rt_amd import scenes
    data = str(tmp_path / "seq")
    z = np.zeros((H, W), np.float32)
    poses = {f: np.asarray(scenes.pose_matrix((0.5 * f, 0.02 * f * f, 1.7), yaw=0.01 * f), np.float32).astype(np.float64) for f in range(n)}
    sequence.write_sequence(data, [{"id": f, "depth": z, "intensity": z, "mask": z > 0, "inclination": [-0.4, 0.03], "sensor2world": poses[f]} for f in range(n)])
    return data, poses


def test_build_sensor_replaces_poses_and_rederives_the_twists(tmp_path):
    data, poses = _cpu_sequence(tmp_path)
    ids = [0, 1, 2, 3]
    seq = sequence.load_sequence(data, "cpu")
    assert simulate.build_sensor(seq, ids) is seq.frames                      # nothing asked for: the sequence's own sensor
    new = {1: uc.far_pose(seed=7), 3: uc.far_pose(seed=9)}
    rf = simulate.build_sensor(seq, ids, poses=new)
    for f in ids:
        want = new.get(f, poses[f])
        assert np.array_equal(rf.pose_meta[f][1].double().numpy(), want) and f not in rf.sweep_meta
        o, d = RangeFrames.range_rays(8, 64, (-0.4, 0.03), torch.tensor(want, dtype=torch.float32))
        assert torch.equal(rf.get_range_rays(f)[0], o) and torch.equal(rf.get_range_rays(f)[1], d)
        assert rf.get_depth(f).shape == (8, 64) and not rf.get_mask(f).any()
    # the ids stay: a pose file may list any of them, and only of them
    with pytest.raises(simulate.SimulateError, match=r"\[5\]"):
        simulate.build_sensor(seq, ids, poses={5: np.eye(4)})
    # through a pose file, as the command reads it
    simulate.write_poses(str(tmp_path / "new.txt"), new)
    back = ingest.read_poses(str(tmp_path / "new.txt"), ids)
    assert sorted(back) == [1, 3] and all(np.array_equal(back[k], new[k]) for k in back)
    # under --sweep poses the twists follow the replaced trajectory; another grid takes its own column times
    moved = {f: poses[f].copy() for f in (1, 2)}
    moved[1][:3, 3] += (0.0, 0.3, 0.0); moved[2][:3, 3] += (0.0, 0.9, 0.0)
    sw = sequence.load_sequence(data, "cpu", sweep="poses", sweep_fraction=0.8)
    rf = simulate.build_sensor(sw, ids, width=48, height=6, poses=moved, sweep_ref=0.0, sweep_direction="ccw", sweep_fraction=0.8)
    want = sweep.twists_from_poses({f: moved.get(f, poses[f]) for f in ids}, 0.8)
    old = sweep.twists_from_poses(poses, 0.8)
    for f in ids:
        xi, tau = rf.sweep_meta[f]
        assert np.array_equal(xi.numpy(), want[f].astype(np.float32)) and tau.shape == (48,)
        assert torch.equal(tau, sweep.column_times(48, 0.0, "ccw").to(torch.float32))
        assert rf.get_range_rays(f)[0].shape == (6, 48, 3)
    assert not np.allclose(want[0], old[0]) and not np.allclose(want[1], old[1]) and np.allclose(want[3], want[2])
    # without replaced poses the stored twists are kept, and a mount carries them into the mounted frame: Exp(xi') = M^-1 Exp(xi) M
    M = simulate.mount_matrix([0.2, 0.0, 0.3, 0.0, 0.01, 0.1])
    rf = simulate.build_sensor(sw, ids, mount=[0.2, 0.0, 0.3, 0.0, 0.01, 0.1])
    for f in ids:
        assert np.abs(rf.pose_meta[f][1].double().numpy() - poses[f] @ M).max() < 1e-6
        xi0 = sw.frames.sweep_meta[f][0].double()
        R0, t0 = sweep._exp64(xi0[None]); R1, t1 = sweep._exp64(rf.sweep_meta[f][0].double()[None])
        E0, E1 = np.eye(4), np.eye(4)
        E0[:3, :3], E0[:3, 3], E1[:3, :3], E1[:3, 3] = R0[0].numpy(), t0[0].numpy(), R1[0].numpy(), t1[0].numpy()
        assert np.abs(E1 - np.linalg.inv(M) @ E0 @ M).max() < 1e-6             # the twist is held in float32
        assert torch.equal(rf.sweep_meta[f][1], sw.frames.sweep_meta[f][1])


def test_simulate_refuses_before_it_touches_a_device(tmp_path):
    data = str(tmp_path / "seq")
    z = np.zeros((8, 64), np.float32)
    sequence.write_sequence(data, [{"id": 0, "depth": z, "intensity": z, "mask": z > 0, "inclination": [-0.4, 0.03], "sensor2world": np.eye(4)}])
    table = str(tmp_path / "beams.txt")
    np.savetxt(table, np.linspace(-0.4, 0.03, 7))
    common = dict(data=data, ckpt=str(tmp_path / "none.pth"), out=str(tmp_path / "out"))
    with pytest.raises(simulate.SimulateError, match="raw"):
        simulate.simulate(frame="raw", **common)
    with pytest.raises(simulate.SimulateError, match="7 angles"):
        simulate.simulate(inclination_table=table, **common)
    with pytest.raises(simulate.SimulateError, match="7 angles"):
        simulate.simulate(inclination_table=table, height=9, **common)
    with pytest.raises(simulate.SimulateError, match="monotonic"):
        simulate.simulate(inclination=[0.1, 0.1], **common)
    with pytest.raises(simulate.SimulateError):
        simulate.simulate(inclination=[0.1, 0.2], inclination_table=table, **common)
    with pytest.raises(simulate.SimulateError):
        simulate.simulate(frame="ego", **common)
    with pytest.raises(simulate.SimulateError):
        simulate.simulate(fmt="pcd", **common)
    assert simulate.main(["--data", data, "--ckpt", "x", "--out", str(tmp_path / "o2"), "--frame", "raw"]) == 2 and not os.path.exists(tmp_path / "o2")
    assert simulate.read_inclination_table(table, 7) == pytest.approx(np.linspace(-0.4, 0.03, 7).tolist())
    M = simulate.mount_matrix([1.0, 2.0, 3.0, 0.0, 0.0, np.pi / 2])
    assert np.allclose(M, [[0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]], atol=1e-15)
    with pytest.raises(simulate.SimulateError):
        simulate.mount_matrix([1.0, 2.0, 3.0])
