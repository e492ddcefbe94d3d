"""TSDF fusion under the sweep model on the CPU: the twin against mesh.integrate_reference at zero motion, the rule header compiled for the host
against the twin bit for bit (and once under the address and undefined-behaviour sanitizers over hostile inputs), the accuracy of the fused wall
against the static fusion, accumulation, the command lines, and the library's build entry, exports, resource gate and refused arguments."""
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

from lidar_rt_amd import mesh, raycast, range_image as ri, sweep_fuse as sf
from tests import mesh_cases as mcs
from tests import sweep_fuse_cases as sfc
from tests import sweep_project_cases as spc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_check", "sweepfuse_check.cpp")


def bits(t):
    return t.numpy().reshape(-1).view(np.uint32) if t.dtype == torch.float32 else t.numpy().reshape(-1)


def same_grid(g, w):
    assert np.array_equal(bits(g.tsdf), bits(w.tsdf)), int((bits(g.tsdf) != bits(w.tsdf)).sum())
    assert np.array_equal(bits(g.weight), bits(w.weight))
    assert (g.intensity is None) == (w.intensity is None)
    if w.intensity is not None:
        assert np.array_equal(bits(g.intensity), bits(w.intensity))


# ---- 1. zero motion is the static fusion ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", sfc.SIZES)
@pytest.mark.parametrize("conv", sfc.CONVENTIONS)
@pytest.mark.parametrize("dims", sfc.GRIDS)
def test_without_motion_the_twin_is_the_static_twin(dims, conv, size):
    H, W = size
    want, _ = mcs.room_reference(dims, 3, H, W, conv)
    fr = mcs.frames_to(mcs.room_frames(3, H, W, conv), "cpu")
    for twist in (None, np.zeros((3, 6)), np.zeros(6)):
        g = mcs.room_grid(dims)
        r = sf.integrate_sweep_reference(g, twist=twist, **fr)
        same_grid(g, want)
        assert r.unseen == 0 and r.fused == int(want.weight.sum()) and r.evals[2:].sum() == 0
    # one zero row among three: the frames of the moving rows are masked out, so that the whole grid is the static frame's contribution
    twist = np.array(spc.PER_FRAME, np.float64)
    twist[1] = 0.0
    only = dict(fr, mask=fr["mask"] & torch.tensor([False, True, False])[:, None, None])
    g, s = mcs.room_grid(dims), mcs.room_grid(dims)
    r = sf.integrate_sweep_reference(g, twist=twist, **only)
    mesh.integrate_reference(s, **only)
    same_grid(g, s)
    assert int(s.weight.sum()) == r.fused and (r.fused > 0 or size == (5, 37))


# ---- 2. the rule header on the host ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sweepfuse_check") / "sweepfuse_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, SRC])
    return exe


def run_host(exe, tmp_path, before, fr, mo, intensity=True, hostile=False):
    """One call of the host program from the state `before` over the frames `fr` under the motion `mo`: (tsdf, weight, intensity or None, counts)."""
    F, H, W = fr["depth"].shape
    T = mesh.grid2sensor(before.origin, fr["sensor2world"])
    inc = np.asarray(fr["inclination"], np.float64)
    off, yaw = ri.convention(fr["data_type"], fr["sensor2ego"])
    xi, tau = sf._motion(mo["twist"], mo["tau"], F, W, mo["t_ref"], mo["direction"])
    N = int(np.prod(before.dims))
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as fh:
        fh.write(struct.pack("<12i", *before.dims, F, H, W, inc.size, int(intensity), int(xi is not None), int(hostile), 0, 0))
        fh.write(struct.pack("<8d", before.voxel, before.trunc, off, yaw, 0.0, 80.0, 0.0, 0.0))
        arrays = [T, inc] + ([xi, tau] if xi is not None else []) + [fr["depth"].numpy(), fr["mask"].numpy().astype(np.uint8)]
        arrays += [fr["intensity"].numpy()] if intensity else []
        arrays += [before.tsdf.numpy(), before.weight.numpy()] + ([before.intensity.numpy()] if intensity else [])
        for a in arrays:
            fh.write(np.ascontiguousarray(a).tobytes())
    res = subprocess.run([exe, inp, out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "SWEEPFUSECHECK ok" in res.stdout, res.stdout + res.stderr
    raw = np.fromfile(out, np.uint8)
    ts, wt = raw[:4 * N].view(np.float32), raw[4 * N:8 * N].view(np.int32)
    it = raw[8 * N:12 * N].view(np.float32) if intensity else None
    return ts, wt, it, raw[(12 if intensity else 8) * N:].view(np.int64), res


def against_twin(exe, tmp_path, before, fr, mo, want, report, intensity=True):
    ts, wt, it, counts, _ = run_host(exe, tmp_path, before, fr, mo, intensity)
    assert np.array_equal(ts.view(np.uint32), bits(want.tsdf)), int((ts.view(np.uint32) != bits(want.tsdf)).sum())
    assert np.array_equal(wt, bits(want.weight))
    if intensity:
        assert np.array_equal(it.view(np.uint32), bits(want.intensity))
    assert counts[0] == report.unseen and counts[1] == report.fused and np.array_equal(counts[2:], report.evals)


@pytest.mark.parametrize("mo_name", sfc.MOTIONS)
@pytest.mark.parametrize("conv", sfc.CONVENTIONS)
def test_the_rule_header_is_the_twin_bit_for_bit(host_check, tmp_path, conv, mo_name):
    for dims in sfc.GRIDS:
        for H, W in sfc.SIZES:
            want, reports = sfc.reference(dims, 3, H, W, conv, mo_name)
            against_twin(host_check, tmp_path, mcs.room_grid(dims), mcs.room_frames(3, H, W, conv), sfc.motion(mo_name, W), want, reports[0])
    assert np.all(sfc.all_evals()[1:] > 0)                                       # the long searches and the ones that do not converge are among them


@pytest.mark.parametrize("conv", sfc.CONVENTIONS)
def test_the_rule_header_on_a_second_call_without_intensity_and_without_a_twist(host_check, tmp_path, conv):
    dims, (H, W) = (17, 19, 23), (8, 64)
    before, _ = sfc.reference(dims, 3, H, W, conv, "strong_ccw")
    after, reports = sfc.reference(dims, 3, H, W, conv, "strong_ccw", True, 2)
    against_twin(host_check, tmp_path, before, mcs.room_frames(3, H, W, conv, 1), sfc.motion("strong_ccw", W), after, reports[1])
    assert int((after.weight > before.weight).sum()) > 0 and int(((after.weight == before.weight) & (before.weight > 0)).sum()) > 0
    want, reports = sfc.reference(dims, 3, H, W, conv, "table", False)
    against_twin(host_check, tmp_path, mcs.room_grid(dims, False), mcs.room_frames(3, H, W, conv), sfc.motion("table", W), want, reports[0], intensity=False)
    static, _ = mcs.room_reference(dims, 3, H, W, conv)
    ts, wt, it, counts, _ = run_host(host_check, tmp_path, mcs.room_grid(dims), mcs.room_frames(3, H, W, conv), dict(twist=None, tau=None, t_ref=0.5, direction="cw"))
    assert np.array_equal(ts.view(np.uint32), bits(static.tsdf)) and np.array_equal(wt, bits(static.weight)) and np.array_equal(it.view(np.uint32), bits(static.intensity))
    assert counts[0] == 0


def test_the_rule_header_under_the_sanitizers_survives_hostile_inputs(tmp_path):
    """A stand-alone program, never a Python process: columns forced far outside [0, W), NaN twists, infinite column times, a NaN and a
    non-monotonic inclination table run through the rule; the sanitizers report any read outside the table or the images."""
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = str(tmp_path / "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    linked = subprocess.run(["g++"] + flags + ["-o", str(tmp_path / "probe"), probe], capture_output=True, text=True)
    if linked.returncode != 0:
        pytest.skip("the sanitizer runtime does not link here: " + (linked.stderr.strip().splitlines() or ["g++ failed"])[-1])
    exe = str(tmp_path / "sweepfuse_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", exe, SRC])
    dims, (H, W), conv = (17, 19, 23), (8, 64), "waymo_table"
    want, reports = sfc.reference(dims, 3, H, W, conv, "strong_ccw")
    ts, wt, it, counts, res = run_host(exe, tmp_path, mcs.room_grid(dims), mcs.room_frames(3, H, W, conv), sfc.motion("strong_ccw", W), hostile=True)
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
    m = re.search(r"hostile: (\d+) searches", res.stdout)
    assert m and int(m.group(1)) >= 7 * 3 * 17 * 19 * 23 // 2, res.stdout    # the hostile passes did search
    assert np.array_equal(wt, bits(want.weight)) and counts[0] == reports[0].unseen


# ---- 3. accuracy: the moving scan fused under the sweep model is as good as a static scan ------------------------------------------------------------------

@pytest.mark.parametrize("conv", sfc.CONVENTIONS)
def test_the_moving_scan_is_fused_as_well_as_a_static_one(conv):
    """Measured (max, median) in metres -- kitti_bounds: e_s 0.0691 / 0.00906, e_u 0.5487 / 0.2469, e_c 0.0553 / 0.00801;
    waymo_table: e_s 0.0821 / 0.01117, e_u 0.5487 / 0.3877, e_c 0.0690 / 0.00993."""
    e = sfc.accuracy(conv)
    print(conv, e)
    assert e["e_c"][0] <= 1.5 * e["e_s"][0] and e["e_c"][1] <= 1.5 * e["e_s"][1], e
    assert e["e_u"][1] >= 5.0 * e["e_c"][1], e


# ---- 4. accumulation and the arguments -------------------------------------------------------------------------------------------------------------------

def test_a_second_call_accumulates_and_the_arguments_are_checked():
    dims, (H, W), conv = (17, 19, 23), (8, 64), "kitti_bounds"
    one, _ = sfc.reference(dims, 3, H, W, conv, "moderate_cw")
    two, reports = sfc.reference(dims, 3, H, W, conv, "moderate_cw", True, 2)
    g = mcs.room_grid(dims)
    for c in range(2):
        r = sf.integrate_sweep(g, **sfc.fuse_kw(mcs.room_frames(3, H, W, conv, c), sfc.motion("moderate_cw", W)))      # a CPU grid goes to the twin
        assert r.fused == reports[c].fused
    same_grid(g, two)
    assert int(two.weight.sum()) == reports[0].fused + reports[1].fused and int(one.weight.sum()) == reports[0].fused
    plain, rep = sfc.reference(dims, 3, H, W, conv, "moderate_cw", False)
    assert plain.intensity is None and np.array_equal(bits(plain.tsdf), bits(one.tsdf)) and rep[0].fused == reports[0].fused
    fr, mo = mcs.room_frames(3, H, W, conv), sfc.motion("moderate_cw", W)
    with pytest.raises(mesh.MeshError, match="go together"):
        sf.integrate_sweep(mcs.room_grid(dims, intensity=False), **sfc.fuse_kw(fr, mo))
    with pytest.raises(mesh.MeshError, match="go together"):
        sf.integrate_sweep(mcs.room_grid(dims), **sfc.fuse_kw(fr, mo, intensity=False))
    for bad, msg in ((dict(twist=np.zeros((2, 6))), "twist must be"), (dict(twist=np.full(6, np.nan)), "non-finite twist"), (dict(tau=np.zeros(W + 1)), "column times"),
                     (dict(direction="up"), "integrate_sweep"), (dict(workspace=torch.zeros(1 << 16, dtype=torch.uint8)), "workspace")):
        with pytest.raises(mesh.MeshError, match=msg):
            sf.integrate_sweep(mcs.room_grid(dims), **dict(sfc.fuse_kw(fr, mo), **bad))
    pts = sf.sweep_points(fr["depth"], fr["sensor2world"], None, fr["inclination"])
    meta_d = mcs.rc.local_directions(H, W, fr["inclination"], "KITTI", None).numpy().astype(np.float64)
    want = (meta_d[None] * fr["depth"].numpy()[..., None].astype(np.float64)) @ np.swapaxes(fr["sensor2world"][:, :3, :3], 1, 2)[:, None] + fr["sensor2world"][:, None, None, :3, 3]
    assert pts.shape == (3, H, W, 3) and np.abs(pts - want).max() < 1e-5        # without a twist: the static grid's points (float32 directions there)


# ---- 5. the command lines ---------------------------------------------------------------------------------------------------------------------------------

def run_mesh(root, out_dir, device, extra=()):
    out = os.path.join(out_dir, "mesh.ply")
    mesh.main(["--data", root, "--out", out, "--voxel", "0.3", "--device", device] + list(extra))
    return out


@pytest.mark.parametrize("tau", (False, True))
def test_mesh_sweep_stored_on_the_cpu_writes_the_twins_mesh_nearer_the_planes(tmp_path, tau):
    """Measured medians of the vertices' distance to the nearest plane, --voxel 0.3: stored 0.01745 m against off 0.05000 m (with the frames' own
    column times: 0.01737 against 0.05000)."""
    root = sfc.write_sweep_sequence(str(tmp_path / "seq"), tau=tau)
    out = run_mesh(root, str(tmp_path / "stored"), "cpu", ["--sweep", "stored", "--batch", "2"] if tau else ["--sweep", "stored"])
    ply = mesh.read_ply(out)
    rep = json.load(open(str(tmp_path / "stored" / "mesh.json")))
    assert rep["sweep"]["mode"] == "stored" and rep["sweep"]["fused"] > 0 and rep["sweep"]["unseen"] >= 0 and rep["args"]["sweep"] == "stored"
    if not tau:                                                                # one call: the twin in one call (with per-frame column times a call per tau)
        want, r, _ = sfc.check_sequence_margins(root, str(tmp_path / "stored"))
        assert want.faces.shape[0] > 1000
        assert np.array_equal(ply.points, want.world()) and np.array_equal(ply.faces, want.faces.numpy())
        assert np.array_equal(ply.intensity.view(np.uint32), want.intensity.numpy().view(np.uint32))
        assert (rep["sweep"]["unseen"], rep["sweep"]["fused"]) == (r.unseen, r.fused)
    off = mesh.read_ply(run_mesh(root, str(tmp_path / "off"), "cpu"))
    rep_off = json.load(open(str(tmp_path / "off" / "mesh.json")))
    assert rep_off["sweep"] == {"mode": "off"}
    e_c, e_u = np.median(sfc.plane_distance(ply.points)), np.median(sfc.plane_distance(off.points))
    print("median distance to the planes: stored", e_c, "off", e_u)
    assert e_c < e_u


def test_a_sequence_without_stored_twists_is_refused_with_the_frames_file(tmp_path):
    root = sfc.write_sweep_sequence(str(tmp_path / "seq"), stored=False)
    with pytest.raises(SystemExit, match=r"frames.000000\.npz: no stored twist"):
        run_mesh(root, str(tmp_path / "m"), "cpu", ["--sweep", "stored"])
    with pytest.raises(SystemExit, match=r"frames.000000\.npz: no stored twist"):
        raycast.main(["--data", root, "--out", str(tmp_path / "r.json"), "--voxel", "0.3", "--device", "cpu", "--fuse-sweep", "stored"])
    assert os.path.getsize(run_mesh(root, str(tmp_path / "off"), "cpu")) > 1000         # --sweep off does not need them


def test_raycast_from_the_sweep_fused_grid_has_the_lower_depth_error(tmp_path):
    """Measured mean depth rmse over the three frames, --voxel 0.3 (misses count with their full range): --fuse-sweep stored 1.5825 m against off
    1.8017 m; the median absolute error is 0.0167 m against 0.0970 m."""
    root = sfc.write_sweep_sequence(str(tmp_path / "seq"))
    rmse = {}
    for mode in ("stored", "off"):
        rep = raycast.main(["--data", root, "--out", str(tmp_path / f"{mode}.json"), "--voxel", "0.3", "--device", "cpu", "--fuse", "all", "--frames", "all",
                            "--sweep", "stored", "--fuse-sweep", mode])
        assert rep["fuse_sweep"]["mode"] == mode and (("fused" in rep["fuse_sweep"]) == (mode == "stored"))
        rmse[mode] = rep["mean"]["depth"]["rmse"]
    print("depth rmse:", rmse)
    assert rmse["stored"] < rmse["off"]


# ---- 6. the library: its build entry, exports and resource gate, refused arguments -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def sweepfuse_lib():
    from lidar_rt_amd import build as lrt_build
    return lrt_build.build_sweepfuse()


def test_the_library_builds_and_exports_what_its_header_declares(sweepfuse_lib):
    from lidar_rt_amd import build as lrt_build
    REPO = os.path.dirname(HERE)
    assert os.path.exists(sweepfuse_lib) and not lrt_build.sweepfuse_is_stale()
    assert lrt_build.SWEEPFUSE_SOURCES == ["lrt_sweepfuse.hip"]
    assert {"lrt_sweepfuse_math.h", "lrt_mesh_math.h", "lrt_sweepproj_math.h", "lrt_project_math.h", "lrt_sweep_math.h"} <= set(lrt_build.SWEEPFUSE_HEADERS)
    assert "lrt_sweepfuse" not in " ".join(lrt_build.MESH_SOURCES + lrt_build.MESH_HEADERS + lrt_build.SWEEPPROJ_SOURCES + lrt_build.SWEEPPROJ_HEADERS)
    src = open(lrt_build.__file__).read()
    assert "build_sweepfuse(force, verbose)" in src[src.index("def _build_product"):src.index("def _build_lib")]
    assert "csrc/liblrt_sweepfuse.so" in open(os.path.join(REPO, "setup.py")).read()
    hdr = open(os.path.join(REPO, "include", "lrt_sweepfuse.h")).read()
    declared = set(re.findall(r"\b(lrt_sweepfuse_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(sf.EXPORTS), declared ^ set(sf.EXPORTS)
    exported = set(re.findall(r"\blrt_sweepfuse_[a-z_]+\b", subprocess.run(["nm", "-D", "--defined-only", sweepfuse_lib], capture_output=True, text=True, check=True).stdout))
    assert exported == declared, exported ^ declared
    lib = sf.load()
    assert lib.lrt_sweepfuse_abi_version() == int(re.search(r"#define\s+LRT_SWEEPFUSE_ABI_VERSION\s+(\d+)", hdr).group(1)) == sf.ABI_VERSION
    for name, val in (("BLOCK", sf.BLOCK), ("MAX_EVAL", sf.MAX_EVAL), ("TABLE", sf.TABLE), ("MAX_FRAMES", sf.MAX_FRAMES)):
        assert int(re.search(rf"#define\s+LRT_SWEEPFUSE_{name}\s+(\d+)", hdr).group(1)) == val, name
    assert sf.BLOCK == mesh.BLOCK and sf.MAX_FRAMES == mesh.MAX_FRAMES
    from lidar_rt_amd import sweep_project
    assert sf.MAX_EVAL == sweep_project.MAX_EVAL and sf.TABLE == sweep_project.TABLE
    assert lib.lrt_sweepfuse_work_bytes(-1, 8) < 0 and lib.lrt_sweepfuse_work_bytes(3, 0) < 0 and lib.lrt_sweepfuse_work_bytes(65537, 8) < 0
    assert lib.lrt_sweepfuse_work_bytes(0, 8) == 0 and lib.lrt_sweepfuse_work_bytes(1, 1) == 256 and lib.lrt_sweepfuse_work_bytes(3, 37) == 10752
    assert sf.work_bytes(16, 2048) == 16 * 2048 * 96


def test_the_kernels_pass_the_resource_gate(sweepfuse_lib):
    from lidar_rt_amd import resources
    res = resources.kernel_resources(sweepfuse_lib)
    own = sorted(n for n in res if resources.is_own_kernel(n))
    assert own == ["k_sf_fuse", "k_sf_table"], own
    assert all(any(re.search(g_, n) for g_ in resources.GATED) for n in own)
    assert resources.violations(res) == []
    assert all(res[n]["vgpr_spill"] == 0 and res[n]["scratch_bytes"] == 0 for n in own)


INTEGRATE_ARGS = ("device", "X", "Y", "Z", "voxel", "trunc", "tsdf", "weight", "intensity", "F", "T", "H", "W", "depth", "mask", "fint", "inclination",
                  "n_inc", "off", "yaw", "min_depth", "max_depth", "twist", "tau", "workspace", "work_bytes", "stream")


def test_argument_errors_come_before_the_device_and_launch_nothing(sweepfuse_lib):
    """Non-null dummy pointers and device 99: a refused argument is reported first; valid arguments reach the device check, which refuses too."""
    lib = sf.load()
    ok = dict(device=99, X=3, Y=3, Z=3, voxel=0.1, trunc=0.3, tsdf=8, weight=8, intensity=None, F=1, T=8, H=4, W=8, depth=8, mask=8, fint=None,
              inclination=8, n_inc=2, off=0.0, yaw=0.0, min_depth=0.0, max_depth=80.0, twist=8, tau=8, workspace=256, work_bytes=768, stream=None)
    call = lambda **kw: lib.lrt_sweepfuse_integrate(*[dict(ok, **kw)[k] for k in INTEGRATE_ARGS])
    for kw, msg in (({"X": 0}, "a grid of 0 x"), ({"X": 65536, "Y": 65536}, "a grid of 65536 x"), ({"voxel": 0.0}, "voxel 0"), ({"F": -1}, "-1 frames"),
                    ({"F": sf.MAX_FRAMES + 1}, "65537 frames"), ({"n_inc": 3}, "3 inclinations"), ({"n_inc": 4, "H": 2}, "4 inclinations"),
                    ({"tsdf": None}, "null tsdf"), ({"intensity": 8}, "go together"), ({"min_depth": 5.0, "max_depth": 1.0}, "depths"), ({"off": 1.0}, "off 1"),
                    ({"tau": None}, "null tau"), ({"workspace": None}, "256-byte aligned"), ({"workspace": 264}, "256-byte aligned"),
                    ({"work_bytes": 767}, "a workspace of 767 bytes"), ({"twist": None, "tau": None, "work_bytes": 0}, "a workspace of 0 bytes"),
                    ({}, "no HIP device 99"), ({"twist": None, "tau": None}, "no HIP device 99")):
        assert call(**kw) == -1, kw
        assert msg in lib.lrt_sweepfuse_last_error().decode(), (kw, lib.lrt_sweepfuse_last_error())
    assert call(F=0) == 0 and call(F=0, workspace=None, work_bytes=0) == 0            # nothing to fuse: no launch, not even a device
