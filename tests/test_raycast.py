"""The ray casting on the CPU (lidar_rt_amd/raycast.py): the library's build entry, exports and resource gate; the rule header against the numpy twin
on the host, bit for bit; a hand case written out sample by sample; planes and a sphere against their closed forms within bounds derived from the
rule; the room grids; refused arguments; and the command line with --device cpu."""
import json
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

from lidar_rt_amd import evaluation, mesh, raycast, sequence
from tests import mesh_cases as mcs
from tests import raycast_cases as rcs
from tests.test_mesh import write_room_sequence

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def twin(grid, o, d, **kw):
    return raycast.raycast_reference(grid, torch.as_tensor(o), torch.as_tensor(d), samples=True, **kw)


# ---- 1. the library: its build entry, exports and resource gate ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def raycast_lib():
    from lidar_rt_amd import build as lrt_build
    return lrt_build.build_raycast()


def test_the_library_builds_and_exports_what_its_header_declares(raycast_lib):
    from lidar_rt_amd import build as lrt_build
    assert os.path.exists(raycast_lib) and not lrt_build.raycast_is_stale()
    assert lrt_build.RAYCAST_SOURCES == ["lrt_raycast.hip"] and "lrt_raycast_math.h" in lrt_build.RAYCAST_HEADERS
    src = open(lrt_build.__file__).read()
    assert "build_raycast(force, verbose)" in src[src.index("def _build_product"):src.index("def _build_lib")]
    assert "csrc/liblrt_raycast.so" in open(os.path.join(REPO, "setup.py")).read()
    hdr = open(os.path.join(REPO, "include", "lrt_raycast.h")).read()
    declared = set(re.findall(r"\b(lrt_raycast(?:_[a-z_]+)?)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(raycast.EXPORTS), declared ^ set(raycast.EXPORTS)
    nm = subprocess.run(["nm", "-D", "--defined-only", raycast_lib], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\blrt_raycast(?:_[a-z_]+)?\b", nm))
    assert exported == declared, exported ^ declared
    lib = raycast.load()
    assert lib.lrt_raycast_abi_version() == int(re.search(r"#define\s+LRT_RAYCAST_ABI_VERSION\s+(\d+)", hdr).group(1)) == raycast.ABI_VERSION
    for name, val in (("BLOCK", raycast.BLOCK), ("MAX_SAMPLES", raycast.MAX_SAMPLES)):
        assert int(re.search(rf"#define\s+LRT_RAYCAST_{name}\s+(\d+)", hdr).group(1)) == val, name
    for name, val in (("MAX_RAYS", raycast.MAX_RAYS), ("MAX_VOXELS", mesh.MAX_VOXELS)):
        assert int(re.search(rf"#define\s+LRT_RAYCAST_{name}\s+(\d+)LL", hdr).group(1)) == val, name


def test_the_kernel_passes_the_resource_gate(raycast_lib):
    from lidar_rt_amd import resources
    res = resources.kernel_resources(raycast_lib)
    own = sorted(n for n in res if resources.is_own_kernel(n))
    assert own == ["k_raycast"], own
    assert all(any(re.search(g_, n) for g_ in resources.GATED) for n in own)
    assert resources.violations(res) == []


# ---- 2. the rule header on the host -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("raycast_check") / "raycast_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "host_check", "raycast_check.cpp")])
    return exe


def host_cases():
    """{name: (grid, rays_o (N, 3), rays_d (N, 3), kw)} -- rays sampled from each case, with the bad rays added."""
    bo, bd = rcs.bad_rays()
    cat = lambda o, d: (np.concatenate([np.asarray(o, np.float32).reshape(-1, 3), bo]), np.concatenate([np.asarray(d, np.float32).reshape(-1, 3), bd]))
    rng = np.random.default_rng(11)
    out = {}
    hg = rcs.hand_grid()
    out["hand"] = (hg, *cat([[1, 1, 0], [1, 1, 8], [0.7, 1.2, -1]], [[0, 0, 1], [0, 0, -1], [0.01, -0.02, 1]]), dict(min_weight=2))
    po, pd, _ = rcs.planar_rays()
    mo, md = rcs.planar_missing_rays()
    out["planar"] = (rcs.planar_grid(), *cat(np.concatenate([po[:100], mo]), np.concatenate([pd[:100], md])), {})
    g, oo, od, _, _ = rcs.oblique_case(0)
    out["oblique"] = (g, *cat(oo, od), {})
    so, sd, _ = rcs.sphere_rays()
    out["sphere"] = (mcs.sdf_grid("sphere"), *cat(so[:100], sd[:100]), {})
    for dims in mcs.GRIDS:
        o, d = rcs.room_rays(2, 8, 64, "waymo_table")
        pick = rng.choice(o.reshape(-1, 3).shape[0], 300, replace=False)
        out[f"room{dims}"] = (rcs.room_grid(dims, "waymo_table")[0], *cat(o.reshape(-1, 3).numpy()[pick], d.reshape(-1, 3).numpy()[pick]),
                              dict(min_weight=2, step=0.3, far_step=0.6, min_depth=1.0, max_depth=30.0))
    return out


HOST_CASES = ["hand", "planar", "oblique", "sphere"] + [f"room{d}" for d in mcs.GRIDS]


@pytest.mark.parametrize("name", HOST_CASES)
def test_the_rule_header_is_the_twin_bit_for_bit(host_check, tmp_path, name):
    grid, o, d, kw = host_cases()[name]
    mw, step, far, lo, hi = raycast.params(grid, **kw)
    want = twin(grid, o, d, **kw)
    N = o.shape[0]
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    has_int = grid.intensity is not None
    with open(inp, "wb") as fh:
        fh.write(struct.pack("<8i", *grid.dims, mw, N, int(has_int), 0, 0))
        fh.write(struct.pack("<8d", grid.voxel, *[float(x) for x in grid.origin], step, far, lo, hi))
        fh.write(grid.tsdf.numpy().tobytes()); fh.write(grid.weight.numpy().tobytes())
        if has_int:
            fh.write(grid.intensity.numpy().tobytes())
        fh.write(np.ascontiguousarray(o, np.float32).tobytes()); fh.write(np.ascontiguousarray(d, np.float32).tobytes())
    res = subprocess.run([host_check, inp, out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "RAYCHECK ok" in res.stdout, res.stdout + res.stderr
    raw = np.fromfile(out, np.uint8)
    depth, hit = raw[:4 * N].view(np.float32), raw[4 * N:5 * N].astype(bool)
    inten, ns = raw[5 * N:9 * N].view(np.float32), raw[9 * N:13 * N].view(np.int32)
    assert np.array_equal(depth.view(np.uint32), want.depth.numpy().view(np.uint32))
    assert np.array_equal(hit, want.hit.numpy())
    if has_int:
        assert np.array_equal(inten.view(np.uint32), want.intensity.numpy().view(np.uint32))
    assert np.array_equal(ns, want.samples.numpy())
    assert np.all(ns[-6:] == 0) and not hit[-6:].any()                              # the bad rays
    if name in ("hand", "planar", "oblique", "sphere"):
        assert hit.sum() > 0


# ---- 3. the hand case -------------------------------------------------------------------------------------------------------------------------------------

def test_the_hand_case():
    """(2, 2, 8) grid, voxel 1, trunc 4, origin 0: centres z = 0.5 ... 7.5, tsdf (4.25 - z) / 4 = 0.9375, 0.6875, 0.4375, 0.1875, -0.0625, ...;
    intensity z / 8.  The ray from (1, 1, 0) along +z: x and y are constant (u_x = u_y = 0, inside [0.5, 1.5]), t_in = 0.5, t_out = 7.5; the
    default step is 0.5 and no cell is all 1.0, so t_k = 0.5 + 0.5 k.  With layer 1 at weight 1 and min_weight 2, the cells 0 and 1 are unknown:

        k  t    cell f    known  D
        1  0.5  0    0    no
        2  1.0  0    0.5  no
        3  1.5  1    0    no
        4  2.0  1    0.5  no
        5  2.5  2    0    yes    0.4375
        6  3.0  2    0.5  yes    0.3125
        7  3.5  3    0    yes    0.1875
        8  4.0  3    0.5  yes    0.0625
        9  4.5  4    0    yes   -0.0625   crossing: w = 0.0625 / 0.125 = 0.5, t* = 4.0 + 0.5 0.5 = 4.25

    intensity: 0.5 (t = 4.0) and 0.5625 (t = 4.5), 0.5 + 0.0625 0.5 = 0.53125.  With layer 4 unobserved the crossing lies in unknown cells (3 and 4):
    no hit, all 15 samples.  The ray from (1, 1, 8) along -z sees the tsdf rise through 0: not a crossing, 15 samples."""
    o = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 8.0]], np.float32)
    d = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]], np.float32)
    r = twin(rcs.hand_grid(1), o, d, min_weight=2)
    assert r.hit.tolist() == [True, False] and r.samples.tolist() == [9, 15]
    assert r.depth.tolist() == [4.25, 0.0] and r.intensity.tolist() == [0.53125, 0.0]
    r = twin(rcs.hand_grid(1), o, d, min_weight=1)                                     # all known: the same crossing
    assert r.hit.tolist() == [True, False] and r.samples.tolist() == [9, 15] and r.depth.tolist() == [4.25, 0.0]
    r = twin(rcs.hand_grid(4), o, d, min_weight=2)
    assert r.hit.tolist() == [False, False] and r.samples.tolist() == [15, 15] and r.depth.tolist() == [0.0, 0.0]


# ---- 4. planes ------------------------------------------------------------------------------------------------------------------------------------------------

def test_an_axis_aligned_plane_is_hit_at_its_closed_form_range():
    """Every tsdf is exact in float32 and no crossing cell is clipped (a sample within a step, 0.125, of the plane has corners within 0.375 <
    trunc = 0.5 of it), so the trilinear values and the crossing are the linear function's up to float64 rounding: within 1 float32 ulp of the
    closed form.  The rays start inside the grid and outside it (the slab entry)."""
    g = rcs.planar_grid()
    o, d, t_exact = rcs.planar_rays()
    o64, u64 = rcs.rule_ray(o, d, rcs.PLANE_ORIGIN)
    inside = np.all((o64 >= 0.125) & (o64 <= np.array(rcs.PLANE_DIMS) * 0.25 - 0.125), 1)
    assert o.shape[0] >= 300 and inside.sum() >= 50 and (~inside).sum() >= 50
    r = twin(g, o, d)
    assert bool(r.hit.all())
    err = np.abs(r.depth.numpy().astype(np.float64) - t_exact)
    ulp = np.spacing(t_exact.astype(np.float32)).astype(np.float64)
    print("planar: largest error / ulp", float((err / ulp).max()))
    assert np.all(err <= ulp)
    assert np.all(r.intensity.numpy() > 0)
    mo, md = rcs.planar_missing_rays()
    r = twin(g, mo, md)
    assert not bool(r.hit.any()) and np.all(r.depth.numpy() == 0) and np.all(r.samples.numpy() > 0)


@pytest.mark.parametrize("seed", range(6))
def test_an_oblique_clipped_plane_is_hit_within_its_bound(seed):
    """trunc = 3 voxels, default steps (0.125, 0.625).  A far step follows only a known sample whose corners all hold 1.0f: it lies at least trunc
    in front of the plane, and a step shorter than trunc cannot reach it.  So the crossing is between two samples a step apart, within 0.125 |n.u| of
    the plane, whose cells' corners lie within 0.125 + sqrt(3) 0.25 < 0.75 of it: unclipped, where the trilinear value of the linear distance is
    exact.  What remains is the float32 rounding of the stored tsdf (2^-24 per value, 2^-24 trunc in distance, / |n.u| along the ray; doubled for
    the two samples) and of the depth: |depth - t_exact| <= ulp32(t_exact) + 2^-23 trunc / |n.u|."""
    g, o, d, t_exact, nu = rcs.oblique_case(seed)
    assert o.shape[0] >= 40
    r = twin(g, o, d)
    assert bool(r.hit.all())
    err = np.abs(r.depth.numpy().astype(np.float64) - t_exact)
    bound = np.spacing(t_exact.astype(np.float32)).astype(np.float64) + rcs.U23 * g.trunc / nu
    print(f"oblique {seed}: largest error / bound", float((err / bound).max()))
    assert np.all(err <= bound)


# ---- 5. the sphere ----------------------------------------------------------------------------------------------------------------------------------------

def test_the_sphere_is_hit_within_the_interpolation_bound():
    """mesh_cases.sdf_grid("sphere"): f = |x - c| - R clipped at trunc = 3 h, R = 1.2, h = 0.25; rays aimed at the centre from distances in
    [R + trunc + step, 4].  Along such a ray the true f is linear (the radial distance), so the crossing's error is the trilinear interpolation
    error of the samples around it.  That error, for a convex function, is at most h^2 / 8 sum_i max f_ii over the cell; f_ii <= 1 / r, and the
    cells the two samples use lie at r >= R - step - sqrt(3) h, so |D - f| <= 3 h^2 / (8 (R - step - sqrt(3) h)) in distance units at each sample,
    which interpolation between them carries to the range along a radial ray.  The float32 tsdf adds 2^-23 trunc:
    delta = 3 h^2 / (8 (R - step - sqrt(3) h)) + 2^-23 trunc, about 0.0365 m."""
    g = mcs.sdf_grid("sphere")
    assert g.trunc == 3 * rcs.SPHERE_H and g.voxel == rcs.SPHERE_H
    o, d, t_exact = rcs.sphere_rays()
    o64, _ = rcs.rule_ray(o, d, (0.0, 0.0, 0.0))
    inside = np.all((o64 >= 0.125) & (o64 <= np.array(g.dims) * 0.25 - 0.125), 1)
    assert inside.sum() >= 50 and (~inside).sum() >= 50
    r = twin(g, o, d)
    delta = rcs.sphere_delta()
    assert abs(delta - 0.0365) < 5e-4
    assert bool(r.hit.all())
    err = np.abs(r.depth.numpy().astype(np.float64) - t_exact)
    print("sphere: largest error", float(err.max()), "delta", delta)
    assert float(err.max()) <= delta


# ---- 6. the room grids ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", list(mcs.GRIDS))
def test_the_room_grids(dims):
    g, margin = rcs.room_grid(dims, "kitti_bounds")
    assert margin >= mcs.MARGIN
    o, d = rcs.room_rays(3, 8, 64, "kitti_bounds")
    r = twin(g, o, d)
    assert r.depth.shape == (3, 8, 64) and r.hit.dtype == torch.bool and r.samples.dtype == torch.int32
    if dims == (1, 9, 40):                                                            # an axis of one voxel: no domain
        assert not bool(r.hit.any()) and int(r.samples.max()) == 0
    else:
        assert bool(r.hit.any()) and int(r.samples.max()) > 0
        assert np.all(r.depth.numpy()[~r.hit.numpy()] == 0) and np.all(r.depth.numpy()[r.hit.numpy()] > 0)
    bo, bd = rcs.bad_rays()
    b = twin(g, bo, bd)
    assert not bool(b.hit.any()) and b.samples.tolist() == [0] * 6 and b.depth.tolist() == [0.0] * 6


def test_the_cpu_entry_is_the_twin_and_shapes_follow_the_rays():
    g = rcs.planar_grid(intensity=False)
    o, d, _ = rcs.planar_rays()
    a = raycast.raycast(g, torch.from_numpy(o[:12]).reshape(3, 4, 3), torch.from_numpy(d[:12]).reshape(3, 4, 3))
    assert a.depth.shape == (3, 4) and a.intensity is None and a.samples is None
    b = twin(g, o[:12], d[:12])
    assert torch.equal(a.depth.reshape(-1), b.depth) and torch.equal(a.hit.reshape(-1), b.hit)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------------------

RAYCAST_ARGS = ("device", "X", "Y", "Z", "voxel", "trunc", "ox", "oy", "oz", "tsdf", "weight", "intensity", "min_weight", "N", "ray_o", "ray_d", "step",
                "far_step", "min_depth", "max_depth", "depth", "hit", "out_intensity", "samples", "stream")


def test_bad_arguments_are_refused_and_named(raycast_lib):
    """The library: a negative code and a message naming the argument, before the device is touched (device 99, dummy pointers); N == 0 returns 0.
    Python: a RaycastError naming it."""
    lib = raycast.load()
    ok = dict(device=99, X=3, Y=3, Z=3, voxel=0.1, trunc=0.3, ox=0.0, oy=0.0, oz=0.0, tsdf=8, weight=8, intensity=None, min_weight=1, N=5, ray_o=8,
              ray_d=8, step=0.05, far_step=0.25, min_depth=0.0, max_depth=80.0, depth=8, hit=8, out_intensity=None, samples=None, stream=None)
    call = lambda **kw: lib.lrt_raycast(*[dict(ok, **kw)[k] for k in RAYCAST_ARGS])
    for kw, msg in (({"X": 0}, "a grid of 0 x"), ({"voxel": 0.0}, "voxel 0"), ({"trunc": -1.0}, "trunc -1"), ({"ox": float("nan")}, "origin"),
                    ({"min_weight": 0}, "min_weight 0"), ({"N": -1}, "-1 rays"), ({"step": 0.0}, "step 0"), ({"far_step": 0.3}, "far_step"),
                    ({"far_step": 0.04}, "far_step"), ({"min_depth": -1.0}, "depths"), ({"min_depth": 80.0}, "depths"),
                    ({"max_depth": float("inf")}, "depths"), ({"step": 1e-20, "far_step": 0.1}, "does not advance"),
                    ({"step": 1e-9, "far_step": 0.1}, "diagonal"), ({"tsdf": None}, "null tsdf"), ({"intensity": 8}, "go together"),
                    ({"out_intensity": 8}, "go together"), ({"ray_o": None}, "null ray_o"), ({}, "no HIP device 99")):
        assert call(**kw) < 0, kw
        assert msg in lib.lrt_raycast_last_error().decode(), (kw, lib.lrt_raycast_last_error())
    assert call(N=0) == 0                                                              # nothing to cast: no launch, not even a device
    g = rcs.planar_grid()
    o, d, _ = rcs.planar_rays()
    o, d = torch.from_numpy(o[:4]), torch.from_numpy(d[:4])
    for kw, msg in (({"min_weight": 0}, "min_weight 0"), ({"step": 0.0}, "step 0"), ({"step": -0.1}, "step -0.1"), ({"far_step": 0.5}, "far_step"),
                    ({"step": 0.2, "far_step": 0.1}, "far_step"), ({"min_depth": -1.0}, "depths"), ({"max_depth": 0.0}, "depths"),
                    ({"max_depth": float("inf")}, "depths"), ({"step": 1e-20, "far_step": 0.1}, "does not advance"),
                    ({"step": 1e-9, "far_step": 0.1}, "diagonal")):
        with pytest.raises(raycast.RaycastError, match=msg):
            raycast.raycast(g, o, d, **kw)
    with pytest.raises(raycast.RaycastError, match="rays_o"):
        raycast.raycast(g, o.double(), d)
    with pytest.raises(raycast.RaycastError, match="rays_d"):
        raycast.raycast(g, o, d[:, :2])
    with pytest.raises(raycast.RaycastError, match="differ in shape"):
        raycast.raycast(g, o, d[:2])
    with pytest.raises(raycast.RaycastError, match="TsdfGrid"):
        raycast.raycast(object(), o, d)


# ---- 8. the command line on the CPU -----------------------------------------------------------------------------------------------------------------------

def evaluate_keys():
    t = torch.rand(8, 8)
    return {"depth": sorted(evaluation.depth_metrics(t, t)), "intensity": sorted(evaluation.intensity_metrics(t, t)),
            "raydrop": sorted(evaluation.raydrop_metrics(t > 0.5, t > 0.5)), "points": ["chamfer_dist", "fscore"]}


def run_cli(root, out_dir, device, extra=()):
    out = os.path.join(out_dir, "raycast.json")
    raycast.main(["--data", root, "--voxel", "0.3", "--device", device, "--out", out, "--sequence", os.path.join(out_dir, "seq")] + list(extra))
    return out


def test_the_command_line_on_the_cpu(tmp_path):
    root = write_room_sequence(str(tmp_path / "data"))
    out = run_cli(root, str(tmp_path / "cpu"), "cpu")
    rep = json.load(open(out))
    keys = evaluate_keys()
    assert {g: sorted(v) for g, v in rep["mean"].items()} == keys
    assert sorted(rep["per_frame"]) == ["0", "1", "2"]
    for f in rep["per_frame"].values():
        assert {g: sorted(v) for g, v in f.items()} == keys
    assert rep["fused_frames"] == [0, 1, 2] and rep["frames"] == [0, 1, 2]
    assert rep["grid"]["voxel"] == 0.3 and rep["grid"]["trunc"] == pytest.approx(0.9)
    assert 0.5 < rep["cast"]["hit_fraction"] <= 1.0 and rep["cast"]["samples_per_ray"]["max"] > 0
    assert all(math.isfinite(v) for g in rep["mean"].values() for v in g.values())
    seq = sequence.load_sequence(str(tmp_path / "cpu" / "seq"), "cpu")
    src = sequence.load_sequence(root, "cpu")
    for f in (0, 1, 2):
        m, dep = seq.frames.get_mask(f), seq.frames.get_depth(f)
        assert torch.equal(dep > 0, m)
        gt, gm = src.frames.get_depth(f), src.frames.get_mask(f)
        both = m & gm
        assert int(both.sum()) > 1000
        err = (dep[both] - gt[both]).abs()
        print(f"frame {f}: median |depth - gt| {float(err.median()):.4f}")
        assert float(err.median()) < 0.3                                                # the map's range is within a voxel of the scan's
        assert torch.equal(seq.frames.get_range_rays(f)[0], src.frames.get_range_rays(f)[0])
