"""The surface meshes on the CPU (lidar_rt_amd/mesh.py): the generated triangle table, closed surfaces over every configuration, negative controls
that the closed-surface check and the sphere bound catch, the analytic sphere in closed form, the rule header against the twin on the host, and the
command line with --device cpu."""
import json
import math
import os
import re
import struct
import subprocess
from collections import Counter

import numpy as np
import pytest
import torch

from lidar_rt_amd import mesh, range_image as ri, sequence
from tests import mesh_cases as mcs
from tests import registration_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
U24 = 2.0 ** -24


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------------------------

def closed_surface_errors(m):
    """The violations of a closed, oriented, 2-manifold triangle mesh: every undirected edge in exactly two faces, once in each direction; no
    repeated vertex id within a face; no unreferenced vertex."""
    f = m.faces.numpy().astype(np.int64).reshape(-1, 3)
    V = m.vertices.shape[0]
    errs = []
    rep = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])
    if rep.any():
        errs.append(f"{int(rep.sum())} faces repeat a vertex")
    used = np.zeros(V, bool)
    used[f.reshape(-1)] = True
    if not used.all():
        errs.append(f"{int((~used).sum())} unreferenced vertices")
    directed = Counter(map(tuple, np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).tolist()))
    bad = [e for e, c in directed.items() if c != 1 or directed.get((e[1], e[0]), 0) != 1]
    if bad:
        errs.append(f"{len(bad)} directed edges not matched by exactly one reverse (e.g. {bad[:3]})")
    return errs


def euler(m):
    f = m.faces.numpy().astype(np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    return m.vertices.shape[0] - len(np.unique(e, axis=0)) + f.shape[0]


def crossed_edges(cfg):
    return {e for e in range(12) if (cfg >> mesh.edge_corners(e)[0] & 1) != (cfg >> mesh.edge_corners(e)[1] & 1)}


# ---- 1. the table -------------------------------------------------------------------------------------------------------------------------------------------

def test_the_committed_header_is_the_generated_table():
    with open(mesh.TABLE_PATH) as f:
        assert f.read() == mesh.table_header()
    table = mesh.mc_table()
    assert len(table) == 256 and table[0] == [] and table[255] == []
    for cfg, tris in enumerate(table):
        used = {e for t in tris for e in t}
        assert used == crossed_edges(cfg), cfg                        # only crossed edges, and every one of them


def test_the_tables_orientation_points_from_negative_to_positive():
    """One negative corner: the triangle's normal points away from it, along (1, 1, 1) for corner 0, at every corner by symmetry."""
    mid = lambda e: 0.5 * (mesh.corner_pos(mesh.edge_corners(e)[0]) + mesh.corner_pos(mesh.edge_corners(e)[1]))
    for n in range(8):
        for cfg, sign in ((1 << n, 1.0), (255 ^ (1 << n), -1.0)):
            (a, b, c), = mesh.mc_table()[cfg]
            nrm = np.cross(mid(b) - mid(a), mid(c) - mid(a))
            centre = (mid(a) + mid(b) + mid(c)) / 3
            assert sign * float(nrm @ (centre - mesh.corner_pos(n))) > 0, (n, cfg)


# ---- 2. closed surfaces ------------------------------------------------------------------------------------------------------------------------------------

def test_random_sign_grids_cover_every_configuration_and_give_closed_surfaces():
    seen = set()
    for seed in mcs.SEEDS:
        g = mcs.random_grid(seed)
        seen |= mcs.configurations(g)
        m = mesh.extract_reference(g)
        assert m.faces.shape[0] > 0
        assert closed_surface_errors(m) == [], seed
    assert seen == set(range(256))


@pytest.mark.parametrize("kind, chi", [("sphere", 2), ("torus", 0)])
def test_sampled_sphere_and_torus_have_their_euler_characteristic(kind, chi):
    m = mesh.extract_reference(mcs.sdf_grid(kind))
    assert closed_surface_errors(m) == []
    assert euler(m) == chi


# ---- 3. negative controls ----------------------------------------------------------------------------------------------------------------------------------

def _fails_somewhere(table):
    return any(closed_surface_errors(mesh.extract_reference(mcs.random_grid(s), table=table)) for s in mcs.SEEDS)


@pytest.mark.parametrize("cfg", [1, 90, 165, 254])
def test_the_closed_surface_check_catches_a_reversed_configuration(cfg):
    table = mesh.mc_table()
    table[cfg] = [(a, c, b) for a, b, c in table[cfg]]
    assert _fails_somewhere(table)


@pytest.mark.parametrize("cfg", [1, 90, 165, 254])
def test_the_closed_surface_check_catches_a_dropped_triangle(cfg):
    table = mesh.mc_table()
    table[cfg] = table[cfg][1:]
    assert _fails_somewhere(table)


# ---- 4. the analytic sphere --------------------------------------------------------------------------------------------------------------------------------

def _sphere_geometry(g):
    X, Y, Z = g.dims
    c = np.stack(np.meshgrid(*[mesh.centres(g.voxel, n) for n in (X, Y, Z)], indexing="ij"), -1).reshape(-1, 3)
    return c, np.linalg.norm(c.astype(np.float64) + g.origin, axis=1)        # the sensor sits at the world origin


def sphere_bound(g):
    """s^2 / (8 (R - s)) + delta: the linear interpolation of R - |x| along an edge of length s (second derivative at most 1 / (R - s)), and delta
    for the float32 roundings: r32 (2^-24 r <= 2^-24 E), the tsdf (2^-24 |d|, d <= 1, which moves the crossing by at most 2^-24 trunc) and the
    vertex (2^-24 |p| <= 2^-24 G per coordinate norm), with E the largest distance of a voxel centre from the sensor and G the norm of the grid's
    extent; 1e-12 covers the float64 steps."""
    s, R = g.voxel, mcs.SPHERE_R
    c, r = _sphere_geometry(g)
    E, G = float(r.max()), float(np.linalg.norm(np.array(g.dims) * s))
    return s * s / (8.0 * (R - s)) + U24 * (E + g.trunc + G) + 1e-12


def test_the_analytic_sphere():
    g, margin = mcs.sphere_reference()
    assert margin >= mcs.MARGIN
    s, R, trunc = g.voxel, mcs.SPHERE_R, g.trunc
    c, r = _sphere_geometry(g)
    fr = mcs.sphere_frames()
    T = mesh.grid2sensor(g.origin, fr["sensor2world"])
    sees, r32s = [], []
    for f in range(2):
        pix, r32, drop, _ = mesh.project_centres(c, 16, 32, fr["inclination"], "KITTI", None, T[f], 0.0, 80.0)
        sees.append((drop == ri.KEEP) & ((R - r32.astype(np.float64)) >= -trunc))
        r32s.append(r32)
    both = sees[0] & sees[1]
    assert np.array_equal(r32s[0][both], r32s[1][both])                         # the roll permutes the coordinates: the same range
    w = g.weight.numpy().reshape(-1)
    assert np.array_equal(w, sees[0].astype(np.int32) + sees[1].astype(np.int32))
    r32 = np.where(sees[0], r32s[0], r32s[1]).astype(np.float64)
    seen = w > 0
    want = np.minimum(1.0, (R - r32) / trunc).astype(np.float32)
    assert np.array_equal(g.tsdf.numpy().reshape(-1)[seen], want[seen])
    assert np.all(g.tsdf.numpy().reshape(-1)[~seen] == 0)
    assert np.all(w[np.abs(r - R) < trunc] > 0)                                 # coverage
    inten = g.intensity.numpy().reshape(-1)
    assert both.any() and np.all(inten[both] == 0.5)
    m = mesh.extract_reference(g)
    assert closed_surface_errors(m) == [] and euler(m) == 2
    p = m.world()
    err = np.abs(np.linalg.norm(p, axis=1) - R)
    bound = sphere_bound(g)
    print("sphere: largest | |p| - R |", float(err.max()), "bound", bound)
    assert float(err.max()) <= bound
    f = m.faces.numpy()
    nrm = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    assert np.all(np.einsum("ij,ij->i", nrm, -p[f].mean(1)) > 0)              # inside is free space: the normals point at the sensor


def test_the_sphere_bound_catches_the_wrong_interpolation(monkeypatch):
    g, _ = mcs.sphere_reference()
    monkeypatch.setattr(mesh, "_vertex_t", lambda da, db: db / (da - db))
    m = mesh.extract_reference(g)
    err = np.abs(np.linalg.norm(m.world(), axis=1) - mcs.SPHERE_R)
    assert float(err.max()) > sphere_bound(g)


# ---- 5. the rule header on the host -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mesh_check") / "mesh_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "host_check", "mesh_check.cpp")])
    return exe


@pytest.mark.parametrize("conv", mcs.CONVENTIONS)
def test_the_rule_header_is_the_twin_bit_for_bit(host_check, tmp_path, conv):
    dims, (H, W), F = (17, 19, 23), (8, 64), 3
    before, _ = mcs.room_reference(dims, F, H, W, conv)                         # the state after one call: the second call starts from it
    after, margin = mcs.room_reference(dims, F, H, W, conv, True, 2)
    assert margin >= mcs.MARGIN
    fr = mcs.room_frames(F, H, W, conv, 1)
    T = mesh.grid2sensor(before.origin, fr["sensor2world"])
    inc = np.asarray(fr["inclination"], np.float64)
    off, yaw = ri.convention(fr["data_type"], fr["sensor2ego"])
    N = math.prod(dims)
    vox = np.random.default_rng(7).choice(N, 1500, replace=False).astype(np.int32)
    v, ax = mesh.emitted_edges(before)                                          # the vertex rule reads the input state
    assert v.size > 50
    edges = np.stack([v, ax], 1).astype(np.int32)
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as fh:
        fh.write(struct.pack("<12i", *dims, F, H, W, inc.size, vox.size, v.size, 1, 0, 0))
        fh.write(struct.pack("<8d", before.voxel, before.trunc, off, yaw, 0.0, 80.0, 0.0, 0.0))
        for a in (T, inc, fr["depth"].numpy(), fr["mask"].numpy().astype(np.uint8), fr["intensity"].numpy()):
            fh.write(np.ascontiguousarray(a).tobytes())
        fh.write(before.tsdf.numpy().tobytes()); fh.write(before.weight.numpy().tobytes()); fh.write(before.intensity.numpy().tobytes())
        fh.write(vox.tobytes()); fh.write(edges.tobytes())
    res = subprocess.run([host_check, inp, out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "MESHCHECK ok" in res.stdout, res.stdout + res.stderr
    raw = np.fromfile(out, np.uint8)
    n = vox.size
    ts, wt, it = (raw[4 * n * k:4 * n * (k + 1)].view(dt) for k, dt in enumerate((np.float32, np.int32, np.float32)))
    assert np.array_equal(ts.view(np.uint32), after.tsdf.numpy().reshape(-1)[vox].view(np.uint32))
    assert np.array_equal(wt, after.weight.numpy().reshape(-1)[vox])
    assert np.array_equal(it.view(np.uint32), after.intensity.numpy().reshape(-1)[vox].view(np.uint32))
    rest = raw[12 * n:]
    vert = rest[:12 * v.size].view(np.float32).reshape(-1, 3)
    vint = rest[12 * v.size:].view(np.float32)
    m = mesh.extract_reference(before)
    assert np.array_equal(vert.view(np.uint32), m.vertices.numpy().view(np.uint32))
    assert np.array_equal(vint.view(np.uint32), m.intensity.numpy().view(np.uint32))


# ---- 6. the command line on the CPU ------------------------------------------------------------------------------------------------------------------------

CUBE_CENTRE, CUBE_SIZE, BOX_SIZE = np.array([4.0, 0.5, -0.1]), 1.0, 1.6


def cube_depth(d_local, P):
    """The room's ranges with an axis-aligned cube (an actor) in it."""
    base = rc.room_depth(d_local, P).numpy().astype(np.float64)
    d = d_local.numpy().astype(np.float64) @ P[:3, :3].T
    o = P[:3, 3]
    lo, hi = CUBE_CENTRE - CUBE_SIZE / 2 - o, CUBE_CENTRE + CUBE_SIZE / 2 - o
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = lo / d, hi / d
    tn, tf = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
    hit = (tn <= tf) & (tn > 0)
    return torch.from_numpy(np.where(hit, np.minimum(tn, base), base).astype(np.float32))


def write_room_sequence(root, cube=False):
    H, W, inc = 16, 128, list(rc.BOUNDS)
    d_local = rc.local_directions(H, W, inc, "KITTI", None)
    rng = np.random.default_rng(3)
    frames = []
    for f in range(3):
        P = rc.exp4(rc.twist(60 + f, 0.5 + 0.3 * f, 3.0))
        d = cube_depth(d_local, P) if cube else rc.room_depth(d_local, P)
        m = torch.isfinite(d) & (d > 0)
        frames.append(dict(id=f, depth=torch.where(m, d, torch.zeros_like(d)), intensity=torch.from_numpy(rng.uniform(0, 1, (H, W)).astype(np.float32)),
                           mask=m, inclination=inc, sensor2world=P.astype(np.float32)))
    boxes = None
    if cube:
        boxes = dict(frames=[0, 1, 2], translation=np.tile(CUBE_CENTRE, (1, 3, 1)), quaternion=np.tile([1.0, 0.0, 0.0, 0.0], (1, 3, 1)),
                     valid=np.ones((1, 3), bool), size=np.full((1, 3), BOX_SIZE))
    sequence.write_sequence(root, frames, "KITTI", boxes=boxes)
    return root


def cli_reference(root, out_dir, extra=()):
    """The mesh the command line must write, computed through the module's twins, and its margin."""
    rep = json.load(open(os.path.join(out_dir, "mesh.json")))
    meta, frames, inc = mesh.load_frames(root, "train", "--static-only" in extra)
    gr = rep["grid"]
    g = mesh.TsdfGrid(gr["origin"], gr["voxel"], gr["dims"], gr["trunc"], "cpu", intensity=True)
    st = lambda k, dt: torch.from_numpy(np.stack([f[k] for f in frames]).astype(dt))
    margin = mesh.integrate_reference(g, st("depth", np.float32), st("mask", np.bool_), np.stack([f["sensor2world"] for f in frames]),
                                      (float(inc[0]), float(inc[1])), "KITTI", None, st("intensity", np.float32), 0.0, 80.0)
    return mesh.extract_reference(g), margin, rep


def run_cli(root, out_dir, device, extra=()):
    out = os.path.join(out_dir, "mesh.ply")
    mesh.main(["--data", root, "--out", out, "--voxel", "0.3", "--device", device] + list(extra))
    return out


def test_the_command_line_on_the_cpu_writes_the_twins_mesh(tmp_path):
    root = write_room_sequence(str(tmp_path / "seq"))
    out = run_cli(root, str(tmp_path / "cpu"), "cpu")
    want, margin, rep = cli_reference(root, str(tmp_path / "cpu"))
    assert margin >= mcs.MARGIN
    ply = mesh.read_ply(out)
    assert want.faces.shape[0] > 1000
    assert np.array_equal(ply.points, want.world()) and np.array_equal(ply.faces, want.faces.numpy())
    assert np.array_equal(ply.intensity.view(np.uint32), want.intensity.numpy().view(np.uint32))
    assert rep["totals"]["vertices"] == want.vertices.shape[0] and rep["totals"]["faces"] == want.faces.shape[0]
    assert rep["frames"] == [0, 1, 2] and all(rep["pixels"][str(i)]["excluded"] == 0 for i in range(3))
    assert rep["grid"]["trunc"] == pytest.approx(0.9) and rep["grid"]["voxel"] == 0.3


def test_static_only_leaves_no_vertex_inside_the_box(tmp_path):
    root = write_room_sequence(str(tmp_path / "seq"), cube=True)
    inside = lambda p: np.all(np.abs(p - CUBE_CENTRE) < BOX_SIZE / 2, axis=1)
    plain = mesh.read_ply(run_cli(root, str(tmp_path / "plain"), "cpu"))
    assert inside(plain.points).sum() > 20                                        # the control: the actor's surface is there without the flag
    out = run_cli(root, str(tmp_path / "static"), "cpu", ["--static-only"])
    ply = mesh.read_ply(out)
    want, margin, rep = cli_reference(root, str(tmp_path / "static"), ["--static-only"])
    assert margin >= mcs.MARGIN
    assert np.array_equal(ply.points, want.world()) and np.array_equal(ply.faces, want.faces.numpy())
    assert sum(rep["pixels"][str(i)]["excluded"] for i in range(3)) > 0
    assert inside(ply.points).sum() == 0


def test_a_grid_above_max_voxels_is_refused_with_its_size(tmp_path):
    root = write_room_sequence(str(tmp_path / "seq"))
    with pytest.raises(SystemExit, match=r"the grid needs \d+ x \d+ x \d+ = \d+ voxels"):
        mesh.main(["--data", root, "--out", str(tmp_path / "m.ply"), "--voxel", "0.3", "--device", "cpu", "--max-voxels", "1000"])


def test_ply_round_trip(tmp_path):
    m = mesh.extract_reference(mcs.random_grid(0))
    mesh.write_ply(str(tmp_path / "a.ply"), m)
    p = mesh.read_ply(str(tmp_path / "a.ply"))
    assert np.array_equal(p.points, m.world()) and np.array_equal(p.faces, m.faces.numpy()) and np.array_equal(p.intensity, m.intensity.numpy())


# ---- 7. the library: its build entry, exports and resource gate, refused arguments -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mesh_lib():
    from lidar_rt_amd import build as lrt_build
    return lrt_build.build_mesh()


def test_the_library_builds_and_exports_what_its_header_declares(mesh_lib):
    from lidar_rt_amd import build as lrt_build
    REPO = os.path.dirname(HERE)
    assert os.path.exists(mesh_lib) and not lrt_build.mesh_is_stale()
    assert lrt_build.MESH_SOURCES == ["lrt_mesh.hip"] and "lrt_mesh_tables.h" in lrt_build.MESH_HEADERS and "lrt_project_math.h" in lrt_build.MESH_HEADERS
    src = open(lrt_build.__file__).read()
    assert "build_mesh(force, verbose)" in src[src.index("def _build_product"):src.index("def _build_lib")]
    assert "csrc/liblrt_mesh.so" in open(os.path.join(REPO, "setup.py")).read()
    hdr = open(os.path.join(REPO, "include", "lrt_mesh.h")).read()
    declared = set(re.findall(r"\b(lrt_mesh_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(mesh.EXPORTS), declared ^ set(mesh.EXPORTS)
    exported = set(re.findall(r"\blrt_mesh_[a-z_]+\b", subprocess.run(["nm", "-D", "--defined-only", mesh_lib], capture_output=True, text=True, check=True).stdout))
    assert exported == declared, exported ^ declared
    lib = mesh.load()
    assert lib.lrt_mesh_abi_version() == int(re.search(r"#define\s+LRT_MESH_ABI_VERSION\s+(\d+)", hdr).group(1)) == mesh.ABI_VERSION
    for name, val in (("BLOCK", mesh.BLOCK), ("SCAN_PASS", mesh.SCAN_PASS), ("MAX_FRAMES", mesh.MAX_FRAMES)):
        assert int(re.search(rf"#define\s+LRT_MESH_{name}\s+(\d+)", hdr).group(1)) == val, name
    assert lib.lrt_mesh_work_bytes(0, 3, 3) < 0 and lib.lrt_mesh_work_bytes(65536, 65536, 1) < 0
    assert lib.lrt_mesh_work_bytes(17, 19, 23) % 256 == 0 and lib.lrt_mesh_work_bytes(17, 19, 23) >= 10 * 17 * 19 * 23


def test_the_kernels_pass_the_resource_gate(mesh_lib):
    from lidar_rt_amd import resources
    res = resources.kernel_resources(mesh_lib)
    own = sorted(n for n in res if resources.is_own_kernel(n))
    assert own == ["k_mesh_count", "k_mesh_faces", "k_mesh_integrate", "k_mesh_scan", "k_mesh_vertices"], own
    assert all(any(re.search(g_, n) for g_ in resources.GATED) for n in own)
    assert resources.violations(res) == []


INTEGRATE_ARGS = ("device", "X", "Y", "Z", "voxel", "trunc", "tsdf", "weight", "intensity", "F", "T", "H", "W", "depth", "mask", "fint", "inclination",
                  "n_inc", "off", "yaw", "min_depth", "max_depth", "stream")


def test_argument_errors_come_before_the_device_and_launch_nothing(mesh_lib):
    """Non-null dummy pointers and device 99: a refused argument is reported first; valid arguments reach the device check, which refuses too."""
    lib = mesh.load()
    ok = dict(device=99, X=3, Y=3, Z=3, voxel=0.1, trunc=0.3, tsdf=8, weight=8, intensity=None, F=1, T=8, H=4, W=8, depth=8, mask=8, fint=None,
              inclination=8, n_inc=2, off=0.0, yaw=0.0, min_depth=0.0, max_depth=80.0, stream=None)
    call = lambda **kw: lib.lrt_mesh_integrate(*[dict(ok, **kw)[k] for k in INTEGRATE_ARGS])
    for kw, msg in (({"X": 0}, "a grid of 0 x"), ({"voxel": 0.0}, "voxel 0"), ({"F": -1}, "-1 frames"), ({"n_inc": 3}, "3 inclinations"),
                    ({"tsdf": None}, "null tsdf"), ({"intensity": 8}, "go together"), ({"min_depth": 5.0, "max_depth": 1.0}, "depths"),
                    ({"off": 1.0}, "off 1"), ({}, "no HIP device 99")):
        assert call(**kw) == -1, kw
        assert msg in lib.lrt_mesh_last_error().decode(), (kw, lib.lrt_mesh_last_error())
    assert call(F=0) == 0                                                              # nothing to fuse: no launch, not even a device
    assert lib.lrt_mesh_count(99, 3, 3, 3, 8, 8, 1, None, 0, 8, None) == -1 and "workspace" in lib.lrt_mesh_last_error().decode()
    assert lib.lrt_mesh_count(99, 3, 3, 3, 8, 8, 1, 256, 255, 8, None) == -1 and "bytes" in lib.lrt_mesh_last_error().decode()
    assert lib.lrt_mesh_write(99, 3, 3, 3, 0.1, 8, None, 256, 1 << 20, -1, 0, None, None, None, None) == -1
    assert "vertices" in lib.lrt_mesh_last_error().decode()
    for bad in ((lambda: mesh.TsdfGrid((0, 0), 0.1, (2, 2, 2))), (lambda: mesh.TsdfGrid((0, 0, 0), -1.0, (2, 2, 2))),
                (lambda: mesh.extract_reference(mcs.random_grid(0), 0))):
        with pytest.raises(mesh.MeshError):
            bad()
    g = mcs.random_grid(0)
    with pytest.raises(mesh.MeshError, match="go together"):
        mesh.integrate(g, torch.ones(1, 4, 8), torch.ones(1, 4, 8, dtype=torch.bool), np.eye(4)[None], [-0.4, 0.1])
