"""Scene initialisation from range images without a GPU: the fourth product library (`liblrt_init.so`: a source list and hash of its own that
moves no other hash, exports, resource gate), the closed-form eigen routine of `lrt_init_math.h` compiled for the host against
`numpy.linalg.eigh`, the `*_reference` twins of `lidar_rt_amd.scene_init` against hand-written brute force on tiny inputs, and the
`init_from_frames` switch of `sequence.scene_from_sequence` on an analytic sequence (CPU tensors: the twins do the work; `distCUDA2`, which
has no CPU path, is replaced by a brute-force expression for these tests)."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from lidar_rt_amd import build as lrt_build, resources, scene_init as si, sequence, training

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "tools"))


# ---- build ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def init_lib():
    return lrt_build.build_init()


def test_the_library_has_a_source_list_of_its_own_and_moves_no_other_hash():
    assert lrt_build.INIT_SOURCES == ["lrt_init.hip"] and "lrt_init_math.h" in lrt_build.INIT_HEADERS
    others = lrt_build.SOURCES + lrt_build.HEADERS + lrt_build.LOSS_SOURCES + lrt_build.LOSS_HEADERS + lrt_build.GRIDCD_SOURCES + lrt_build.GRIDCD_HEADERS
    assert not any("lrt_init" in f for f in others)
    # the three other libraries' hashes at the commit this library was added on: committed profiles are keyed by them
    assert lrt_build.source_hash() == "2c98b54882a7ff74"          # moved twice since: the non-finite-input fixes in lrt_chamfer.hip; a comment of include/lrt.h (lrt_xchg_apply, zero_only on an overflowed block)
    assert lrt_build.loss_source_hash() == "cc56b0c83f72d5ca"
    assert lrt_build.gridcd_source_hash() == "fd279d9f7ff67722"
    assert lrt_build.init_source_hash() not in (lrt_build.source_hash(), lrt_build.loss_source_hash(), lrt_build.gridcd_source_hash())
    assert os.path.basename(lrt_build.INIT_LIB) == "liblrt_init.so"
    assert lrt_build.INIT_LIB not in (lrt_build.LIB, lrt_build.LOSS_LIB, lrt_build.GRIDCD_LIB)
    assert "build_init(force, verbose)" in open(lrt_build.__file__).read()             # _build_product builds it


def test_the_library_builds_and_exports_what_its_header_declares(init_lib):
    assert os.path.exists(init_lib) and not lrt_build.init_is_stale()
    assert open(lrt_build.INIT_STAMP).read().strip() == lrt_build.init_source_hash()
    hdr = open(os.path.join(REPO, "include", "lrt_init.h")).read()
    declared = set(re.findall(r"\b(lrt_init_[a-z_]+)\s*\(", hdr))
    assert declared == set(si.EXPORTS), declared ^ set(si.EXPORTS)
    lib = si.load()
    for n in declared:
        assert hasattr(lib, n), n
    assert lib.lrt_init_abi_version() == int(re.search(r"#define\s+LRT_INIT_ABI_VERSION\s+(\d+)", hdr).group(1)) == si.ABI_VERSION


def test_every_kernel_passes_the_resource_gate(init_lib):
    res = resources.kernel_resources(init_lib)
    own = sorted(n for n in res if resources.is_own_kernel(n))
    assert len(own) >= 10 and all(n.startswith("k_in_") for n in own), own
    assert all(any(re.search(g_, n) for g_ in resources.GATED) for n in own)
    assert resources.violations(res) == []
    for n in own:
        assert res[n]["vgpr_spill"] == 0 and res[n]["scratch_bytes"] == 0 and not res[n]["dynamic_stack"], (n, res[n])
    resources.check(init_lib)


def test_work_bytes_and_argument_errors_without_a_device(init_lib):
    lib = si.load()
    assert lib.lrt_init_normals_work_bytes(0, 5) == 0 and lib.lrt_init_normals_work_bytes(1 << 14, 1 << 14) == 0
    assert lib.lrt_init_voxel_work_bytes(0) == 0 and lib.lrt_init_voxel_work_bytes(1 << 40) == 0
    nb = lib.lrt_init_normals_work_bytes(66, 1030)
    assert nb >= 66 * 1030 * 16 and nb % 16 == 0 and lib.lrt_init_voxel_work_bytes(1000) >= 3 * 1000 * 4
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    dev = 1 << 20
    for d in ((dev,) if torch.cuda.is_available() else (dev, 0)):
        assert lib.lrt_init_normals(d, 4, 4, p, p, p, p, 6, p, p, p, nb, None) < 0 and b"no HIP device" in lib.lrt_init_last_error()
        assert lib.lrt_init_assign(d, 16, p, p, p, 0, None, None, None, p, p, p, None) < 0 and b"no HIP device" in lib.lrt_init_last_error()
        assert lib.lrt_init_voxel_keys(d, 16, p, 0.1, p, p, p, nb, None) < 0 and b"no HIP device" in lib.lrt_init_last_error()
        assert lib.lrt_init_voxel_mean(d, 16, p, p, p, p, p, p, p, p, p, p, p, nb, None) < 0 and b"no HIP device" in lib.lrt_init_last_error()


# ---- the eigen routine on the host --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def init_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("init_check") / "init_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "host_check", "init_check.cpp")])
    return exe


def run_init_check(exe, cov):
    """(n, 3) eigenvector, (n, 3) eigenvalues, (n,) return value of in_smallest_eigenvector for (n, 3, 3) symmetric matrices."""
    c6 = np.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]], 1).astype(np.float64)
    r = subprocess.run([exe], input=struct.pack("<q", len(cov)) + c6.tobytes(), capture_output=True, check=True, timeout=120)
    out = np.frombuffer(r.stdout, np.float64).reshape(-1, 7)
    return out[:, :3], out[:, 3:6], out[:, 6]


def eigen_cases(kind, n=4000, seed=0):
    """Seeded symmetric test matrices Q diag(l) Q^T: noisy planes (l0 << l1 ~ l2), needles (l0 < l1 << l2) and near-isotropic blobs."""
    rng = np.random.default_rng(seed + {"plane": 1, "needle": 2, "blob": 3}[kind])
    Q = np.linalg.qr(rng.standard_normal((n, 3, 3)))[0]
    if kind == "plane":
        lam = np.stack([10 ** rng.uniform(-8, -3, n), rng.uniform(0.01, 1, n), rng.uniform(0.01, 1, n)], 1)
    elif kind == "needle":
        l0 = 10 ** rng.uniform(-5.5, -4, n)
        lam = np.stack([l0, l0 * rng.uniform(2, 10, n), rng.uniform(0.1, 1, n)], 1)
    else:
        lam = 1 + 0.1 * rng.uniform(-1, 1, (n, 3))
    lam = np.sort(lam, 1) * 10 ** rng.uniform(-3, 3, (n, 1))
    cov = np.einsum("nij,nj,nkj->nik", Q, lam, Q)
    return 0.5 * (cov + cov.transpose(0, 2, 1))


def ill_conditioned(lam):
    return (lam[:, 1] - lam[:, 0]) / np.maximum(lam[:, 2], 1e-300) < 1e-6


def host_distance(exe):
    """The largest 1 - |n . n_ref| between the header's routine and eigh over the well-conditioned cases of the three seeded sets."""
    worst = 0.0
    for kind in ("plane", "needle", "blob"):
        cov = eigen_cases(kind)
        lam, vec = np.linalg.eigh(cov)
        ill = ill_conditioned(lam)
        assert ill.mean() <= 0.01, (kind, ill.mean())                    # the seeded sets keep the numpy path itself under the cap
        n, _, rc = run_init_check(exe, cov)
        assert (rc[~ill] == 1).all() and np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-14)
        worst = max(worst, float((1 - np.abs((n * vec[:, :, 0]).sum(1)))[~ill].max()))
    return worst


def test_smallest_eigenvector_agrees_with_eigh(init_check):
    d = host_distance(init_check)
    print(f"SCENEINIT|host eigenvector distance|{d:.3e}")
    # 1 - cos of an angle of ~2^-53 l2 / (l1 - l0) <= 1e-10 is far below the resolution of the measure itself (a few 2^-53)
    assert d <= 1e-14, d


def test_rank_deficient_matrices_fall_back_to_z(init_check):
    v = np.array([1.0, 2.0, 3.0])
    cov = np.stack([np.zeros((3, 3)), np.diag([2.0, 0.0, 0.0]), np.outer(v, v), np.diag([0.0, 0.0, 5.0]), np.full((3, 3), np.nan)])
    n, lam, rc = run_init_check(init_check, cov)
    assert (rc == 0).all() and np.array_equal(n, np.tile([0.0, 0.0, 1.0], (5, 1)))
    # a plane in exact arithmetic is NOT degenerate: rank 2, the normal is its null vector
    n, lam, rc = run_init_check(init_check, np.diag([3.0, 0.0, 1.0])[None])
    assert rc[0] == 1 and np.array_equal(np.abs(n[0]), [0.0, 1.0, 0.0])


def test_covariance_of_point_lists_on_the_host(init_check):
    rng = np.random.default_rng(5)
    n = 500
    pts = rng.uniform(-30, 30, (n, 8, 3)).astype(np.float32)
    cnt = rng.integers(3, 9, n).astype(np.int32)
    blob = struct.pack("<q", n) + b"".join(pts[i].tobytes() + struct.pack("<i", int(cnt[i])) for i in range(n))
    r = subprocess.run([init_check, "cov"], input=blob, capture_output=True, check=True, timeout=120)
    out = np.frombuffer(r.stdout, np.float64).reshape(-1, 7)
    worst = 0.0
    for i in range(n):
        q = pts[i, :cnt[i]].astype(np.float64)
        lam, vec = np.linalg.eigh(np.cov(q.T, bias=True))
        worst = max(worst, 1 - abs(float(out[i, :3] @ vec[:, 0])))
    assert worst <= 1e-12, worst


# ---- the twins against hand-written brute force -------------------------------------------------------------------------------------------------

def _f32_d2(c, q):
    d = (c - q).astype(np.float32).astype(np.float64)
    t = np.float32(d[0] * d[0]); t = np.float32(d[1] * d[1] + np.float64(t)); return np.float32(d[2] * d[2] + np.float64(t))


def _brute_lists(pts, mask, k):
    HW = pts.shape[0]
    out = np.full((HW, 8), -1, np.int64)
    vi = [i for i in range(HW) if mask[i]]
    for i in vi:
        pairs = sorted((float(_f32_d2(pts[j], pts[i])), j) for j in vi)
        for s, (_, j) in enumerate(pairs[:k]):
            out[i, s] = j
    return out


def test_neighbour_order_with_a_constructed_tie():
    # a 3 x 4 grid of points on the integer lattice, one duplicated point and one masked pixel: ties decide
    H, W = 3, 4
    o = torch.zeros(H, W, 3)
    d = torch.tensor([[[float(x), float(y), 0.0] for x in range(W)] for y in range(H)])
    d[2, 3] = d[0, 0]                                                              # pixel 11 duplicates pixel 0
    r = torch.ones(H, W)
    m = torch.ones(H, W, dtype=torch.bool); m[1, 1] = False
    for k in (6, 4, 3):
        nrm, nbr = si.estimate_normals_reference(o, d, r, m, k)
        want = _brute_lists((o + d * r[..., None]).reshape(-1, 3).numpy(), m.reshape(-1).numpy(), k)
        assert np.array_equal(nbr.reshape(-1, 8).numpy(), want), k
    nbr = nbr.reshape(-1, 8)
    assert nbr[0, :2].tolist() == [0, 11] and nbr[11, :2].tolist() == [0, 11]      # distance 0 twice: the lower pixel index first
    assert nbr[5].tolist() == [-1] * 8 and (nbr[:, 3:] == -1).all()                # masked pixel; nothing beyond k = 3
    assert nbr[6, :3].tolist() == [6, 2, 7]                                        # (2,1): itself, then distance 1 to pixels 2, 7, 10 (5 is masked): lowest first
    # all points in the plane z = 0: rank 2 wherever the list is not collinear, normal +-z facing the sensor at the origin... which lies IN the plane:
    # the dot product is exactly 0 and the first non-zero component decides
    n6 = si.estimate_normals_reference(o, d, r, m, 6)[0]
    assert torch.equal(n6[0, 1], torch.tensor([0.0, 0.0, 1.0])) and float(n6[1, 1].abs().sum()) == 0.0
    # two valid pixels: fewer than 3 listed points
    m2 = torch.zeros(H, W, dtype=torch.bool); m2[0, 1] = m2[2, 2] = True
    n2, l2 = si.estimate_normals_reference(o, d, r, m2, 6)
    assert l2[0, 1].tolist() == [1, 10] + [-1] * 6 and torch.equal(n2[0, 1], torch.tensor([0.0, 0.0, 1.0]))


def test_normals_face_the_sensor_and_match_a_known_plane():
    rng = np.random.default_rng(2)
    H, W = 6, 9
    o = torch.tensor([0.3, -0.2, 1.0]).expand(H, W, 3).contiguous()
    nrm_true = np.array([0.2, -0.1, 1.0]); nrm_true /= np.linalg.norm(nrm_true)
    d = rng.standard_normal((H, W, 3)); d[..., 2] = -np.abs(d[..., 2]) - 0.5; d /= np.linalg.norm(d, axis=-1, keepdims=True)
    t = (-2.0 - o.numpy().astype(np.float64) @ nrm_true) / (d @ nrm_true)           # the plane n . p = -2
    n, nbr = si.estimate_normals_reference(o, torch.as_tensor(d, dtype=torch.float32), torch.as_tensor(t, dtype=torch.float32), torch.ones(H, W, dtype=torch.bool))
    assert float((n.double() @ torch.as_tensor(nrm_true)).min()) > 1 - 1e-6       # up: towards the sensor
    p = o + torch.as_tensor(d, dtype=torch.float32) * torch.as_tensor(t, dtype=torch.float32)[..., None]
    assert float(((o - p).double() * n.double()).sum(-1).min()) >= 0.0


def _poses():
    s = np.sqrt(0.5)
    return (torch.tensor([[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], [0.5, 0.0, 0.0, 3.0 * s, 0.0, 0.0, 3.0 * s], [9.0, 9.0, 9.0, 1.0, 0.0, 0.0, 0.0]]),
            torch.tensor([[2.0, 2.0, 2.0], [4.0, 1.5, 2.0], [100.0, 100.0, 100.0]]), torch.tensor([1, 1, 0], dtype=torch.uint8))


def test_assignment_strict_face_first_actor_and_absent_actor():
    poses, sizes, present = _poses()              # actor 1: yaw 90 degrees, un-normalised quaternion; actor 2 would hold everything but is absent
    pts = torch.tensor([[0.5, 0.5, 0.5],          # in both boxes: the first wins
                        [1.0, 0.0, 0.0],          # ON actor 0's face (strict <): not actor 0, so actor 1 gets it (local (0, -0.5, 0))
                        [0.5, 1.5, 0.0],          # only in actor 1: local = R^T (p - t) = (1.5, 0, 0)
                        [5.0, 5.0, 5.0],          # in no present box
                        [0.0, 0.0, 0.0]])         # masked out
    nrm = torch.tensor([[1.0, 0.0, 0.0]] * 5)
    mask = torch.tensor([1, 1, 1, 1, 0], dtype=torch.bool)
    label, lp, ln = si.assign_to_boxes_reference(pts, nrm, mask, poses, sizes, present)
    assert label.tolist() == [1, 2, 2, 0, -1]
    assert torch.equal(lp[0], pts[0]) and torch.allclose(lp[1], torch.tensor([0.0, -0.5, 0.0]), atol=1e-6) and torch.equal(lp[3], pts[3]) and torch.equal(lp[4], pts[4])
    assert torch.allclose(lp[2], torch.tensor([1.5, 0.0, 0.0]), atol=1e-6) and torch.allclose(ln[2], torch.tensor([0.0, -1.0, 0.0]), atol=1e-6)
    # just inside the face: in
    pts[1, 0] = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    assert si.assign_to_boxes_reference(pts, nrm, mask, poses, sizes, present)[0].tolist() == [1, 1, 2, 0, -1]
    # no actors at all: every valid pixel is background
    lab0 = si.assign_to_boxes_reference(pts, nrm, mask, None, None, None)[0]
    assert lab0.tolist() == [0, 0, 0, 0, -1]


def test_voxel_mean_origin_key_order_and_unrenormalised_normals():
    # voxel 1 m; minimum (0, 0, 0) -> origin (-0.5, -0.5, -0.5): a point at 0.4 shares the voxel of the minimum, one at 0.6 does not
    pts = torch.tensor([[0.6, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.6], [0.4, 0.4, 0.4], [0.0, 0.7, 0.0], [0.45, 0.0, 0.0]])
    inten = torch.tensor([1.0, 0.2, 0.3, 0.4, 0.5, 0.9])
    nrm = torch.tensor([[1.0, 0, 0], [0, 0, 1.0], [0, 1.0, 0], [0, 0, -1.0], [1.0, 0, 0], [1.0, 0, 0]])
    keys = si.voxel_keys_reference(pts, 1.0)
    assert keys.tolist() == [1 << 42, 0, 1, 0, 1 << 21, 0]
    p, i, n, c = si.voxel_downsample_reference(pts, inten, nrm, 1.0)
    assert c.tolist() == [3, 1, 1, 1]                                             # ascending key: (0,0,0), (0,0,1), (0,1,0), (1,0,0)
    assert torch.allclose(p[0], torch.tensor([0.85 / 3, 0.4 / 3, 0.4 / 3])) and torch.equal(p[1], pts[2]) and torch.equal(p[2], pts[4]) and torch.equal(p[3], pts[0])
    assert torch.allclose(i, torch.tensor([0.5, 0.3, 0.5, 1.0]))
    assert torch.allclose(n[0], torch.tensor([1.0 / 3, 0.0, 0.0]), atol=1e-7)     # (0,0,1) + (0,0,-1) + (1,0,0) over 3: not a unit vector
    # one voxel more than 21 bits hold: an error, not a wrap
    far = torch.tensor([[0.0, 0.0, 0.0], [float(1 << 21), 0.0, 0.0]])
    with pytest.raises(si.SceneInitError, match="2\\^21"):
        si.voxel_downsample_reference(far, torch.zeros(2), torch.zeros(2, 3), 1.0)
    ok = torch.tensor([[0.0, 0.0, 0.0], [float((1 << 21) - 1), 0.0, 0.0]])
    assert si.voxel_downsample_reference(ok, torch.zeros(2), torch.zeros(2, 3), 1.0)[3].tolist() == [1, 1]


def test_hip_entry_points_refuse_bad_arguments():
    o, d, r, m = torch.zeros(4, 4, 3), torch.ones(4, 4, 3), torch.ones(4, 4), torch.ones(4, 4, dtype=torch.bool)
    with pytest.raises(si.SceneInitError, match="k = 9"):
        si.estimate_normals(o, d, r, m, k=9)
    with pytest.raises(si.SceneInitError, match="voxel_size"):
        si.voxel_downsample(torch.zeros(3, 3), torch.zeros(3), torch.zeros(3, 3), 0.0)


# ---- the switch -------------------------------------------------------------------------------------------------------------------------------------

def _cpu_dist2(points):
    """distCUDA2 restated for CPU tensors: the mean squared distance to the three nearest other points."""
    d = torch.cdist(points.double(), points.double()) ** 2
    d.fill_diagonal_(float("inf"))
    return d.topk(min(3, points.shape[0] - 1), dim=1, largest=False).values.mean(1).float()


@pytest.fixture()
def cpu_knn(monkeypatch):
    from lidar_rt_amd.simple_knn import _C
    monkeypatch.setattr(_C, "distCUDA2", _cpu_dist2)


def _parent_scene_from_sequence(seq, max_sh_degree=3, max_points=2_000_000, seed=0):
    """What scene_from_sequence did before the switch existed, restated: the yardstick of `switch off`."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    rf, dev = seq.frames, next(iter(seq.frames.depth.values())).device
    if "background" in seq.init:
        c = seq.init["background"]; pts, inten, nrm = c["points"], c["intensity"], c.get("normals")
    else:
        pts = torch.cat([rf.inverse_projection_with_range(f, rf.get_depth(f)) for f in seq.train_frames])
        inten, nrm = torch.cat([rf.get_intensity(f).reshape(-1).index_select(0, rf.mask_index[f]) for f in seq.train_frames]), None
        if pts.shape[0] > max_points:
            sel = torch.randperm(pts.shape[0], generator=g)[:max_points].to(dev); pts, inten = pts[sel], inten[sel]
    assets = [training.GaussianAsset.from_points(pts, inten.clamp(0, 1), nrm, max_sh_degree=max_sh_degree, extent=float(seq.meta.get("extent", 1.0)))]
    for a, tb in enumerate(seq.boxes):
        c = seq.init.get(f"actor_{a:02d}")
        if c is not None:
            p_, i_, n_ = c["points"], c["intensity"], c.get("normals")
        else:
            u = torch.rand((2000, 3), generator=g).to(dev)
            p_, i_, n_ = tb.min_xyz + u * (tb.max_xyz - tb.min_xyz), torch.full((2000,), 0.5, device=dev), None
        assets.append(training.GaussianAsset.from_points(p_, i_.clamp(0, 1), n_, max_sh_degree=max_sh_degree, bounding_box=tb,
                                                         extent=float((tb.max_xyz - tb.min_xyz).norm())))
    return training.GaussianScene(assets)


def _tensors(scene):
    return [t.detach() for a in scene.gaussians_assets for t in (a._xyz, a._features_dc, a._features_rest, a._scaling, a._rotation, a._opacity)]


@pytest.fixture(scope="module")
def seq_dir(tmp_path_factory):
    import bench_scene_init
    root = str(tmp_path_factory.mktemp("seq") / "plain")
    bench_scene_init.write_analytic_sequence(root, 8, 64, n_frames=3, n_actors=2)
    return root


def test_switch_off_builds_the_parents_scene(seq_dir, cpu_knn):
    seq = sequence.load_sequence(seq_dir, "cpu")
    for max_points in (2_000_000, 300):
        torch.manual_seed(3); want = _parent_scene_from_sequence(seq, max_points=max_points, seed=5)
        torch.manual_seed(3); have = sequence.scene_from_sequence(seq, max_points=max_points, seed=5)
        torch.manual_seed(3); have2 = sequence.scene_from_sequence(seq, max_points=max_points, seed=5, init_from_frames=False, voxel_size=0.3, k=4)
        for w, h, h2 in zip(_tensors(want), _tensors(have), _tensors(have2)):
            assert torch.equal(w, h) and torch.equal(w, h2)
        assert [a.extent for a in want.gaussians_assets] == [a.extent for a in have.gaussians_assets]
    assert not hasattr(seq, "init_report")


def test_switch_on_uses_real_returns_normals_and_keeps_given_clouds(seq_dir, cpu_knn, tmp_path):
    import bench_scene_init
    seq = sequence.load_sequence(seq_dir, "cpu")
    clouds = si.init_clouds(seq, k=6, voxel_size=0.15, obj_pt_num=200, seed=1)
    again = si.init_clouds(seq, k=6, voxel_size=0.15, obj_pt_num=200, seed=1)
    assert set(clouds) == {"background", "actor_00", "actor_01"}
    for name in clouds:
        for key in ("points", "intensity", "normals"):
            assert torch.equal(clouds[name][key], again[name][key]), (name, key)
    bgc = clouds["background"]
    assert bgc["points"].shape[0] > 100 and bgc["normals"].shape == bgc["points"].shape
    nz = bgc["normals"][:, 2]
    assert float((nz > 0.99).float().mean()) > 0.9                                 # the ground plane's returns: normals up, towards the sensor
    total = sum(int(seq.frames.mask[f].sum()) for f in seq.train_frames)
    assert bgc["points"].shape[0] < total                                          # the voxel mean merged returns of three frames
    for a in (0, 1):
        c = clouds[f"actor_{a:02d}"]
        assert c["points"].shape[0] == 200 and c["real"] > 0
        half = 0.5 * (seq.boxes[a].max_xyz - seq.boxes[a].min_xyz)
        assert bool((c["points"].abs() < half).all())                              # actor-frame coordinates inside the tracking box
        real_i = c["intensity"][:c["real"]] if c["real"] < 200 else c["intensity"]
        assert float(real_i.max()) > 0.5 or c["real"] == 200                       # the bodies' recorded intensity (0.8), not the padding's 0.5
    # the scene: normals reach from_points (flat quaternions aligned with them), actors start from their returns
    torch.manual_seed(0); s1 = sequence.scene_from_sequence(seq, seed=1, init_from_frames=True)
    torch.manual_seed(0); s2 = sequence.scene_from_sequence(seq, seed=1, init_from_frames=True)
    for x, y in zip(_tensors(s1), _tensors(s2)):
        assert torch.equal(x, y)
    assert s1.gaussians_assets[0]._xyz.shape[0] == bgc["points"].shape[0]
    R = training._rotation_matrix(s1.gaussians_assets[0]._rotation.detach())
    assert float((R[:, :, 2] * bgc["normals"]).sum(1).min()) > 1 - 1e-4            # third axis = the estimated normal
    assert seq.init_report["actor_00"]["real"] > 0 and seq.init_report["background"]["points"] == bgc["points"].shape[0]
    # --max-points still caps the background
    torch.manual_seed(0)
    assert sequence.scene_from_sequence(seq, seed=1, init_from_frames=True, max_points=50).gaussians_assets[0]._xyz.shape[0] == 50
    # clouds under DIR/init win; only the missing ones come from the frames
    given = {"background": {"points": np.random.default_rng(0).uniform(-5, 5, (40, 3)), "intensity": np.full(40, 0.25)},
             "actor_01": {"points": np.random.default_rng(1).uniform(-0.5, 0.5, (30, 3)), "intensity": np.full(30, 0.75)}}
    root = str(tmp_path / "with_init")
    bench_scene_init.write_analytic_sequence(root, 8, 64, n_frames=3, n_actors=2, init=given, with_extent=False)
    seq2 = sequence.load_sequence(root, "cpu")
    torch.manual_seed(0); s3 = sequence.scene_from_sequence(seq2, seed=1, init_from_frames=True)
    assert torch.equal(s3.gaussians_assets[0]._xyz.detach(), seq2.init["background"]["points"].float())
    assert torch.equal(s3.gaussians_assets[2]._xyz.detach(), seq2.init["actor_01"]["points"].float())
    assert s3.gaussians_assets[1]._xyz.shape[0] == 2000 and set(seq2.init_report) == {"actor_00"} and seq2.init_report["actor_00"]["real"] > 0
    # without `extent` in meta.json and without a given background, the extent is the reference's quantile rule
    root = str(tmp_path / "no_extent")
    bench_scene_init.write_analytic_sequence(root, 8, 64, n_frames=3, n_actors=0, with_extent=False)
    seq3 = sequence.load_sequence(root, "cpu")
    torch.manual_seed(0); s4 = sequence.scene_from_sequence(seq3, seed=1, init_from_frames=True)
    pts = s4.gaussians_assets[0]._xyz.detach().double().numpy()
    want = float(int(np.quantile(2 * np.linalg.norm(pts - pts.mean(0), axis=1), 0.9)))
    assert s4.gaussians_assets[0].extent == want and want >= 1.0


def test_train_has_the_three_flags():
    from lidar_rt_amd import train
    src = open(train.__file__).read()
    for flag in ('"--init-from-frames"', '"--voxel-size"', '"--init-knn"'):
        assert flag in src
    assert "init_from_frames=bool(args.init_from_frames)" in src
