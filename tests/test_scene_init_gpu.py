"""Scene initialisation from range images on the GPU (lidar_rt_amd.scene_init, liblrt_init.so): neighbour lists equal to brute force exactly,
normals against float64 eigh on the same lists, the sign rule and the fall-backs, the split by tracking box and the voxel mean against their
float64 twins, outputs written whole, repeatability, stream order, and `python -m lidar_rt_amd.train --init-from-frames` end to end.

Measured lines (`SCENEINIT|...`) are printed before the assertions (run with -s); profiles/scene_init.md records them."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from lidar_rt_amd import scene_init as si, scenes

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "tools"))
DEV = torch.device("cuda:0")
SIZES = [(5, 7), (11, 200), (16, 256), (66, 1030)]
MASKS = ["all", "drop30", "none", "two", "five"]
CLOUDS = ["coherent", "incoherent", "lattice"]


def _case(H, W, mask, cloud, seed=0):
    """(o, d, range, mask) on the device, float32 / bool."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    o, d = scenes.kitti_rays(H, W, origin=(1.5, -2.0, 0.7))
    if cloud == "coherent":                                                  # wavy planes
        r = (6.0 + 30.0 * rng.uniform(size=(H, 1)) + 3.0 * np.sin(np.arange(W) / 9.0)[None, :] + rng.uniform(0, 0.5, (H, W))).astype(np.float32)
    elif cloud == "incoherent":                                              # independent random ranges: the search degenerates towards brute force
        r = rng.uniform(1, 80, (H, W)).astype(np.float32)
    else:                                                                    # lattice: rays quantised to a coarse grid at one range: duplicated points, equal distances
        d = np.round(d * 2) / 2
        d[np.abs(d).sum(-1) == 0] = (1.0, 0.0, 0.0)
        d = d.astype(np.float32); o = np.zeros_like(o)
        r = np.full((H, W), 4.0, np.float32)
    m = np.ones((H, W), bool)
    if mask == "drop30":
        m = rng.uniform(size=(H, W)) >= 0.3
    elif mask == "none":
        m[:] = False
    elif mask in ("two", "five"):
        m[:] = False
        m.reshape(-1)[rng.choice(H * W, 2 if mask == "two" else 5, replace=False)] = True
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=DEV)
    return t(o), t(d), t(r), t(m)


def _sample(H, W, n=4096, seed=0):
    """Linear pixel indices: every pixel of a small image; of a large one a seeded sample that holds pixels of all four borders."""
    if H * W <= n:
        return None
    g = torch.Generator().manual_seed(seed)
    top, bottom = torch.arange(0, W, 9), (H - 1) * W + torch.arange(0, W, 9)
    left, right = torch.arange(H) * W, torch.arange(H) * W + W - 1
    border = torch.unique(torch.cat([top, bottom, left, right]))
    rest = torch.randperm(H * W, generator=g)[: n - border.shape[0]]
    return torch.cat([border, rest]).to(DEV)


@pytest.mark.parametrize("H,W", SIZES)
def test_neighbour_lists_equal_brute_force_exactly(H, W):
    q = _sample(H, W)
    ties = 0
    for mask in MASKS:
        for cloud in CLOUDS:
            o, d, r, m = _case(H, W, mask, cloud)
            pts = o + d * r[..., None]
            want8 = si.neighbours_reference(pts, m, 8, queries=q, pairs=1 << 25)      # one scan: the list for k is its first k entries
            want8 = want8.reshape(-1, 8)
            for k in (6, 4):
                nbr = si.estimate_normals(o, d, r, m, k)[1].reshape(-1, 8)
                have = nbr if q is None else nbr.index_select(0, q)
                want = want8.clone(); want[:, k:] = -1
                assert torch.equal(have, want), (H, W, mask, cloud, k, int((have != want).any(1).sum()))
                assert bool((nbr[~m.reshape(-1)] == -1).all())
            if cloud == "lattice" and mask in ("all", "drop30"):
                p = pts.reshape(-1, 3)[m.reshape(-1)]
                ties += int(p.shape[0] - torch.unique(p, dim=0).shape[0])
            if mask == "two":
                v = torch.nonzero(m.reshape(-1)).squeeze(1)
                assert (nbr[v][:, 2:] == -1).all() and (nbr[v][:, :2] >= 0).all() and nbr[v[0], 0] == v[0] and nbr[v[1], 0] == v[1]
    assert ties > 0                                                                  # the lattice did produce distinct pixels with identical points


@pytest.fixture(scope="module")
def host_bound(tmp_path_factory):
    """max(4 x the host's largest distance between the header's routine and eigh, 1e-12): the factor covers the device's libm."""
    from tests.test_scene_init import host_distance
    exe = str(tmp_path_factory.mktemp("init_check") / "init_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "host_check", "init_check.cpp")])
    d = host_distance(exe)
    print(f"SCENEINIT|host eigenvector distance|{d:.3e}")
    return max(4.0 * d, 1e-12), d


def _angle_measure(n, ref):
    """1 - |cos| of the angle between float32 normals, in float64 on the normalised vectors (a float32 unit vector's length is 1 only to 2^-24)."""
    a, b = n.double().reshape(-1, 3), ref.double().reshape(-1, 3)
    a, b = a / a.norm(dim=1, keepdim=True).clamp_min(1e-300), b / b.norm(dim=1, keepdim=True).clamp_min(1e-300)
    return 1.0 - (a * b).sum(1).abs()


@pytest.mark.parametrize("H,W", SIZES)
def test_normals_against_float64_eigh_on_the_same_lists(H, W, host_bound):
    bound, host = host_bound
    for mask in ("all", "drop30", "five"):
        for cloud in ("coherent", "incoherent"):
            o, d, r, m = _case(H, W, mask, cloud)
            n, nbr = si.estimate_normals(o, d, r, m, 6)
            pts = o + d * r[..., None]
            ref, lam = si.normals_from_lists_reference(pts, o, m, nbr, return_eigenvalues=True)
            lam = lam.reshape(-1, 3)
            valid = m.reshape(-1).cpu()
            ill = ((lam[:, 1] - lam[:, 0]) / lam[:, 2].clamp_min(1e-300) < 1e-6) & valid
            assert int(ill.sum()) <= 0.01 * max(1, int(valid.sum())), (H, W, mask, cloud, int(ill.sum()))
            dist = _angle_measure(n.cpu(), ref.cpu())
            keep = valid & ~ill
            worst = float(dist[keep].max()) if bool(keep.any()) else 0.0
            print(f"SCENEINIT|normals {H}x{W} {mask} {cloud}|host {host:.3e}|device {worst:.3e}|ill {int(ill.sum())}/{int(valid.sum())}")
            assert worst <= bound, (H, W, mask, cloud, worst, bound)
            assert float(n[~m].abs().sum()) == 0.0
            # every normal is a unit vector (float32) and faces the sensor: n . (o - p) >= 0 in float64
            nv = n[m].double()
            assert bool(((nv.norm(dim=1) - 1).abs() < 1e-6).all())
            v = (o[m].double() - pts[m].double())
            s = nv[:, 0] * v[:, 0] + nv[:, 1] * v[:, 1] + nv[:, 2] * v[:, 2]
            assert float(s.min()) >= 0.0, (H, W, mask, cloud, float(s.min()))


def test_exact_plane_and_the_fall_backs():
    H, W = 16, 256
    o, d = scenes.kitti_rays(H, W)
    down = d[..., 2] < -0.05
    r = np.where(down, -1.7 / np.minimum(d[..., 2], -0.05), 0.0).astype(np.float32)        # the plane z = -1.7 seen from the origin
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=DEV)
    o, d, r, m = t(o), t(d), t(r), t(down)
    n, nbr = si.estimate_normals(o, d, r, m, 6)
    assert int(m.sum()) > 1000 and bool((nbr[m][:, :6] >= 0).all())                        # every list is complete and, all returns being on the plane, lies on it
    assert float(n[m][:, 2].min()) > 0.999, float(n[m][:, 2].min())
    # two valid pixels: fewer than 3 listed points
    o2, d2, r2, m2 = _case(11, 200, "two", "coherent")
    n2 = si.estimate_normals(o2, d2, r2, m2, 6)[0]
    assert torch.equal(n2[m2], torch.tensor([[0.0, 0.0, 1.0]] * 2, device=DEV)) and float(n2[~m2].abs().sum()) == 0.0
    # six collinear points (one ray direction, six ranges): a covariance of rank 1.  n . (o - p) is exactly 0 there: +z by the first-component rule
    o3 = torch.zeros(5, 7, 3, device=DEV); d3 = torch.zeros(5, 7, 3, device=DEV); d3[..., 0] = 1.0
    r3 = torch.arange(35, device=DEV, dtype=torch.float32).reshape(5, 7) + 1.0
    m3 = torch.zeros(5, 7, dtype=torch.bool, device=DEV); m3.reshape(-1)[[0, 3, 8, 20, 21, 34]] = True
    n3, l3 = si.estimate_normals(o3, d3, r3, m3, 6)
    assert bool((l3[m3][:, :6] >= 0).all()) and torch.equal(n3[m3], torch.tensor([[0.0, 0.0, 1.0]] * 6, device=DEV))


def _actors(A, pts, m, seed):
    """Pose table seeded on the cloud: actor 0 on a return, actor 1 overlapping it with an un-normalised quaternion, actor 2 huge but absent."""
    rng = np.random.default_rng(seed)
    if A == 0:
        return None, None, None
    v = pts[m]
    c = v[int(rng.integers(0, v.shape[0]))].cpu().numpy()
    poses = np.zeros((A, 7), np.float32); sizes = np.zeros((A, 3), np.float32); present = np.ones(A, np.uint8)
    for a in range(A):
        yaw = rng.uniform(0, 2 * np.pi)
        q = np.array([np.cos(yaw / 2), 0.02 * a, -0.03 * a, np.sin(yaw / 2)])
        poses[a, :3] = c + np.array([0.8 * a, -0.4 * a, 0.1 * a]); poses[a, 3:] = q * (1.0 + 1.5 * a)        # actor 1: |q| = 2.5
        sizes[a] = (6.0, 3.0, 2.5)
    if A == 3:
        sizes[2] = (500.0, 500.0, 500.0); present[2] = 0
    t = lambda x: torch.as_tensor(x, device=DEV)
    return t(poses), t(sizes), t(present)


@pytest.mark.parametrize("A", [0, 1, 3])
def test_assignment_against_the_twin(A):
    H, W = 11, 200
    o, d, r, m = _case(H, W, "drop30", "coherent")
    pts = o + d * r[..., None]
    nrm = si.estimate_normals(o, d, r, m, 6)[0]
    poses, sizes, present = _actors(A, pts, m, seed=3)
    label, lp, ln = si.assign_to_boxes(pts, nrm, m, poses, sizes, present)
    wl, wp, wn, margin = si.assign_to_boxes_reference(pts, nrm, m, poses, sizes, present, return_margin=True)
    edge = (margin.to(DEV) < 1e-5) & m
    assert int(edge.sum()) <= 0.01 * int(m.sum())
    ok = ~edge
    assert torch.equal(label[ok], wl[ok])
    assert bool((label[~m] == -1).all()) and bool((label[m] >= 0).all())
    if A == 0:
        assert bool((label[m] == 0).all())
    else:
        assert int((label == 1).sum()) > 0 and int((label == 0).sum()) > 0
    if A == 3:
        assert int((label == 2).sum()) > 0 and int((label == 3).sum()) == 0        # the overlap went to actor 0 first; the absent actor took nothing
        both = (wl == 1) & ok                                                       # some of actor 0's points also lie in actor 1's box
        loc1 = si.assign_to_boxes_reference(pts, nrm, m, poses[1:2], sizes[1:2], present[1:2])[0]
        assert int((both & (loc1 == 1)).sum()) > 0
    tol = 2.0 * float(np.spacing(np.float32(pts[m].abs().max().item())))
    errp, errn = float((lp - wp)[ok].abs().max()), float((ln - wn)[ok].abs().max())
    print(f"SCENEINIT|assign A={A}|local point err {errp:.3e}|local normal err {errn:.3e}|tol {tol:.3e}|edge {int(edge.sum())}/{int(m.sum())}")
    assert errp <= tol and errn <= tol
    keep = ok & (label <= 0)
    assert torch.equal(lp[keep], pts[keep]) and torch.equal(ln[keep], nrm[keep])    # world values unchanged


def _voxel_case(name):
    rng = np.random.default_rng(11)
    if name == "one_point":
        p = np.array([[3.0, -2.0, 0.5]], np.float32)
    elif name == "one_voxel":
        p = (np.array([10.0, 20.0, -3.0]) + rng.uniform(0.0, 0.05, (1000, 3))).astype(np.float32)
        p[0] = (10.0, 20.0, -3.0)
    else:                                                                        # 200 k points, about 40 x 40 x 25 voxels of 0.15 m
        p = (rng.uniform(0, 1, (200_000, 3)) * np.array([6.0, 6.0, 3.75]) + np.array([-3.0, 5.0, -1.0])).astype(np.float32)
    n = rng.standard_normal(p.shape).astype(np.float32); n /= np.linalg.norm(n, axis=1, keepdims=True)
    i = rng.uniform(0, 1, p.shape[0]).astype(np.float32)
    t = lambda x: torch.as_tensor(x, device=DEV)
    return t(p), t(i), t(n)


@pytest.mark.parametrize("name", ["one_point", "one_voxel", "many"])
def test_voxel_mean_against_the_twin(name):
    p, i, n = _voxel_case(name)
    have = si.voxel_downsample(p, i, n, 0.15)
    want = si.voxel_downsample_reference(p, i, n, 0.15)
    M = want[3].shape[0]
    assert have[3].shape[0] == M and torch.equal(have[3], want[3]) and int(have[3].sum()) == p.shape[0]
    assert {"one_point": M == 1, "one_voxel": M == 1, "many": 30_000 < M <= 41 * 41 * 26}[name], M      # extent / voxel per axis, one more: the origin sits half a voxel below the minimum
    # the rows are in ascending key order: the keys of the mean points of the twin and of the operator are the same sequence
    for h, w in zip(have[:3], want[:3]):
        h64, w64 = h.double().cpu().numpy(), w.double().cpu().numpy()
        ulp = np.spacing(np.maximum(np.abs(h64), np.abs(w64)).astype(np.float32)).astype(np.float64)
        assert (np.abs(h64 - w64) <= ulp).all(), (name, float(np.abs(h64 - w64).max()))
    if name == "many":
        keys = si.voxel_keys_reference(p, 0.15)
        assert np.array_equal(np.unique(keys, return_counts=True)[1], have[3].cpu().numpy())
        assert float(have[2].norm(dim=1).min()) < 0.9                            # mean normals are not renormalised


def test_voxel_key_overflow_is_an_error_not_a_wrap():
    p = torch.tensor([[0.0, 0.0, 0.0], [0.0, float(1 << 21), 0.0]], device=DEV)
    with pytest.raises(si.SceneInitError, match="2\\^21"):
        si.voxel_downsample(p, torch.zeros(2, device=DEV), torch.zeros(2, 3, device=DEV), 1.0)
    p[1, 1] = float((1 << 21) - 1)
    assert si.voxel_downsample(p, torch.zeros(2, device=DEV), torch.zeros(2, 3, device=DEV), 1.0)[3].tolist() == [1, 1]


def _raw_calls(fill):
    """All four entry points through ctypes on pre-filled output buffers: every output tensor."""
    lib = si.load()
    H, W = 11, 200
    o, d, r, m = _case(H, W, "drop30", "coherent")
    m8 = m.view(torch.uint8)
    st = torch.cuda.current_stream(DEV).cuda_stream
    full = lambda shape, dt=torch.float32: torch.full(shape, fill if dt == torch.float32 else -77, dtype=dt, device=DEV)
    work = torch.empty(int(lib.lrt_init_normals_work_bytes(H, W)) // 8 + 1, dtype=torch.float64, device=DEV)
    nbr, nrm = full((H, W, 8), torch.int32), full((H, W, 3))
    assert lib.lrt_init_normals(0, H, W, o.data_ptr(), d.data_ptr(), r.data_ptr(), m8.data_ptr(), 6, nbr.data_ptr(), nrm.data_ptr(), work.data_ptr(), work.numel() * 8, st) == 0
    pts = (o + d * r[..., None]).contiguous()
    poses, sizes, present = _actors(3, pts, m, seed=3)
    lab, lp, ln = full((H, W), torch.int32), full((H, W, 3)), full((H, W, 3))
    assert lib.lrt_init_assign(0, H * W, pts.data_ptr(), nrm.data_ptr(), m8.data_ptr(), 3, poses.data_ptr(), sizes.data_ptr(), present.data_ptr(), lab.data_ptr(),
                               lp.data_ptr(), ln.data_ptr(), st) == 0
    N = H * W
    P, I, Nn = pts.reshape(-1, 3), r.reshape(-1).contiguous(), nrm.reshape(-1, 3)
    vwork = torch.empty(int(lib.lrt_init_voxel_work_bytes(N)) // 8 + 1, dtype=torch.float64, device=DEV)
    keys, info = full((N,), torch.int64), full((2,), torch.int32)
    assert lib.lrt_init_voxel_keys(0, N, P.data_ptr(), 0.5, keys.data_ptr(), info.data_ptr(), vwork.data_ptr(), vwork.numel() * 8, st) == 0
    sk, perm = torch.sort(keys, stable=True)
    perm = perm.to(torch.int32)
    op, oi, on, cnt = full((N, 3)), full((N,)), full((N, 3)), full((N,), torch.int32)
    assert lib.lrt_init_voxel_mean(0, N, sk.data_ptr(), perm.data_ptr(), P.data_ptr(), I.data_ptr(), Nn.data_ptr(), op.data_ptr(), oi.data_ptr(), on.data_ptr(),
                                   cnt.data_ptr(), info.data_ptr(), vwork.data_ptr(), vwork.numel() * 8, st) == 0
    return [nbr, nrm, lab, lp, ln, keys, info, op, oi, on, cnt]


def test_outputs_are_written_whole_and_repeat_bit_for_bit():
    runs = [_raw_calls(fill) for fill in (float("nan"), 0.0, float("nan"))]
    torch.cuda.synchronize()
    M = int(runs[0][6][0])
    assert 0 < M < 11 * 200 and int(runs[0][6][1]) == 0
    for other in runs[1:]:
        for x, y in zip(runs[0], other):
            assert not bool(torch.isnan(x.float()).any()) and torch.equal(x, y)
    nbr, lab, cnt, op = runs[0][0], runs[0][2], runs[0][10], runs[0][7]
    assert int((nbr == -77).sum()) == 0 and int((lab == -77).sum()) == 0 and int((cnt == -77).sum()) == 0
    assert int(cnt[M:].abs().sum()) == 0 and float(op[M:].abs().sum()) == 0.0 and int(cnt[:M].min()) >= 1      # zeros from row M on


def test_the_calls_are_stream_ordered_behind_a_busy_kernel_without_a_host_wait():
    from tests.test_stream_order_gpu import _busy
    o, d, r, m = _case(66, 1030, "drop30", "coherent")
    pts = o + d * r[..., None]
    poses, sizes, present = _actors(3, pts, m, seed=3)

    def step(depth):
        n, nbr = si.estimate_normals(o, d, depth, m, 6)
        return (n, nbr) + si.assign_to_boxes(o + d * depth[..., None], n, m, poses, sizes, present)
    want = step(r * 1.01)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _busy(0.01); torch.cuda.synchronize()
        _busy(0.4)
        marker = torch.cuda.Event(); marker.record()
        t0 = time.perf_counter()
        got = step(r * 1.01)                                                      # its input is produced on this stream, behind the busy kernel
        host_s = time.perf_counter() - t0
        still_busy = not marker.query()
    assert still_busy, f"the GPU finished the dummy work before the calls were enqueued ({host_s * 1e3:.1f} ms of host time)"
    assert host_s < 0.1, f"enqueueing took {host_s * 1e3:.1f} ms of host time while the GPU was busy: something waited"
    side.synchronize()
    for x, y in zip(want, got):
        assert torch.equal(x, y)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------

def test_training_from_frames_end_to_end(tmp_path):
    """A 16 x 256 sequence with two actors and no init/ directory: `train --init-from-frames --iters 30 --deterministic`, twice."""
    import bench_scene_init
    from tests.test_train_entry_gpu import _load
    data = str(tmp_path / "seq")
    bench_scene_init.write_analytic_sequence(data, 16, 256, n_frames=4, n_actors=2, noise=0.01)
    assert not os.path.exists(os.path.join(data, "init"))
    common = ["--data", data, "--init-from-frames", "--iters", "30", "--log-every", "1", "--save-every", "30", "--deterministic"]
    run = lambda out: subprocess.run([sys.executable, "-m", "lidar_rt_amd.train", "--out", out] + common, cwd=REPO, capture_output=True, text=True, timeout=600)
    a = run(str(tmp_path / "a"))
    assert a.returncode == 0, a.stdout[-2000:] + a.stderr[-3000:]
    rows = [json.loads(l) for l in a.stdout.splitlines() if l.startswith("{")]
    rep = [r for r in rows if "init_from_frames" in r][0]["init_from_frames"]["clouds"]
    log = [r for r in rows if "iteration" in r]
    print(f"SCENEINIT|train --init-from-frames|loss@1 {log[0]['loss']:.5f}|loss@30 {log[-1]['loss']:.5f}|clouds {json.dumps(rep)}")
    assert log[0]["iteration"] == 1 and log[-1]["iteration"] == 30 and np.isfinite(log[-1]["loss"])
    assert log[-1]["loss"] < log[0]["loss"], (log[0]["loss"], log[-1]["loss"])
    assert set(rep) == {"background", "actor_00", "actor_01"}
    assert rep["actor_00"]["real"] > 0 and rep["actor_01"]["real"] > 0 and rep["background"]["points"] > 0
    b = run(str(tmp_path / "b"))
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-3000:]
    pa, pb = _load(tmp_path / "a" / "chkpnt30.pth")[0], _load(tmp_path / "b" / "chkpnt30.pth")[0]
    assert len(pa) == len(pb) == 3
    for ga, gb in zip(pa, pb):
        for i in (1, 2, 3, 4, 5, 6):
            assert torch.equal(ga[i].detach().cpu(), gb[i].detach().cpu()), i
