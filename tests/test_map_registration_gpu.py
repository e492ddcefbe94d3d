"""Scan-to-map registration on the GPU: `linearize_to_grid` and `align_to_grid` of `liblrt_mapreg.so` against the float64 twin on every case of
tests/map_registration_cases.py, equal bits for equal inputs, a batch against its frames one by one, frozen poses, a chain of calls without a
host read, the inverse pose, and `track_and_fuse` on the device against the twin."""
import math

import numpy as np
import pytest
import torch

from lidar_rt_amd import map_registration as mr, registration as rg
from tests import map_registration_cases as mc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U = 2.0 ** -53


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def same(x, y):
    return torch.equal(bits(x), bits(y))


def run(key, init=None, frames=None, **kw):
    c = mc.case(key)
    grid, src = mc.to_device(c, DEV)
    X0 = (c.X_start if init is None else init).to(DEV)
    if frames is not None:
        src, X0 = tuple(t[frames] for t in src), X0[frames]
    return mr.align_to_grid(grid, src, X0, c.iters, c.huber, min_pairs=c.min_pairs, **kw)


@pytest.mark.parametrize("key", mc.LINEARIZE_KEYS)
def test_linearize_is_the_twin(key):
    """cell equal on every pixel -- seeded inputs with a margin, the same float64 rule of + - * / and floor -- sums[29] the count of cell >= 0, and
    every other sum within N 2^-53 sum |term| of the twin's; at the start pose and at the true pose."""
    c = mc.case(key)
    grid, src = mc.to_device(c, DEV)
    for name, X in mc.linearize_points(c):
        sums, cell = mr.linearize_to_grid(grid, src, X.to(DEV), c.huber)
        t_sums, t_cell, ab, _ = mc.linearize_reference(key, name)
        assert sums.shape == (c.F, mr.NSUM) and cell.shape == (c.F, c.H, c.W) and cell.dtype == torch.int32
        assert torch.equal(cell.cpu(), t_cell), (key, name, int((cell.cpu() != t_cell).sum()))
        assert torch.equal(sums[:, 29].cpu(), (cell.cpu() >= 0).reshape(c.F, -1).sum(1).double())
        n = torch.tensor([max(v, 1) for v in c.n_valid], dtype=torch.float64)[:, None]
        excess = ((sums.cpu() - t_sums).abs() - n * U * ab).max()
        print(key, name, "terms", sums[:, 29].tolist(), "largest |difference| - bound:", float(excess))
        assert float(excess) <= 0.0, (key, name)
    only_sums, none = mr.linearize_to_grid(grid, src, X.to(DEV), c.huber, want_cell=False)
    assert none is None and same(only_sums, sums)


def test_the_edge_cases_on_the_device():
    """The last voxel centre (cell n - 2), an axis of 2 voxels and of 1 voxel, unobserved corners and free space: what the twin says, pixel by pixel
    (test_linearize_is_the_twin) -- and here that each of them does occur in what the device returned."""
    c = mc.case("last_centre")
    grid, src = mc.to_device(c, DEV)
    _, cell = mr.linearize_to_grid(grid, src, c.X_start.to(DEV), c.huber)
    X, Y, Z = c.grid.dims
    assert int(cell[0, 0, 7]) == ((X - 2) * Y + (Y - 2)) * Z + (Z - 2) and int(cell[0, 0, 1]) == ((X - 2) * Y + 1) * Z + 1
    c = mc.case("thin1")
    grid, src = mc.to_device(c, DEV)
    sums, cell = mr.linearize_to_grid(grid, src, c.X_start.to(DEV), c.huber)
    assert not sums.any() and bool((cell == -1).all())
    c = mc.case("holes")
    grid, src = mc.to_device(c, DEV)
    _, cell = mr.linearize_to_grid(grid, src, c.X_start.to(DEV), c.huber)
    assert 100 <= int((cell >= 0).sum()) < c.n_valid[0] - 30


@pytest.mark.parametrize("key", mc.ALIGN_KEYS)
def test_align_is_the_twin(key):
    """|X_hip - X_twin| <= 64 N 2^-53 cond(A) max(1, |t|) per entry (N the valid source pixels, cond(A) the twin's at its last iteration, recorded
    with the case), equal status and equal term counts in every iteration, a symmetric hessian within 1e-9 of the twin's, and G X = 1.

    The bound on G X - 1, from the three-term sums.  G's rotation is X's transposed, bit for bit, so the rotation block of G X is R^T R: each of the
    K steps X <- X Exp(delta) rounds three-term sums of products of entries <= 1 (4 u per entry), Exp itself is orthonormal to a few u, and the
    product formed here on the host adds 3 u: 16 u (K + 1).  The translation column is -(R^T t) + R^T t with both rounded as three-term sums:
    2 (3 u) sum_j |R_ji t_j| <= 6 u sqrt(3) |t|, and the last addition 2 u more: 8 u sqrt(3) max(1, |t|)."""
    c = mc.case(key)
    got, want = run(key), mc.reference(key)
    assert got.X.shape == got.G.shape == (c.F, 3, 4) and got.log.shape == (c.F, c.iters, mr.NLOG) and got.hessian.shape == (c.F, 6, 6)
    assert got.status.cpu().tolist() == want.status.tolist()
    assert torch.equal(got.log[:, :, 0].cpu(), want.log[:, :, 0]) and torch.equal(got.log[:, :, 5].cpu(), want.log[:, :, 5]) and not got.log[:, :, 6:].any()
    for f in range(c.F):
        diff = float((got.X[f].cpu() - want.X[f]).abs().max())
        X, G = got.X[f].cpu().numpy(), got.G[f].cpu().numpy()
        t = max(1.0, float(np.linalg.norm(X[:, 3])))
        GX = G[:, :3] @ X + np.concatenate([np.zeros((3, 3)), G[:, 3:]], 1) - np.eye(4)[:3]
        rot, tr = float(np.abs(GX[:, :3]).max()), float(np.abs(GX[:, 3]).max())
        print(key, f, "G X - 1: rotation", rot, "bound", 16 * U * (c.iters + 1), "translation", tr, "bound", 8 * U * math.sqrt(3.0) * t)
        assert rot <= 16 * U * (c.iters + 1) and tr <= 8 * U * math.sqrt(3.0) * t
        assert np.array_equal(G[:, :3], X[:, :3].T)
        if int(want.status[f]) in (rg.FEW, rg.PIVOT):
            assert diff == 0.0 and same(got.X[f].cpu(), c.X_start[f])            # X_init, bit for bit
            continue
        bound = 64.0 * c.n_valid[f] * U * mc.RECORDED[key][0] * max(1.0, float(want.X[f][:, 3].norm()))
        print(key, f, "largest |X_hip - X_twin|:", diff, "bound:", bound)
        assert diff <= bound, (key, f, diff, bound)
        h = want.hessian[f]
        assert float((got.hessian[f].cpu() - h).abs().max()) <= 1e-9 * float(h.abs().max())
        assert torch.equal(got.hessian[f], got.hessian[f].T)


def test_two_calls_give_equal_bits_and_a_batch_is_its_frames_run_singly():
    a, b = run("batch3"), run("batch3")
    for x, y in zip(a, b):
        assert same(x, y)
    for f in range(3):
        one = run("batch3", frames=slice(f, f + 1))
        for x, y in zip(a, one):
            assert same(x[f:f + 1], y), f
    ws = torch.empty(mr.work_bytes(3, 16, 128) + 512, dtype=torch.uint8, device=DEV)
    for x, y in zip(a, run("batch3", workspace=ws)):
        assert same(x, y)


def test_a_pose_handed_on_without_a_host_read_is_the_single_call():
    """Four iterations, then four more from X_out as it lies on the device: the poses of one call of eight, as long as no frame stopped in the
    first four (a status freezes X; the second call would start afresh)."""
    key = "room3_16x128_waymo_table"
    c = mc.case(key)
    grid, src = mc.to_device(c, DEV)
    kw = dict(huber=c.huber, min_pairs=c.min_pairs)
    whole = mr.align_to_grid(grid, src, c.X_start.to(DEV), 8, **kw)
    first = mr.align_to_grid(grid, src, c.X_start.to(DEV), 4, **kw)
    second = mr.align_to_grid(grid, src, first.X, 4, **kw)                  # no host read in between
    assert first.status.cpu().tolist() == [rg.OK]
    assert same(second.X, whole.X) and same(second.G, whole.G) and same(second.hessian, whole.hessian)
    assert same(torch.cat([first.log, second.log], 1), whole.log)


def test_track_and_fuse_on_the_device_is_the_twin():
    """Four frames of 16 x 128 on a grid of voxel 0.5 m, trunc 1.5 m (the twin's margin there is 7e-7; at 0.4 m it is 2e-10), from the true steps.  Every pose within the align bound of the twin's,
    accumulated: frame k within k * 64 N 2^-53 cond(A_k) max(1, |t|), cond(A_k) the twin's.  The weights equal the twin's exactly if the twin's
    margin (projection, sampling) is at least 1e-9 -- the poses differ by far less; otherwise at most 1e-4 of the voxels may differ."""
    frames, images, truth, kw = mc.trajectory(4, 16, 128)
    steps = {i: np.linalg.inv(truth[i - 1]) @ truth[i] for i in (1, 2, 3)}
    twin_grid = mc.tracking_grid(frames, truth, 0.5, 1.5)
    want, wrep = mr.track_and_fuse(twin_grid, frames, images, steps=steps, **kw)
    grid = mc.tracking_grid(frames, truth, 0.5, 1.5, device=DEV)
    d_frames = {i: tuple(t.to(DEV) for t in g) for i, g in frames.items()}
    d_images = {i: tuple(t.to(DEV) for t in g) for i, g in images.items()}
    got, rep = mr.track_and_fuse(grid, d_frames, d_images, steps=steps, **kw)
    assert [(r["id"], r["status"], r["terms"]) for r in rep["frames"]] == [(r["id"], r["status"], r["terms"]) for r in wrep["frames"]] and rep["failed"] == []
    acc = 0.0
    for k, i in enumerate(sorted(frames)):
        if k:
            X = mr.grid_pose(twin_grid, want[i])
            acc += 64.0 * 16 * 128 * U * wrep["frames"][k]["cond"] * max(1.0, float(np.linalg.norm(X[:3, 3])))
        diff = float(np.abs(got[i] - want[i]).max())
        print(i, "largest |pose - twin|:", diff, "bound:", acc)
        assert diff <= acc, (i, diff, acc)
    differ = int((grid.weight.cpu() != twin_grid.weight).sum())
    print("weights that differ:", differ, "of", twin_grid.weight.numel(), "twin margin", wrep["margin"])
    assert int(twin_grid.weight.max()) == 4
    if wrep["margin"] >= mc.MARGIN:
        assert differ == 0
    else:
        assert differ <= 1e-4 * twin_grid.weight.numel(), "the share of voxels whose weight differs from the twin's"
