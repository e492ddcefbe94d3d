"""Scan registration on the GPU: `linearize` and `align` of `liblrt_reg.so` against the float64 twin on every case of tests/registration_cases.py,
equal bits for equal inputs, pairs in one call against pairs one by one, frozen poses, a chain of calls without a host read, the odometry of
three frames, and the launch count."""
import numpy as np
import pytest
import torch

from lidar_rt_amd import registration as rg
from tests import registration_cases as rc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U = 2.0 ** -53


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def same(x, y):
    return torch.equal(bits(x), bits(y))


def on_device(key):
    c = rc.case(key)
    src, tgt = rc.to_device(c, DEV)
    return c, src, tgt


def run(key, init=None, schedule=None, pairs=None, **kw):
    c, src, tgt = on_device(key)
    if pairs is not None:
        src, tgt = tuple(t[pairs] for t in src), tuple(t[pairs] for t in tgt)
    return rg.align(src, tgt, init, c.schedule if schedule is None else schedule, min_pairs=c.min_pairs, **c.kw, **kw)


@pytest.mark.parametrize("key", rc.KEYS)
def test_linearize_is_the_twin(key):
    """assoc equal on every pixel -- seeded inputs, the same float64 rule -- and every sum within N 2^-53 sum |term| of the twin's."""
    c, src, tgt = on_device(key)
    windows = [(int(c.schedule[0][0]), int(c.schedule[0][1]), float(c.schedule[0][2])), (int(c.schedule[-1][0]), int(c.schedule[-1][1]), float(c.schedule[-1][2]))]
    if key == "wide":
        windows.append((4, 16, 3.0))
    for name, X in rc.linearize_points(c):
        for rh, rw, md in windows:
            sums, assoc = rg.linearize(src, tgt, X.to(DEV), rh, rw, md, **c.kw)
            t_sums, t_assoc, ab = rg.linearize_reference(c.src, c.tgt, X, rh, rw, md, return_abs=True, **c.kw)
            assert sums.shape == (c.F, rg.NSUM) and assoc.shape == (c.F, c.H, c.W) and assoc.dtype == torch.int32
            assert torch.equal(assoc.cpu(), t_assoc), (key, name, rh, rw, int((assoc.cpu() != t_assoc).sum()))
            n = torch.tensor([max(v, 1) for v in c.n_valid], dtype=torch.float64)[:, None]
            excess = ((sums.cpu() - t_sums).abs() - n * U * ab).max()
            print(key, name, rh, rw, "largest |difference| - bound:", float(excess))
            assert float(excess) <= 0.0, (key, name, rh, rw)
            assert torch.equal(sums[:, 29].cpu(), (t_assoc >= 0).reshape(c.F, -1).sum(1).double())
    only_sums, none = rg.linearize(src, tgt, X.to(DEV), rh, rw, md, want_assoc=False, **c.kw)
    assert none is None and same(only_sums, sums)


@pytest.mark.parametrize("key", rc.KEYS)
def test_align_is_the_twin(key):
    """|X_hip - X_twin| <= 64 N 2^-53 cond(A) max(1, |t|) per entry (N the valid source pixels, cond(A) the twin's at its last iteration, recorded
    with the case), equal status and equal partner counts in every iteration."""
    c = rc.case(key)
    got, want = run(key), rc.reference(key)
    assert got.X.shape == (c.F, 3, 4) and got.log.shape == (c.F, len(c.schedule), rg.NLOG) and got.hessian.shape == (c.F, 6, 6)
    assert got.status.cpu().tolist() == want.status.tolist()
    assert torch.equal(got.log[:, :, 0].cpu(), want.log[:, :, 0]) and torch.equal(got.log[:, :, 5].cpu(), want.log[:, :, 5]) and not got.log[:, :, 6:].any()
    for f in range(c.F):
        diff = float((got.X[f].cpu() - want.X[f]).abs().max())
        if int(want.status[f]) in (rg.FEW, rg.PIVOT):
            assert diff == 0.0
            continue
        bound = 64.0 * c.n_valid[f] * U * rc.RECORDED[key][2] * max(1.0, float(want.X[f][:, 3].norm()))
        print(key, f, "largest |X_hip - X_twin|:", diff, "bound:", bound)
        assert diff <= bound, (key, f, diff, bound)
        h = want.hessian[f]
        assert float((got.hessian[f].cpu() - h).abs().max()) <= 1e-9 * float(h.abs().max())
        assert torch.equal(got.hessian[f], got.hessian[f].T)


def test_two_calls_give_the_same_bits_and_a_batch_is_its_pairs():
    a, b = run("batch3"), run("batch3")
    assert same(a.X, b.X) and same(a.log, b.log) and same(a.hessian, b.hessian) and torch.equal(a.status, b.status)
    for f in range(3):
        one = run("batch3", pairs=slice(f, f + 1))
        assert same(one.X[0], a.X[f]) and same(one.log[0], a.log[f]) and same(one.hessian[0], a.hessian[f]) and int(one.status[0]) == int(a.status[f]), f
    c, src, tgt = on_device("batch3")
    flat = rg.align(tuple(t[0] for t in src), tuple(t[0] for t in tgt), None, c.schedule, min_pairs=c.min_pairs, **c.kw)      # without a pair axis
    assert flat.X.shape == (3, 4) and same(flat.X, a.X[0]) and flat.status.shape == ()
    ws = torch.full((rg.work_bytes(3, c.H, c.W) + 512,), 0xAB, dtype=torch.uint8, device=DEV)                               # a dirty workspace of the caller
    d = run("batch3", workspace=ws)
    assert same(d.X, a.X) and same(d.log, a.log)


def test_a_failed_pair_returns_the_bits_of_its_start():
    c, src, tgt = on_device("batch3")
    init = torch.from_numpy(np.stack([rc.exp4(rc.twist(30 + f, 0.2, 1.0))[:3] for f in range(3)])).to(DEV)
    r = rg.align(src, tgt, init, c.schedule, min_pairs=c.min_pairs, **c.kw)
    assert r.status.cpu().tolist()[1:] == [rg.FEW, rg.FEW] and same(r.X[1], init[1]) and same(r.X[2], init[2]) and not same(r.X[0], init[0])
    tn = tgt[1].clone()
    tn[2] = float("nan")                                                                  # a system that is not a number: status 2
    r2 = rg.align(src, (tgt[0], tn, tgt[2]), init, c.schedule[:3], min_pairs=c.min_pairs, **c.kw)
    assert r2.status.cpu().tolist() == [rg.OK, rg.FEW, rg.PIVOT] and same(r2.X[2], init[2]) and same(r2.X[1], init[1])
    assert r2.log[2, :, 5].cpu().tolist() == [2.0, 2.0, 2.0] and not r2.log[2, :, 3:5].any()


def test_a_converged_pair_stops_where_its_log_says():
    full = run("room_b")
    st = full.log[0, :, 5].cpu()
    first = int((st == 3).nonzero()[0])
    assert 0 < first < len(st) - 1 and bool((st[first:] == 3).all()) and bool((st[:first] == 0).all())
    c = rc.case("room_b")
    for k in (first, first + 1):                                                          # the schedule cut before / after the converging iteration
        cut = run("room_b", schedule=c.schedule[:k])
        assert same(cut.X, full.X) and int(cut.status[0]) == (rg.OK if k == first else rg.CONVERGED), k
    before = run("room_b", schedule=c.schedule[:first - 1])
    assert not same(before.X, full.X)
    assert not full.log[0, first + 1:, 3:5].any() and float(full.log[0, first, 3]) < 1e-5


def test_a_chain_on_the_device_is_the_chain_through_the_host():
    c, src, tgt = on_device("room_a")
    s1, s2 = c.schedule[:2], c.schedule[2:]
    with torch.cuda.stream(torch.cuda.Stream(DEV)):
        torch.cuda.set_sync_debug_mode("error")                                          # a host wait between the two calls would raise
        try:
            a = rg.align(src, tgt, None, s1, min_pairs=c.min_pairs, **c.kw)
            b = rg.align(src, tgt, a.X, s2, min_pairs=c.min_pairs, **c.kw)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.current_stream(DEV).synchronize()
    a_host = rg.align(src, tgt, None, s1, min_pairs=c.min_pairs, **c.kw).X.cpu()
    b_host = rg.align(src, tgt, a_host.clone().to(DEV), s2, min_pairs=c.min_pairs, **c.kw)
    assert same(b.X, b_host.X) and same(b.log, b_host.log)
    whole = run("room_a")
    assert same(b.X, whole.X)                                                             # and both are the one call with the whole schedule


def test_odometry_on_the_device_is_the_twins_trajectory():
    """Each pair within the bound of align; the third pose is two compositions, so its bound is the sum of the two pairs' bounds times the norms
    of the factors (<= 2 here: rotations, and translations below 1 m)."""
    frames, truth, kw = rc.odometry_frames(3)
    want, w_rep = rg.odometry(frames, **kw)
    got, g_rep = rg.odometry({i: tuple(t.to(DEV) for t in g) for i, g in frames.items()}, **kw)
    assert g_rep["pairs"] == w_rep["pairs"] and g_rep["failed"] == []
    n = 16 * 128
    pair = 64.0 * n * U * 40.0                                                           # cond(A) of these pairs is about 30 (RECORDED of the room cases)
    assert np.array_equal(got[10], np.eye(4))
    for i, k in ((12, 1), (14, 2)):
        diff = float(np.abs(got[i] - want[i]).max())
        print(i, "largest |pose_hip - pose_twin|:", diff, "bound:", 2.0 * k * pair)
        assert diff <= 2.0 * k * pair, (i, diff)
    geo = rg.frame_geometry(torch.linalg.norm(frames[12][0], dim=-1).to(DEV), frames[12][2].to(DEV), kw["inclination"], 16, 128)
    assert geo[0].device.type == "cuda" and float((geo[0].cpu() - frames[12][0]).abs().max()) <= 1e-5 and torch.equal(geo[2].cpu(), frames[12][2])


def test_align_is_two_launches_per_iteration():
    from torch.profiler import ProfilerActivity, profile
    c, src, tgt = on_device("batch3")
    run("batch3")
    init = torch.eye(4, dtype=torch.float64, device=DEV)[:3].expand(3, 3, 4).contiguous()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        r = rg.align(src, tgt, init, c.schedule, min_pairs=c.min_pairs, **c.kw)
        torch.cuda.synchronize()
    ev = {e.key: e.count for e in prof.key_averages() if e.device_time_total > 0}
    K = len(c.schedule)
    ours = {k: v for k, v in ev.items() if "k_reg_" in k}
    assert sum(v for k, v in ours.items() if "k_reg_linearize" in k) == K and sum(v for k, v in ours.items() if "k_reg_solve" in k) == K, ev
    kernels = sum(v for k, v in ev.items() if "memcpy" not in k.lower() and "memset" not in k.lower())
    assert kernels == 2 * K, ev                                                           # all three pairs at once, and nothing else is launched
    assert r.X.is_cuda
