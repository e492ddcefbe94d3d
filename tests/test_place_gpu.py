"""The place matcher on the GPU: `describe` and `match` of `liblrt_place.so` EQUAL to their numpy twins, int for int, on the cases of
tests/place_cases.py; the launch counts, equal bits for equal inputs, a stream of the caller's, and `pose_graph.close_loops` on the device accepting
the twin's edges within the bound `align` already has against its twin."""
import math

import numpy as np
import pytest
import torch

from lidar_rt_amd import place, pose_graph as pg
from tests import place_cases as pc
from tests.test_registration_gpu import U                                   # 2^-53: the unit of the bound of align against its twin

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ALL_GRIDS = pc.GRIDS + (pc.ODD_GRID,)


def on_device(F, H, W):
    p, m = pc.frames(F, H, W)
    return p.to(DEV), m.to(DEV)


@pytest.mark.parametrize("shape", pc.SHAPES)
@pytest.mark.parametrize("grid", ALL_GRIDS)
def test_describe_and_match_are_the_twins(shape, grid):
    (F, H, W), (NR, NS) = shape, grid
    p, m = on_device(F, H, W)
    if NS > W:                                                                # 60 and 128 sectors over 37 or 40 columns
        with pytest.raises(place.PlaceError, match=f"{NS} sectors over {W} columns"):
            place.describe(p, m, pc.Z_LO, NR, NS, **pc.RULE)
        return
    desc, sums = place.describe(p, m, pc.Z_LO, NR, NS, **pc.RULE)
    w_desc, w_sums = pc.described(F, H, W, NR, NS)
    assert desc.dtype == torch.uint8 and desc.shape == (F, NS, place.padded(NR)) and sums.dtype == torch.int32 and sums.shape == (F,)
    assert torch.equal(desc.cpu(), w_desc), (shape, grid, int((desc.cpu() != w_desc).sum()))
    assert torch.equal(sums.cpu(), w_sums)
    if F > 2:
        assert not desc[F // 2].any() and torch.equal(desc[F - 1], desc[0]) and int(sums[0]) > 0       # the all-invalid frame in the middle, the equal pair
    for gap in (0, 1, F):
        bd, bs = place.match(desc, gap)
        w_bd, w_bs = pc.matched(F, H, W, NR, NS, gap)
        assert bd.dtype == torch.int32 and bd.shape == (F, F)
        assert torch.equal(bd.cpu(), w_bd), (shape, grid, gap, int((bd.cpu() != w_bd).sum()))
        assert torch.equal(bs.cpu(), w_bs), (shape, grid, gap, int((bs.cpu() != w_bs).sum()))
        if gap == F:
            assert bool((bd == -1).all()) and bool((bs == -1).all())
    one, s1 = place.describe(p[0], m[0], pc.Z_LO, NR, NS, **pc.RULE)                                   # without a frame axis
    assert torch.equal(one, desc[0]) and int(s1) == int(sums[0])


def test_more_candidates_than_a_tile_and_the_tie_on_j():
    """33 frames: three tiles of 16 candidates, the last with one; rows whose triangle ends inside a tile and inside a wave's four candidates."""
    desc9, sums9 = pc.described(9, 8, 40, *pc.ODD_GRID)
    idx = torch.tensor([k % 9 for k in range(33)])
    desc, sums = desc9[idx].contiguous(), sums9[idx]
    for gap in (0, 3, 20):
        bd, bs = place.match(desc.to(DEV), gap)
        w_bd, w_bs = place.match_reference(desc, gap)
        assert torch.equal(bd.cpu(), w_bd) and torch.equal(bs.cpu(), w_bs), gap
    bd, bs = place.match(desc.to(DEV), 3)
    got = place.candidates(bd, bs, sums.to(DEV), top=2, max_score=0.0)
    assert got == place.candidates(*place.match_reference(desc, 3), sums, top=2, max_score=0.0)
    assert [(i, j) for i, j, _, _ in got if i == 27] == [(27, 0), (27, 8)]                             # frames 0, 8, 9, 17, 18 equal frame 27: the lower j first
    tie = pc.described(9, 8, 40, 4, 8)[0].clone()
    tie[:, 4:] = tie[:, :4]                                                                            # period 4 of 8 sectors: two shifts tie, the lower wins
    bd, bs = place.match(tie.to(DEV), 0)
    w_bd, w_bs = place.match_reference(tie, 0)
    assert torch.equal(bd.cpu(), w_bd) and torch.equal(bs.cpu(), w_bs) and int(bs.max()) < 4


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = {e.key: e.count for e in prof.key_averages() if e.device_time_total > 0}
    return {k: v for k, v in ev.items() if "memcpy" not in k.lower() and "memset" not in k.lower()}


def test_every_operator_launches_one_kernel_whatever_the_images_hold():
    counts = {}
    p, m = on_device(5, 16, 128)
    for key, mask in (("seeded", m), ("empty", torch.zeros_like(m)), ("full", torch.ones_like(m))):
        desc, _ = place.describe(p, mask, pc.Z_LO, 20, 60, **pc.RULE)
        for name, fn in (("describe", lambda: place.describe(p, mask, pc.Z_LO, 20, 60, **pc.RULE)), ("match", lambda: place.match(desc, 1)),
                         ("match_all_outside", lambda: place.match(desc, 5))):
            ev = launches(fn)
            assert all("k_place_" in k for k in ev), (key, name, ev)
            counts.setdefault(name, {})[key] = sum(ev.values())
    print(counts)
    assert counts == {n: {"seeded": 1, "empty": 1, "full": 1} for n in ("describe", "match", "match_all_outside")}


def test_a_second_call_returns_the_same_bits():
    p, m = on_device(5, 16, 128)
    first = place.describe(p, m, pc.Z_LO, 32, 128, **pc.RULE)
    held = [torch.full((1 << 20,), 0xAB, dtype=torch.uint8, device=DEV) for _ in range(2)]              # dirty memory for the next outputs to land in
    del held
    again = place.describe(p, m, pc.Z_LO, 32, 128, **pc.RULE)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    a, b = place.match(first[0], 1), place.match(again[0], 1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_a_stream_of_the_callers_orders_against_the_torch_ops_around_it():
    p, m = on_device(5, 16, 128)
    w_desc, w_sums = pc.described(5, 16, 128, 20, 60)
    w_bd, w_bs = pc.matched(5, 16, 128, 20, 60, 1)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        big = torch.randn(4096, 4096, device=DEV)
        for _ in range(4):
            big = big @ big * 1e-3                                                                      # work in front of the call, on the same stream
        q = p + 0.0 * big[0, 0].nan_to_num(0.0, 0.0, 0.0)                                               # the input is made by a torch op of that stream
        desc, sums = place.describe(q, m, pc.Z_LO, 20, 60, **pc.RULE)
        bd, bs = place.match(desc, 1)
        after = (desc.long().sum((1, 2)), bd.clone(), bs + 0)                                          # torch ops that follow on the stream
    side.synchronize()
    assert torch.equal(desc.cpu(), w_desc) and torch.equal(sums.cpu(), w_sums) and torch.equal(after[0].cpu(), w_sums.long())
    assert torch.equal(after[1].cpu(), w_bd) and torch.equal(after[2].cpu(), w_bs)


def test_close_loops_on_the_device_accepts_the_twins_edges_and_optimize_ends_within_the_bound():
    want = pc.tour_reference()
    fr, truth = pc.tour_on(DEV)
    got = pc.run_tour(fr, truth)
    key = lambda rep: [(r["source"], r["target"], r["shift"], r["status"]) for r in rep["accepted"]]
    assert key(got.loop_report) == key(want.loop_report) == [(8, 0, 0, 3)]
    assert got.loop_report["rejected"] == [] and got.loop_report["accepted"][0]["score"] == want.loop_report["accepted"][0]["score"]
    # the bound of test_registration_gpu.test_align_is_the_twin, per entry of X: 64 N 2^-53 cond(A) max(1, |t|), N the valid source pixels and cond(A)
    # the twin's hessian's -- for the loop edge and for every odometry step
    n_valid = {i: int(g[2].sum()) for i, g in pc.tour()[0].items()}
    edge_bound = lambda src, hess, X: 64.0 * n_valid[src] * U * float(np.linalg.cond(hess)) * max(1.0, float(np.linalg.norm(X[:, 3])))
    b_loop = edge_bound(8, want.loops[0]["info"], want.loops[0]["Z"])
    d_loop = float(np.abs(got.loops[0]["Z"] - want.loops[0]["Z"]).max())
    print("largest |X_hip - X_twin| of the loop edge:", d_loop, "bound:", b_loop)
    assert d_loop <= b_loop
    total = b_loop
    for g, w in zip(got.steps, want.steps):
        b = edge_bound(w["source"], w["hessian"], w["X"])
        assert (g["source"], g["target"], g["status"]) == (w["source"], w["target"], w["status"]) and float(np.abs(g["X"] - w["X"]).max()) <= b
        total += b
    # optimize: the minimiser moves with the measurements by H^-1 sum J^T info eps, so |delta| <= |H^-1| sum |J| |info| |eps| <= cond(H) sum |J| |eps|
    # (every edge's info is a summand of a diagonal block of H, so |info| <= |H|).  |eps| <= sqrt(12) b for the 12 entries of an X within b each;
    # |J| <= |Jr^-1| |Ad| <= 2 (1 + |t|) for residuals of a few millimetres and poses within |t| of each other.  A pose moved by the twist delta
    # moves by at most (1 + |t|) |delta| per entry.  The informations differ as the X do; that is of second order in the bounds.
    edges = pg.odometry_edges(want.steps) + want.loops
    cond_h = float(np.linalg.cond(pg.normal_matrix(want.solved, edges)))
    reach = 1.0 + max(float(np.linalg.norm(T[:3, 3] - want.solved[0][:3, 3])) for T in want.solved.values())
    bound = cond_h * 2.0 * reach * math.sqrt(12.0) * total * reach
    diff = max(float(np.abs(got.solved[i] - want.solved[i]).max()) for i in want.solved)
    print("largest |pose_hip - pose_twin| after optimize:", diff, "bound:", bound, "cond(H):", cond_h)
    assert diff <= bound and got.solve_report["converged"]
