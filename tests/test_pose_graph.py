"""The pose graph without a GPU: the Jacobians against central differences, the solver on a seeded closed trajectory, the gates of `close_loops`,
the room tour end to end on the twins, and `ingest --odometry --loop-closure` on the CPU path."""
import json
import math
import os

import numpy as np
import pytest
import torch

from lidar_rt_amd import ingest, place, pose_graph as pg, registration as rg, sequence
from tests import place_cases as pc, registration_cases as rc


def bump(T, d):
    return pg._compose(T, *rg.exp_reference(d))


# ---- 1. the Jacobians ---------------------------------------------------------------------------------------------------------------------------------------------

def test_both_jacobians_against_central_differences():
    """Central differences with h = 1e-6 in float64: the truncation is h^2 |r'''| / 6, about 1e-12 times the third derivative (of order 10 with
    translations of a few metres), and the rounding 2^-53 |r| / h, about 1e-9: the bound is 1e-7."""
    rng = np.random.default_rng(0)
    h, worst = 1e-6, 0.0
    for trial in range(12):
        xs = [np.concatenate([rng.normal(size=3) * 3.0, rng.normal(size=3)]) for _ in range(2)]
        for x, angle in zip(xs, (2.0, 2.0 * rng.uniform())):                  # rotations up to 2 rad, one of the two poses AT 2 rad
            x[3:] *= angle / np.linalg.norm(x[3:])
        Ta, Tb = pc.exp34(xs[0]), pc.exp34(xs[1])
        Z = bump(pg.relative(Ta, Tb), np.concatenate([rng.normal(size=3) * 0.5, rng.normal(size=3) * (0.4 if trial % 3 else 1e-3)]))
        r, Ja, Jb = pg.jacobians(Z, Ta, Tb)
        assert np.array_equal(r, pg.residual(Z, Ta, Tb))
        Na, Nb = np.zeros((6, 6)), np.zeros((6, 6))
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            Na[:, k] = (pg.residual(Z, bump(Ta, d), Tb) - pg.residual(Z, bump(Ta, -d), Tb)) / (2.0 * h)
            Nb[:, k] = (pg.residual(Z, Ta, bump(Tb, d)) - pg.residual(Z, Ta, bump(Tb, -d))) / (2.0 * h)
        worst = max(worst, float(np.abs(Na - Ja).max()), float(np.abs(Nb - Jb).max()))
    print("largest |J - central difference|:", worst)
    assert worst < 1e-7
    coef = (1.0, 0.5, 1.0 / 12.0, 0.0, -1.0 / 720.0, 0.0, 1.0 / 30240.0, 0.0, -1.0 / 1209600.0, 0.0, 1.0 / 47900160.0, 0.0, -691.0 / 1307674368000.0)
    for angle in (0.5, 1.0001e-2, 0.9999e-2, 1e-5):                            # Jr^-1 = sum B_n / n! (-ad)^n, twelve terms: both branches meet it
        xi = np.array([0.3, -0.2, 0.5, 6.0, 4.0, -5.0])
        xi[3:] *= angle / np.linalg.norm(xi[3:])
        ad = np.zeros((6, 6))
        ad[:3, :3] = ad[3:, 3:] = pg.sw._hat_np(xi[3:])
        ad[:3, 3:] = pg.sw._hat_np(xi[:3])
        series, power = np.zeros((6, 6)), np.eye(6)
        for c in coef:
            series, power = series + c * power, power @ ad
        assert np.abs(pg.right_jacobian_inverse(xi) - series).max() < 1e-12, angle   # the next term is (angle / 2 pi)^14: 4e-16 at 0.5 rad
    assert np.array_equal(pg.right_jacobian_inverse(np.zeros(6)), np.eye(6))
    T = pc.exp34([1.0, 2.0, 3.0, 0.3, -0.2, 0.9])                              # Ad: T Exp(d) T^-1 = Exp(Ad(T) d)
    d = np.array([1e-3, -2e-3, 5e-4, 3e-4, 2e-4, -1e-3])
    left = pg._compose(pc.exp34(pg.adjoint(T) @ d), T[:, :3], T[:, 3])            # Exp(Ad(T) d) T
    assert np.abs(left - bump(T, d)).max() < 1e-14


# ---- 2. the solver ------------------------------------------------------------------------------------------------------------------------------------------------

def test_a_graph_that_agrees_with_its_poses_returns_them_bit_for_bit():
    truth, chain, edges, loop = pc.trajectory()
    agree = [dict(e, Z=pg.relative(chain[e["a"]][:3], chain[e["b"]][:3])) for e in edges + [loop]]
    out, rep = pg.optimize(chain, agree)
    assert rep["cost"] == [0.0] and rep["iterations"] == 0 and rep["converged"]
    assert all(np.array_equal(out[i], chain[i]) for i in chain)
    out, rep = pg.optimize({7: chain[7]}, [])                                    # one pose, nothing to solve
    assert np.array_equal(out[7], chain[7]) and rep["iterations"] == 0 and rep["unknowns"] == 0


def test_one_exact_loop_edge_closes_the_seeded_trajectory():
    truth, chain, edges, loop = pc.trajectory()
    n = pc.GRAPH["n"]
    before = pc.position_errors(chain, truth)
    assert before[-1] >= 100.0 * pg.DEFAULT_TOL and before[-1] > 0.05
    out, rep = pg.optimize(chain, edges + [loop])
    after = pc.position_errors(out, truth)
    print("last pose's error: chain", before[-1], "solved", after[-1], "cost", rep["cost"][0], "->", rep["cost"][-1], "iterations", rep["iterations"])
    assert rep["converged"] and rep["cost"][-1] < rep["cost"][0] and all(b <= a for a, b in zip(rep["cost"], rep["cost"][1:]))
    # n - 1 odometry edges and the loop edge carry the same information, so the minimiser spreads the chain's closing error evenly over the n
    # edges of the cycle (springs of one stiffness in a row): the loop edge keeps 1 / n of it, and the last pose hangs on the fixed first one by
    # that edge alone.  The solver stops at steps below tol, which moves no pose by more than tol per coordinate.
    bound = before[-1] / n + math.sqrt(3.0) * pg.DEFAULT_TOL
    assert after[-1] <= bound, (after[-1], bound)
    assert bool((after <= before).all()), np.nonzero(after > before)[0]         # no node ends further from the truth than the chain had it
    assert before[-1] <= 2.0 * pc.RECORDED_GRAPH["last_chain"] and after[-1] <= 2.0 * pc.RECORDED_GRAPH["last_solved"]
    assert rep["loops"][0]["before"][0] > 0.05 and rep["loops"][0]["after"][0] <= bound and rep["loops"][0]["kind"] == "loop"
    assert out[0].tobytes() == chain[0].tobytes()                                # the lowest id is fixed


def test_a_failed_odometry_pair_keeps_the_system_solvable():
    truth, chain, edges, loop = pc.trajectory()
    steps = [{"source": e["b"], "target": e["a"], "X": e["Z"], "hessian": e["info"], "status": rg.CONVERGED} for e in edges]
    steps[10] = dict(steps[10], status=rg.FEW, hessian=np.zeros((6, 6)))         # kept its guess: its hessian says nothing
    steps[20] = dict(steps[20], status=rg.PIVOT, hessian=np.full((6, 6), np.nan))
    made = pg.odometry_edges(steps)
    assert [e["kind"] for e in made].count("weak") == 2 and made[10]["kind"] == "weak"
    assert np.array_equal(made[10]["info"], pg.DEFAULT_WEAK_SCALE * pc.GRAPH["info"] * np.eye(6)) and np.array_equal(made[9]["info"], edges[9]["info"])
    out, rep = pg.optimize(chain, made + [loop])
    assert rep["converged"] and all(np.isfinite(out[i]).all() for i in out)
    after = pc.position_errors(out, truth)
    assert after[-1] < 1e-3 and [l["kind"] for l in rep["loops"]] == ["weak", "weak", "loop"]
    out, rep = pg.optimize(chain, pg.odometry_edges(steps, weak_info=1e-9))     # no loop edge: the weak edges alone still hold their nodes
    assert rep["converged"] and all(np.isfinite(out[i]).all() for i in out)
    with pytest.raises(pg.PoseGraphError, match="weak_info"):
        pg.odometry_edges(steps, weak_info=0.0)
    cut, rep = pg.optimize(chain, [e for k, e in enumerate(edges) if k != 10] + [loop])      # without the pair at all the loop edge holds the far side
    assert rep["converged"] and pc.position_errors(cut, truth)[-1] < 1e-3


def test_a_graph_over_the_limit_raises():
    n = pg.MAX_UNKNOWNS // 6 + 2
    poses = {i: np.eye(4) for i in range(n)}
    with pytest.raises(pg.PoseGraphError, match=f"6 \\(F - 1\\) <= {pg.MAX_UNKNOWNS}"):
        pg.optimize(poses, [])
    with pytest.raises(pg.PoseGraphError, match="two different ids"):
        pg.optimize({0: np.eye(4), 1: np.eye(4)}, [{"a": 0, "b": 5, "Z": np.eye(4)[:3], "info": np.eye(6)}])
    with pytest.raises(pg.PoseGraphError, match="info must be"):
        pg.optimize({0: np.eye(4), 1: np.eye(4)}, [{"a": 0, "b": 1, "Z": np.eye(4)[:3], "info": np.eye(3)}])


# ---- 3. the room tour, end to end on the twins ----------------------------------------------------------------------------------------------------------------------

def test_the_tour_ends_where_the_cases_say():
    truth = pc.tour_truth()
    X = pg.relative(truth[0][:3], truth[pc.TOUR["n"] - 1][:3])
    t, a = rc.pose_error(X, np.eye(4)[:3])
    assert len(truth) <= 10 and t <= 0.5 and a <= math.radians(5.0) and t > 0.2
    fr, _ = pc.tour()
    pts, msk = torch.stack([fr[i][0] for i in sorted(fr)]), torch.stack([fr[i][2] for i in sorted(fr)])
    desc, sums = place.describe(pts, msk, -pc.TOUR["sensor_height"], r_max=pc.TOUR["r_max"])
    bd, bs = place.match(desc, pc.TOUR["gap"])
    assert int((bd >= 0).sum()) == 1 and int(bd[8, 0]) >= 0                      # the gap leaves only the closing pair eligible


def test_close_loops_finds_and_accepts_the_closing_pair():
    ref = pc.tour_reference()
    fr, truth = pc.tour()
    assert [(r["source"], r["target"]) for r in ref.loop_report["accepted"]] == [(8, 0)] and ref.loop_report["rejected"] == []
    row = ref.loop_report["accepted"][0]
    print("the closing pair:", row)
    assert row["score"] <= place.DEFAULT_MAX_SCORE and row["overlap"] >= pg.DEFAULT_MIN_OVERLAP and row["rms"] <= pg.DEFAULT_MAX_RMS and row["status"] == rg.CONVERGED
    assert abs(row["score"] - pc.TOUR_TABLE[0][3]) < 1e-3 and abs(row["overlap"] - pc.TOUR_TABLE[0][4]) < 1e-3 and abs(row["rms"] - pc.TOUR_TABLE[0][5]) < 1e-4
    edge = ref.loops[0]
    assert (edge["a"], edge["b"], edge["kind"]) == (0, 8, "loop") and edge["info"].shape == (6, 6)
    Zt = pc.closing_truth()
    alone = rg.align_reference(fr[8], fr[0], None, pg.LOOP_SCHEDULE, **pc.TOUR_KW)
    e_alone, e_loop = rc.pose_error(alone.X.numpy(), Zt), rc.pose_error(edge["Z"], Zt)
    print("the closing pair's X against the truth:", e_loop, "align_reference alone:", e_alone)
    assert e_alone[0] <= 2.0 * pc.RECORDED_TOUR["align_alone"][0] and e_alone[1] <= 2.0 * pc.RECORDED_TOUR["align_alone"][1]
    assert e_loop[0] <= 2.0 * pc.RECORDED_TOUR["align_alone"][0] and e_loop[1] <= 2.0 * pc.RECORDED_TOUR["align_alone"][1]


def test_optimize_does_not_open_the_loop_the_chain_had():
    ref = pc.tour_reference()
    Zt = pc.closing_truth()
    chain, solved = pg.closure_error(ref.chain, 0, 8, Zt), pg.closure_error(ref.solved, 0, 8, Zt)
    print("closure error: chain", chain, "solved", solved)
    assert solved[0] <= chain[0] and solved[1] <= chain[1]
    assert chain[0] <= 2.0 * pc.RECORDED_TOUR["closure_chain"][0] and chain[1] <= 2.0 * pc.RECORDED_TOUR["closure_chain"][1]
    assert solved[0] <= 2.0 * pc.RECORDED_TOUR["closure_solved"][0] and solved[1] <= 2.0 * pc.RECORDED_TOUR["closure_solved"][1]
    rep = ref.solve_report
    assert rep["converged"] and rep["cost"][-1] < rep["cost"][0] and rep["unknowns"] == 48 and rep["edges"] == 9
    assert rep["loops"][0]["after"][0] < rep["loops"][0]["before"][0] and rep["loops"][0]["shift"] == 0 and rep["loops"][0]["partners"] > 1000
    assert np.array_equal(ref.solved[0], ref.chain[0])


def test_a_wrong_loop_edge_beyond_max_drift_is_rejected_before_the_solve():
    ref = pc.tour_reference()
    fr, truth = pc.tour()
    far = {i: T.copy() for i, T in ref.chain.items()}
    far[8][:3, 3] += np.array([6.0, 0.0, 0.0])                                   # a chain that says frame 8 stands 6 m from frame 0
    loops, rep = pg.close_loops(fr, far, ref.steps, sensor_height=pc.TOUR["sensor_height"], gap=pc.TOUR["gap"], r_max=pc.TOUR["r_max"], **pc.TOUR_KW)
    assert loops == [] and rep["accepted"] == [] and rep["candidates"] == 1
    assert (rep["rejected"][0]["source"], rep["rejected"][0]["target"]) == (8, 0) and "max_drift 0.1" in rep["rejected"][0]["reason"]
    path = pg.path_lengths(far)[1][-1]
    assert 6.0 > 0.1 * path + rep["reach"] and rep["reach"] == (pc.TOUR["r_max"] - place.DEFAULT_R_MIN) / place.DEFAULT_RINGS
    tight, rep = pg.close_loops(fr, ref.chain, ref.steps, sensor_height=pc.TOUR["sensor_height"], gap=pc.TOUR["gap"], r_max=pc.TOUR["r_max"], max_rms=0.001, **pc.TOUR_KW)
    assert tight == [] and "max_rms 0.001" in rep["rejected"][0]["reason"]
    none, rep = pg.close_loops(fr, ref.chain, ref.steps, sensor_height=pc.TOUR["sensor_height"], gap=pc.TOUR["gap"], r_max=pc.TOUR["r_max"], max_score=0.1, **pc.TOUR_KW)
    assert none == [] and rep["candidates"] == 0
    with pytest.raises(pg.PoseGraphError, match="sensor_height is required"):
        pg.close_loops(fr, ref.chain, ref.steps, **pc.TOUR_KW)
    with pytest.raises(pg.PoseGraphError, match="the same ids"):
        pg.close_loops(fr, {0: np.eye(4)}, ref.steps, sensor_height=1.8, **pc.TOUR_KW)


def test_odometry_returns_its_steps_only_when_asked():
    fr, truth = pc.tour()
    two = {i: fr[i] for i in (0, 1, 2)}
    plain, rep0 = rg.odometry(two, **pc.TOUR_KW)
    again, rep1 = rg.odometry(two, return_steps=True, **pc.TOUR_KW)
    assert "steps" not in rep0 and sorted(rep1) == sorted(list(rep0) + ["steps"]) and {k: rep1[k] for k in rep0} == rep0
    assert all(np.array_equal(plain[i], again[i]) for i in plain)
    for k, s in enumerate(rep1["steps"]):
        reg = rg.align_reference(fr[k + 1], fr[k], None if k == 0 else torch.from_numpy(rep1["steps"][k - 1]["X"]), **pc.TOUR_KW)
        assert (s["source"], s["target"], s["status"]) == (k + 1, k, int(reg.status))
        assert np.array_equal(s["X"], reg.X.numpy()) and np.array_equal(s["hessian"], reg.hessian.numpy())


# ---- 4. ingest ------------------------------------------------------------------------------------------------------------------------------------------------------

COMMON = ["--height", "16", "--width", "128", "--inclination", str(rc.BOUNDS[0]), str(rc.BOUNDS[1]), "--device", "cpu", "--max-depth", "80"]


def _write_clouds(folder, frames):
    os.makedirs(folder, exist_ok=True)
    for i, (pts, _, mask) in frames.items():
        p = pts[mask].numpy()
        np.save(os.path.join(folder, f"{i}.npy"), np.concatenate([p, np.full((p.shape[0], 1), 0.5, np.float32)], 1))


def test_ingest_refuses_loop_closure_without_its_partners(tmp_path, capsys):
    fr, _ = pc.tour()
    pts, out = str(tmp_path / "pts"), str(tmp_path / "out")
    _write_clouds(pts, {i: fr[i] for i in (0, 1)})
    np.save(str(tmp_path / "poses.npy"), np.stack([np.eye(4)] * 2))
    assert ingest.main(["--points", pts, "--out", out, "--poses", str(tmp_path / "poses.npy"), "--loop-closure", "--sensor-height", "1.8"] + COMMON) == 2
    assert "--loop-closure goes with --odometry" in capsys.readouterr().err
    assert ingest.main(["--points", pts, "--out", out, "--odometry", "--loop-closure"] + COMMON) == 2
    assert "--loop-closure and --sensor-height Z go together" in capsys.readouterr().err
    assert ingest.main(["--points", pts, "--out", out, "--odometry", "--sensor-height", "1.8"] + COMMON) == 2
    assert "--discover-actors and --sensor-height Z go together" in capsys.readouterr().err
    assert not os.path.exists(out)
    with pytest.raises(ValueError, match="loop_closure needs sensor_height"):
        ingest.ingest_point_clouds(out, [(0, np.zeros((4, 4), np.float32), None)], 16, 128, list(rc.BOUNDS), device="cpu", odometry={"loop_closure": {}})


def test_ingest_with_loop_closure_writes_poses_that_close_the_loop(tmp_path, capsys):
    fr, truth = pc.tour()
    pts, plain, closed = str(tmp_path / "pts"), str(tmp_path / "plain"), str(tmp_path / "closed")
    _write_clouds(pts, fr)
    np.savetxt(str(tmp_path / "first.txt"), truth[0])
    base = ["--points", pts, "--odometry", "--first-pose", str(tmp_path / "first.txt")] + COMMON
    assert ingest.main(base + ["--out", plain]) == 0
    assert ingest.main(base + ["--out", closed, "--loop-closure", "--sensor-height", "1.8", "--loop-gap", "8", "--place-range", "20"]) == 0
    assert "1 loops closed" in capsys.readouterr().out
    a, b = json.load(open(os.path.join(plain, "ingest.json"))), json.load(open(os.path.join(closed, "ingest.json")))
    assert "loop_closure" not in a["odometry"]
    lc = b["odometry"].pop("loop_closure")
    assert {k: v for k, v in b["odometry"].items() if k != "first_pose"} == {k: v for k, v in a["odometry"].items() if k != "first_pose"}
    assert [(r["source"], r["target"]) for r in lc["accepted"]] == [(8, 0)] and lc["rejected"] == [] and lc["gap"] == 8 and lc["top"] == 2
    assert lc["closure_error"] < lc["closure_error_chain"] and lc["converged"] and lc["cost"][-1] < lc["cost"][0]
    Zt = pc.closing_truth()
    read = lambda root: {i: np.load(sequence._frame_path(root, i))["sensor2world"].astype(np.float64) for i in (0, 8)}
    e_plain, e_closed = pg.closure_error(read(plain), 0, 8, Zt), pg.closure_error(read(closed), 0, 8, Zt)
    print("closure error of the written poses: chain", e_plain, "closed", e_closed)
    assert e_closed[0] < e_plain[0] and e_closed[1] < e_plain[1]
