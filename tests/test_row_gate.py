"""Negative controls of the per-row gate (tests/row_gate.py), on the CPU: the float32 oracle plays the implementation.  Clean, it must be
accepted on every scene of tests/test_row_gradients_gpu.py with at least 70 % of the touched rows sensitive and without one event ray of
its own.  Corrupted one way at a time on the deep scene it must be REFUSED -- while the statistics the suite had until now (relative L2 below
1e-3 and at most 2e-3 of the elements outside 1e-3, tests/test_hip_parity.py) still pass, against the float32 oracle and against the
float64 one.  Where a corruption of every row would move those statistics (1 % on an axis of `d_scales`, a sign on 1 % of the `d_rotations`
rows) it is applied to as many of the smallest sensitive rows as they let through: the gate has to see a few rows, which is its point."""
import numpy as np
import pytest

from tests import row_gate
from tests.hip_util import frac_outside, rel_l2
from tests.row_gate import GRADS, Reference, SCENES, scene

BG = (0.3, 0.7, 0.2)
ALL = GRADS + ("accum",)


def old_statistics_pass(x, bw):
    return all(rel_l2(x[k], bw[p][k]) < 1e-3 and frac_outside(x[k], bw[p][k], 1e-3) <= 2e-3 for k in ALL for p in ("f32", "f64"))


@pytest.fixture(scope="module")
def deep():
    ref = Reference(*scene(*SCENES["deep"]), 3, BG)
    mask = ref.f32_events
    bw = ref.backward(mask)
    stats = {k: row_gate.row_stats(bw["f32"][k], bw["f64"][k]) for k in ALL}
    sens = np.all([stats[k][4] for k in ALL], 0)          # rows that are sensitive in every tensor
    assert sens.sum() > 100
    return ref, mask, bw, stats, sens


def _copy(g):
    return {k: np.array(v, np.float64, copy=True) for k, v in g.items()}


@pytest.mark.parametrize("name", list(SCENES))
def test_clean_float32_oracle_is_accepted(name):
    ref = Reference(*scene(*SCENES[name]), 3, BG)
    assert ref.f32_events.sum() == 0, (name, np.nonzero(ref.f32_events)[0])         # seeds without an event ray of the float32 oracle's own
    bw = ref.backward(ref.f32_events)
    row_gate.check(name, "f32-oracle", bw["f32"], bw["f32"], bw["f64"])             # (asserts the 70 % sensitive rows too)
    assert old_statistics_pass(bw["f32"], bw)
    if name == "deep":
        fw = ref._oracle("f64").forward(ref.o, ref.d, ref.sc["shs"], 3, ref.bg, stats=True)
        assert fw["n_comp"].mean() >= 15 and fw["n_comp"].max() > 16
    if name == "deep-unhittable":
        assert not bw["f64"]["accum"][::5].any() and not bw["f64"]["means"][::5].any()
    if name == "deep-by-distance":
        assert (np.diff(np.linalg.norm(ref.sc["means"], axis=1)) >= 0).all() and ref.P % 64 != 0


def _by_size(bw, stats, rows_):
    """`rows_` (a mask) in ascending order of what a row weighs in the relative L2 of its tensor: max over the tensors of |row| / |tensor|."""
    z = np.max([np.linalg.norm(row_gate.rows(bw["f64"][k], len(rows_)), axis=1) / np.linalg.norm(bw["f64"][k]) for k in ALL], 0)
    idx = np.nonzero(rows_)[0]
    return idx[np.argsort(z[idx], kind="stable")]


# Each corruption yields candidates, the literal one first and then smaller ones; the test takes the first that the old statistics let through.
def _one_ray_removed(ref, mask, bw, stats, sens):
    for g in _by_size(bw, stats, sens):                  # a sensitive Gaussian; the ray in the middle of those that composite it
        rays = [r for r in range(ref.HW) if int(g) in ref.seq["f32"][r].tolist() and not mask[r]]
        if len(rays) < 2:
            continue
        m2 = mask.copy(); m2[rays[len(rays) // 2]] = True
        less = ref.backward(m2)["f32"]
        x = _copy(bw["f32"])
        for k in GRADS:
            x[k][g] = less[k][g]
        yield f"Gaussian {g}, 1 of {len(rays)} rays", x


def _rows_swapped(ref, mask, bw, stats, sens):
    order = _by_size(bw, stats, stats["accum"][3])[::-1]       # neighbours in size, the largest pair first: the largest swap the old statistics miss
    for i in range(0, len(order) - 1, 2):
        a, b = order[i], order[i + 1]
        x = _copy(bw["f32"])
        for k in ALL:
            x[k][[a, b]] = x[k][[b, a]]
        yield f"rows {a} and {b} (ranks {i}, {i + 1} of {len(order)} by size)", x


def _scales_axis_1_percent(ref, mask, bw, stats, sens):
    s, T, c = stats["scales"][:3]
    col = np.abs(bw["f64"]["scales"][:, 1])
    # 0.01 |x_1| > 1e-3 s + c T  <=  |x_1| = s >= 200 c T: rows the rule must refuse
    sure = np.nonzero((col == s) & (s >= 200 * c * T))[0]
    sure = sure[np.argsort(s[sure], kind="stable")]
    for idx, name in [(np.nonzero(stats["scales"][3])[0], "every touched row")] + [(sure[:n], f"the {n} smallest rows with |x_1| = s >= 200 c T") for n in (8, 4, 2, 1)]:
        x = _copy(bw["f32"]); x["scales"][idx, 1] *= 1.01
        yield name, x


def _rotations_negated(ref, mask, bw, stats, sens):
    s, T, c, touched = stats["rotations"][:4]
    t_idx = np.nonzero(touched)[0]
    n1 = max(len(t_idx) // 100, 1)
    # 2 s > 1e-3 s + c T  <=  s >= c T: rows the rule must refuse
    sure = np.nonzero(touched & (s >= c * T))[0]
    rng = np.random.default_rng(3)
    cands = [(rng.choice(t_idx, n1, replace=False), f"a random 1 % ({n1}) of the touched rows")]
    for n in (8, 4, 2, 1):
        cands.append((rng.choice(sure, n, replace=False), f"{n} random rows with s >= c T"))
    small = sure[np.argsort(s[sure], kind="stable")]
    for n in (8, 4, 2, 1):
        cands.append((small[:n], f"the {n} smallest rows with s >= c T"))
    for idx, name in cands:
        x = _copy(bw["f32"]); x["rotations"][idx] *= -1.0
        yield name, x


def _last_touched_row_zeroed(ref, mask, bw, stats, sens):
    touched = np.nonzero(stats["accum"][3])[0]
    for g in touched[::-1]:                              # the last touched row, else the last one before it that ...
        if g != touched[-1] and not sens[g]:
            continue
        x = _copy(bw["f32"])
        for k in ALL:
            x[k][g] = 0.0
        yield f"row {g} ({len(touched) - 1 - int(np.searchsorted(touched, g))} touched rows from the end)", x


def _untouched_row_leftover(ref, mask, bw, stats, sens):
    x = _copy(bw["f32"])
    g = int(np.nonzero(~stats["accum"][3])[0][0])
    x["means"][g, 2] = 1e-6
    yield f"row {g}", x


def _accum_halved(ref, mask, bw, stats, sens):
    for g in _by_size(bw, stats, sens)[:4]:
        x = _copy(bw["f32"]); x["accum"][g] *= 0.5
        yield f"row {g}", x


CORRUPTIONS = {"one ray's contribution removed from a row": _one_ray_removed, "two touched rows swapped": _rows_swapped,
               "column 1 of d_scales x 1.01": _scales_axis_1_percent, "d_rotations negated": _rotations_negated,
               "last touched row zeroed": _last_touched_row_zeroed, "1e-6 left in an untouched row": _untouched_row_leftover,
               "accum of one row halved": _accum_halved}


@pytest.mark.parametrize("what", list(CORRUPTIONS))
def test_corruption_passes_the_old_statistics_and_is_refused(deep, what):
    ref, mask, bw, stats, sens = deep
    assert not row_gate.accepted(bw["f32"], bw["f32"], bw["f64"])
    for name, x in CORRUPTIONS[what](*deep):
        if old_statistics_pass(x, bw):
            break
    else:
        pytest.fail(f"{what}: no variant passes the old statistics")
    refused = row_gate.accepted(x, bw["f32"], bw["f64"])
    print(f"ROWGATE-CONTROL|{what}|{name}|refused by {refused}")
    assert refused, (what, name)
