"""The LBVH checker of tests/bvh_check.py tested without a GPU: a checker that can only pass protects nothing.

The layout restatement is pinned to hand-derived level counts, the numpy reference builder's trees pass the checker, and every single mutation
of a passing tree that tests/test_lbvh_invariants_gpu.py relies on the checker to see is reported under the invariant it breaks."""
import functools

import numpy as np
import pytest

from lidar_rt_amd import scenes
from tests import bvh_check as bc

# P -> (leaves, [nodes of level 1, 2, ...]): 8 slots per leaf, ceil(n / 8) nodes over n children, at least one
LAYOUTS = {
    0: (0, [1]), 1: (1, [1]), 8: (1, [1]), 9: (2, [1]), 64: (8, [1]), 65: (9, [2, 1]), 512: (64, [8, 1]), 513: (65, [9, 2, 1]),
    4096: (512, [64, 8, 1]), 4097: (513, [65, 9, 2, 1]),                                    # the first tree with 4 levels
    32_769: (4097, [513, 65, 9, 2, 1]),                                                     # ... with 5
    262_145: (32_769, [4097, 513, 65, 9, 2, 1]),                                            # ... with 6
    8_388_609: (1_048_577, [131_073, 16_385, 2049, 257, 33, 5, 1]),                         # the first with 257 level-4 nodes
}


@pytest.mark.parametrize("P", sorted(LAYOUTS))
def test_layout_gives_the_hand_derived_level_counts(P):
    leaves, counts = LAYOUTS[P]
    lay = bc.tree_layout(P)
    assert lay.leaves == leaves and lay.levels == len(counts) and lay.cnt[0] == leaves and lay.cnt[1:] == counts
    assert lay.n_nodes == sum(counts) and lay.off[lay.levels] == 0                        # the root is node 0, the levels follow top down
    for l in range(lay.levels, 1, -1):
        assert lay.off[l - 1] == lay.off[l] + lay.cnt[l]
    if P == 8_388_609:
        assert lay.cnt[4] == 257 and bc.tree_layout(P - 1).cnt[4] == 256


def _params(P, seed=5):
    sc = scenes.make_scene(P, seed=seed, radius_scale=0.25)
    return {k: sc[k] for k in ("means", "scales", "rotations", "opacities")}


def _order(p):
    """Some spatial order (any permutation gives a valid tree): by x."""
    return np.argsort(p["means"][:, 0], kind="stable")


@functools.lru_cache(maxsize=None)
def _passing(P=4097):
    p = _params(P)
    order = _order(p)
    rec, soa, aos = bc.reference_tree(order, p)
    for a in (order, rec, soa, aos):
        a.setflags(write=False)
    return p, order, rec, soa, aos


@pytest.mark.parametrize("mod", [1.0, 0.5])
@pytest.mark.parametrize("P", [5, 513, 4097])
def test_reference_trees_pass(P, mod):
    p = _params(P)
    order = _order(p)
    rec, soa, aos = bc.reference_tree(order, p, mod)
    assert rec.shape == (P, 16) and soa.shape == aos.shape == (bc.tree_layout(P).n_nodes, 64)
    assert bc.quads64(**p).hittable.sum() > 0.8 * P
    assert not bc.check_tree(order, rec, soa, aos, p, mod)
    assert not bc.check_nodes(soa, aos, P, None, from_level=2)


def test_reference_tree_with_unhittable_gaussians_at_the_end_and_in_the_middle_passes():
    P = 4097
    p = _params(P)
    order = _order(p)
    p["opacities"] = p["opacities"].copy(); p["means"] = p["means"].copy(); p["scales"] = p["scales"].copy()
    p["opacities"][order[-700:]] = 0.001                     # a whole level-2 node's worth of trailing slots: empty leaves, empty level-1 nodes
    p["opacities"][order[1000:1100]] = 0.0                   # whole leaves in the middle
    p["means"][order[2000:2003]] = np.nan
    p["scales"][order[2500]] = 0.0
    q = bc.quads64(**p)
    assert not q.hittable[order[-700:]].any() and not q.hittable[order[1000:1100]].any() and not q.hittable[order[[2000, 2001, 2002, 2500]]].any()
    rec, soa, aos = bc.reference_tree(order, p)
    assert not bc.check_tree(order, rec, soa, aos, p)
    lay = bc.tree_layout(P)
    _, _, ptr, flag = bc.aos_boxes(aos)
    l1 = flag[lay.off[1]:]
    assert l1[15].tolist() == [1, 1, 1, 1, 1, 2, 2, 2] and (l1[16] == 2).all() and l1[17].tolist() == [2] + [1] * 7      # leaves 125 .. 136 (slots 1000 .. 1095) hold nothing to hit
    assert (l1[54:] == 2).all() and l1[53].tolist() == [1] + [2] * 7                                        # the trailing 700 slots: leaves 425 .. 512
    assert (flag[lay.off[2]:lay.off[1]].reshape(-1)[:lay.cnt[1]] == 2).sum() == 12                         # ... and the level-1 nodes 16 and 54 .. 64 above them


def test_a_culled_tree_with_a_padding_tail_passes():
    """A subset of the Gaussians in 1024 slots, the tail padding: the culled form of I1 (order None)."""
    P = 4097
    p = _params(P)
    order = _order(p)[100:900]
    rec, soa, aos = bc.reference_tree(order, p, slots=1024)
    assert bc.padding_slots(rec)[800:].all() and not bc.padding_slots(rec)[:800].any()
    assert not bc.check_tree(None, rec, soa, aos, p)
    rec2 = rec.copy(); rec2[10] = rec2[11]
    assert bc.tags(bc.check_tree(None, rec2, soa, aos, p)) >= {"I1"}
    rec2 = rec.copy(); rec2[900, 3] = 0.5; rec2[900, 7] = 3.0        # a padding slot that claims a Gaussian: nothing below its leaf's empty child
    assert bc.tags(bc.check_tree(None, rec2, soa, aos, p)) >= {"I5"}


# ------------------------------------------------------------------------------------------------------------------ mutations
def _both(soa, aos, node, child, axis, hi, value):
    """Set one face of one child's box in both copies."""
    soa[node, (24 if hi else 0) + 8 * axis + child] = value
    aos[node, 8 * child + 2 * axis + (1 if hi else 0)] = value


def _mutants():
    p, order, rec, soa, aos = _passing()
    lay = bc.tree_layout(rec.shape[0])
    q = bc.quads64(**p)
    out = {}

    def fresh():
        return rec.copy(), soa.copy(), aos.copy()

    # a leaf whose parent box it does not define on the mutated face, so that the mutation breaks nothing one level up: found by search
    slo, shi = bc.soa_boxes(soa)
    l1 = slice(lay.off[1], lay.off[1] + lay.cnt[1])
    inner = np.nonzero((shi[l1][:, :, 0] < shi[l1][:, :, 0].max(1, keepdims=True)) & (shi[l1][:, :, 0] < 1e29))
    j1, c1 = int(inner[0][0]), int(inner[1][0])
    leaf = 8 * j1 + c1
    slots = np.arange(8 * leaf, 8 * leaf + 8)
    k_max = slots[np.argmax(q.corners[order[slots]][:, :, 0].max(1))]

    r, s, a = fresh()                                       # one leaf box shrunk past one corner
    _both(s, a, lay.off[1] + j1, c1, 0, True, np.float32(q.corners[order[k_max]][:, 0].max() - 1e-3))
    out["leaf box shrunk past a corner"] = ((r, s, a), {"I2"}, set())
    r, s, a = fresh()                                       # ... by one float32 step of the corner itself (zero tolerance)
    _both(s, a, lay.off[1] + j1, c1, 0, True, np.nextafter(np.float32(q.corners[order[k_max]][:, 0].max()), np.float32(-np.inf)))
    out["leaf box one ulp inside a corner"] = ((r, s, a), {"I2"}, set())
    r, s, a = fresh()                                       # one leaf box swollen by a metre (towards -x, where it may define the parent: I4 may follow)
    _both(s, a, lay.off[1] + j1, c1, 0, False, s[lay.off[1] + j1, c1] - np.float32(1.0))
    out["leaf box swollen by a metre"] = ((r, s, a), {"I3"}, {"I4"})
    r, s, a = fresh()                                       # ... by three pads
    g_min = order[slots[np.argmin((q.mu - q.h)[order[slots]][:, 0])]]
    _both(s, a, lay.off[1] + j1, c1, 0, False, np.float32((q.mu - q.h - 3 * q.pad)[g_min, 0]))
    out["leaf box swollen by three pads"] = ((r, s, a), {"I3"}, {"I4"})
    r, s, a = fresh()                                       # one upper box not the union of its children
    _both(s, a, lay.off[2] + 3, 2, 1, True, s[lay.off[2] + 3, 24 + 8 + 2] + np.float32(1e-3))
    out["upper box not the union"] = ((r, s, a), {"I4"}, set())
    r, s, a = fresh()                                       # a stale, larger top-level box: the root's child 0 as a wider scene left it
    for axis in range(3):
        _both(s, a, 0, 0, axis, False, s[0, 8 * axis] - np.float32(30.0))
        _both(s, a, 0, 0, axis, True, s[0, 24 + 8 * axis] + np.float32(30.0))
    out["stale larger top box"] = ((r, s, a), {"I4"}, set())
    r, s, a = fresh()                                       # a non-empty child flagged empty: a subtree hidden from the walk
    a[lay.off[3] + 1, 8 * 0:8 * 0 + 6] = bc.EMPTY
    a.view(np.int32)[lay.off[3] + 1, 6:8] = (0, 2)
    out["non-empty child flagged empty (AoS)"] = ((r, s, a), {"I5", "I8"}, {"I7"})
    r, s, a = fresh()                                       # the same in both copies
    a[lay.off[3] + 1, 0:6] = bc.EMPTY
    a.view(np.int32)[lay.off[3] + 1, 6:8] = (0, 2)
    s[lay.off[3] + 1, 0:48:8] = bc.EMPTY
    out["non-empty child flagged empty (both)"] = ((r, s, a), {"I5", "I8"}, {"I4"})
    r, s, a = fresh()                                       # an empty child with a live box: the last level-1 node's unused child slots
    last = lay.off[1] + lay.cnt[1] - 1
    assert (a.view(np.int32)[last, 15::8] == 2).all()       # 513 leaves: the last level-1 node holds one
    a[last, 8 * 5:8 * 5 + 6] = a[last, 0:6]
    a.view(np.int32)[last, 8 * 5 + 6:8 * 5 + 8] = (8 * (lay.cnt[1] - 1) + 5, 1)
    s[last, 5:48:8] = s[last, 0:48:8]
    out["empty child with a live box"] = ((r, s, a), {"I5"}, {"I4", "I8"})
    r, s, a = fresh()                                       # two child pointers of one kind swapped: every leaf is still walked once, I6 alone can see it
    ai = a.view(np.int32)
    ai[lay.off[2] + 1, [6, 14]] = ai[lay.off[2] + 1, [14, 6]]
    out["two child pointers swapped"] = ((r, s, a), {"I6"}, set())
    r, s, a = fresh()                                       # a leaf pointer and an inner pointer swapped: the walk loses a subtree and meets a leaf that is none
    ai = a.view(np.int32)
    ai[lay.off[2] + 1, 6], ai[lay.off[1] + 20, 6] = ai[lay.off[1] + 20, 6], ai[lay.off[2] + 1, 6]
    out["a leaf and an inner pointer swapped"] = ((r, s, a), {"I6", "I8"}, set())
    r, s, a = fresh()                                       # a child pointer that repeats its neighbour's: one subtree walked twice, one never
    ai = a.view(np.int32)
    ai[lay.off[2] + 1, 6] = ai[lay.off[2] + 1, 14]
    out["a child pointer repeated"] = ((r, s, a), {"I6", "I8"}, set())
    r, s, a = fresh()                                       # one AoS box word differing from SoA, by one float32 step
    a[lay.off[1] + 7, 8 * 3 + 2] = np.nextafter(a[lay.off[1] + 7, 8 * 3 + 2], np.float32(-np.inf))
    out["one AoS box word differs"] = ((r, s, a), {"I7"}, set())
    r, s, a = fresh()                                       # a record index repeated
    r.view(np.int32)[200, 11] = r.view(np.int32)[201, 11]
    out["record index repeated"] = ((r, s, a), {"I1"}, {"I2"})
    r, s, a = fresh()                                       # a hittable record marked -1
    assert r[300, 3] > 0
    r[300, 3] = r[300, 7] = -1
    out["hittable record marked -1"] = ((r, s, a), {"I1"}, {"I3"})     # (its leaf's box still holds it: larger than the quads that are left)
    r, s, a = fresh()                                       # a wrong header, a wrong leaf flag
    s.view(np.int32)[lay.off[1] + 2, 48] += 8
    a.view(np.int32)[lay.off[1] + 2, 7] = 0
    out["wrong header and leaf flag"] = ((r, s, a), {"I6", "I8"}, set())
    r, s, a = fresh()                                       # a NaN box word
    _both(s, a, lay.off[1] + 4, 1, 2, True, np.float32(np.nan))
    out["NaN box word"] = ((r, s, a), {"I5"}, {"I2", "I3", "I4"})
    return p, order, out


MUTANTS = ["leaf box shrunk past a corner", "leaf box one ulp inside a corner", "leaf box swollen by a metre", "leaf box swollen by three pads",
           "upper box not the union", "stale larger top box", "non-empty child flagged empty (AoS)", "non-empty child flagged empty (both)",
           "empty child with a live box", "two child pointers swapped", "a leaf and an inner pointer swapped", "a child pointer repeated", "one AoS box word differs", "record index repeated",
           "hittable record marked -1", "wrong header and leaf flag", "NaN box word"]


@functools.lru_cache(maxsize=None)
def _mutants_once():
    return _mutants()


def test_the_unmutated_tree_passes_and_every_mutant_is_listed():
    p, order, rec, soa, aos = _passing()
    assert not bc.check_tree(order, rec, soa, aos, p)
    assert sorted(_mutants_once()[2]) == sorted(MUTANTS)


@pytest.mark.parametrize("name", MUTANTS)
def test_a_single_mutation_is_reported_under_its_invariant(name):
    p, order, out = _mutants_once()
    (rec, soa, aos), must, may = out[name]
    found = bc.tags(bc.check_tree(order, rec, soa, aos, p))
    assert must <= found, (name, found)
    assert found <= must | may, (name, found)


def test_swapped_pointers_between_two_levels_are_seen_by_the_walk():
    """Two pointers swapped inside one node keep the walk complete (I6 alone sees them); a pointer that leads to another LEVEL does not."""
    p, order, rec, soa, aos = _passing()
    lay = bc.tree_layout(rec.shape[0])
    a = aos.copy()
    a.view(np.int32)[lay.off[3], 6] = lay.off[1] + 9          # a level-3 child that points at a level-1 node: its leaves come twice, others never
    found = bc.tags(bc.check_tree(order, rec, soa, a, p))
    assert {"I6", "I8"} <= found, found


def test_quads_restates_the_hittable_rule_at_its_edges():
    one = np.float32(1.0) / np.float32(255.0)
    op = np.array([one, np.nextafter(one, np.float32(1)), 0.0, 0.99, 1.0, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5], np.float32)
    n = op.shape[0]
    m = np.tile(np.float32([1, 2, 3]), (n, 1)); s = np.full((n, 2), 0.01, np.float32); q = np.tile(np.float32([1, 0, 0, 0]), (n, 1))
    m[5, 0] = np.nan; m[6, 1] = np.inf; s[7, 0] = np.nan; s[8, 1] = 0.0; s[9, 0] = -0.1; q[10] = 0.0
    got = bc.quads64(m, s, q, op)
    assert got.hittable.tolist() == [False, True, False, True, True, False, False, False, False, False, False]
    # just above the threshold the float32 product 255 op is 1 + 2^-23: f = sqrt(2 ln(1 + 2^-23)) + 0.01, not the float64 product's
    assert abs(got.f[1] - (np.sqrt(2 * np.log1p(2.0 ** -23)) + 0.01)) < 1e-12
    assert abs(got.f[4] - (np.sqrt(2 * np.log(255.0)) + 0.01)) < 1e-12
    # corners of an axis-aligned quad: mu +- ex x +- ey y
    e = float(np.float32(0.01)) * got.f[4]
    np.testing.assert_allclose(got.corners[4][:, 0].max() - 1.0, e, rtol=1e-12)
    np.testing.assert_allclose(got.h[4], [e, e, 0.0], atol=1e-15)
