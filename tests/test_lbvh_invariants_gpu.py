"""The software LBVH itself, read back from the device and checked against what a valid tree IS (tests/bvh_check.py: I1 .. I8).

Every result of the tracer depends on the tree, and nothing else examines it: the image tests see a lost or clipped primitive only when a
ray happens to cross the missing sliver, and a box that is too large, a stale top box or a wrong `empty` flag changes no image at all.  Here the
records (lrt_debug_read 1), the sorted order (0) and BOTH copies of the nodes -- SoA (2), which only the K-buffer fallback reads, and AoS
(10), which the shipped forward walks -- are read back after every kind of build the library has and checked against the float64 quads of the
Gaussians: containment with zero tolerance, tightness to two pads, exact unions above, empties, pointers, equality of the two copies, and a
walk by pointers alone.  Culled builds are also held against a float64 brute force over their ray set: nothing that a ray can hit is left out.
The checker itself is tested without a GPU in tests/test_bvh_check.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from lidar_rt_amd import _capi, scenes
from lidar_rt_amd.diff_lidar_tracer import Tracer, _C
from lidar_rt_amd.parallel import column_slab
from oracle.bruteforce import QuadScene
from tests import bvh_check as bc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tests.hip_util import DEFAULT_OPTS, DEV, settings

KEYS = ("means", "scales", "rotations", "opacities")


# ------------------------------------------------------------------------------------------------------------------ scenes
def _scene(P, seed=None, radius_scale=0.25):
    if P == 0:
        return {"means": np.zeros((0, 3), np.float32), "scales": np.zeros((0, 2), np.float32), "rotations": np.zeros((0, 4), np.float32),
                "opacities": np.zeros((0, 1), np.float32), "shs": np.zeros((0, 16, 3), np.float32)}
    return scenes.make_scene(P, seed=(31 + P) if seed is None else seed, radius_scale=radius_scale)


# kinds of edge rows: (name, can it be hit)
EDGE_KINDS = (("op == 1/255", False), ("op just above 1/255", True), ("op 0", False), ("op 0.99", True), ("op 1", True), ("NaN mean", False),
              ("infinite mean", False), ("NaN scale", False), ("zero scale", False), ("negative scale", False), ("zero quaternion", False),
              ("mean at 1e4 m", True), ("mean at 1e5 m", True), ("aspect 1e4", True), ("aspect 1e-4", True), ("quaternion of norm 1e-3", True),
              ("quaternion of norm 1e3", True))


def _edge_scene(P, seed=7):
    """make_scene(P) with about 2 % of the rows replaced by the edge rows above, in turn; (scene, rows, kind of each row)."""
    sc = _scene(P)
    rng = np.random.default_rng(seed + P)
    rows = rng.choice(P, max(len(EDGE_KINDS), P // 50), replace=False)
    kind = np.arange(rows.shape[0]) % len(EDGE_KINDS)
    one = np.float32(1.0) / np.float32(255.0)
    m, s, q, op = sc["means"], sc["scales"], sc["rotations"], sc["opacities"]
    for g, k in zip(rows, kind):
        if k == 0: op[g] = one
        elif k == 1: op[g] = np.nextafter(one, np.float32(1)); s[g] = np.minimum(s[g], np.float32(0.01))
        elif k == 2: op[g] = 0.0
        elif k == 3: op[g] = 0.99
        elif k == 4: op[g] = 1.0
        elif k == 5: m[g, g % 3] = np.nan
        elif k == 6: m[g, g % 3] = np.inf if g % 2 else -np.inf
        elif k == 7: s[g, g % 2] = np.nan
        elif k == 8: s[g, g % 2] = 0.0
        elif k == 9: s[g, g % 2] = -s[g, g % 2]
        elif k == 10: q[g] = 0.0
        elif k == 11: m[g] = m[g] / np.linalg.norm(m[g]) * np.float32(1e4); s[g] = 1e-4
        elif k == 12: m[g] = m[g] / np.linalg.norm(m[g]) * np.float32(1e5); s[g] = 1e-4
        elif k == 13: s[g] = (1.0, 1e-4)
        elif k == 14: s[g] = (1e-4, 1.0)
        elif k == 15: q[g] = q[g] * np.float32(1e-3)
        elif k == 16: q[g] = q[g] * np.float32(1e3)
    return sc, rows, kind


def _moved(sc, rng, it, step):
    """The drift of tests/test_carried_build_gpu.py: centres by step x it (normal), scales by 1 %, opacities by 0.01, some of them to below 1 / 255."""
    m = dict(sc)
    m["means"] = (sc["means"] + step * it * rng.normal(size=sc["means"].shape)).astype(np.float32)
    m["scales"] = (sc["scales"] * np.exp(0.01 * it * rng.normal(size=sc["scales"].shape))).astype(np.float32)
    m["opacities"] = np.clip(sc["opacities"] + 0.01 * it * rng.normal(size=sc["opacities"].shape), 0.002, 0.99).astype(np.float32)
    return m


# ------------------------------------------------------------------------------------------------------------------ device
def _tracer(**opts):
    tr = Tracer()
    for k, v in {**DEFAULT_OPTS, **opts}.items():
        tr.optix_context.set_option(k, v)
    return tr


def _dev(sc):
    return {k: torch.as_tensor(np.ascontiguousarray(v, np.float32), device=DEV) for k, v in sc.items()}


def _build(tr, t, mod=1.0, cull=None):
    _C.build_from_gaussians(tr.optix_context, t["means"], t["scales"], t["rotations"], t["opacities"], mod, cull_rays=cull)
    torch.cuda.synchronize()


def _forward(tr, t, hw=(8, 64)):
    o, d = scenes.kitti_rays(*hw)
    out, _ = tr(torch.as_tensor(o, device=DEV), torch.as_tensor(d, device=DEV), None, t["means"], torch.zeros_like(t["means"]), shs=t["shs"],
                opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"], tracer_settings=settings(scenes.BG_DEFAULT, 3))
    torch.cuda.synchronize()
    tr.check(DEV)
    return out


def _handle(tr):
    st = tr.optix_context
    return st, st.handle(DEV)[1]


def _size(tr, which):
    st, h = _handle(tr)
    st._lib.lrt_debug_read.restype = C.c_longlong
    n = int(st._lib.lrt_debug_read(h, which, None, C.c_longlong(0), None))
    assert n >= 0, (which, n, st._lib.lrt_last_error())
    return n


def _read(tr, which, dtype=np.float32):
    st, h = _handle(tr)
    n = _size(tr, which)
    buf = np.zeros(max(n, 4), np.uint8)
    got = int(st._lib.lrt_debug_read(h, which, buf.ctypes.data_as(C.c_void_p), C.c_longlong(n), None))
    assert got == n, (which, got, n)
    return buf[:n].view(dtype).copy()


def _tree(tr, culled=False):
    """(order or None, records, SoA nodes, AoS nodes) of the current build."""
    rec = _read(tr, 1).reshape(-1, 16)
    soa, aos = _read(tr, 2).reshape(-1, 64), _read(tr, 10).reshape(-1, 64)
    assert _size(tr, 0) == rec.shape[0] * 4
    return (None if culled else _read(tr, 0, np.uint32)), rec, soa, aos


def _bits(a, name):
    """The words that mean something, as bit patterns: a SoA node has 50 of them (48 box words, first child, leaf flag; the other 14 are never written)."""
    return (a[:, :50] if name == "SoA nodes" else a).view(np.uint32)


def _params(sc):
    return {k: sc[k] for k in KEYS}


def _checked(tr, sc, mod=1.0, culled=False):
    tree = _tree(tr, culled)
    violations = bc.check_tree(*tree, _params(sc), mod)
    assert not violations, "\n".join(violations)
    return tree


# ------------------------------------------------------------------------------------------------------------------ 1. fresh builds
FRESH = [(P, 1.0) for P in (0, 1, 7, 8, 9, 64, 65, 511, 512, 513, 4096, 4097, 32_769, 262_145)] + [(P, m) for P in (513, 4097) for m in (0.5, 2.0)]


@pytest.mark.parametrize("P,mod", FRESH)
def test_fresh_build(P, mod):
    sc = _scene(P)
    tr = _tracer()
    _build(tr, _dev(sc), mod)
    order, rec, soa, aos = _checked(tr, sc, mod)
    lay = bc.tree_layout(P)
    assert rec.shape[0] == P and soa.shape[0] == aos.shape[0] == lay.n_nodes
    if P:
        assert (rec[:, 3] > 0).sum() > 0.8 * P               # the scene can be hit
    if mod != 1.0:                                           # the modifier scales flim and the rows of the record, never the boxes
        tr1 = _tracer()
        _build(tr1, _dev(sc), 1.0)
        _, rec1, soa1, aos1 = _tree(tr1)
        np.testing.assert_array_equal(_bits(soa, "SoA nodes"), _bits(soa1, "SoA nodes"))
        np.testing.assert_array_equal(_bits(aos, "AoS nodes"), _bits(aos1, "AoS nodes"))
        live = rec1[:, 3] > 0
        np.testing.assert_allclose(rec[live, 7] * mod, rec1[live, 7], rtol=3e-7)


@pytest.mark.parametrize("P", [513, 4097, 40_000])
def test_fresh_build_of_the_edge_scene(P):
    sc, rows, kind = _edge_scene(P)
    want = np.array([EDGE_KINDS[k][1] for k in kind])
    q = bc.quads64(**_params(sc))
    assert set(kind.tolist()) == set(range(len(EDGE_KINDS)))
    bad = rows[q.hittable[rows] != want]
    assert bad.size == 0, [(int(g), EDGE_KINDS[kind[list(rows).index(g)]][0]) for g in bad[:5]]      # the restatement calls the rows what they were made to be
    tr = _tracer()
    _build(tr, _dev(sc))
    order, rec, soa, aos = _checked(tr, sc)                   # (I1: the library's hittable set equals the restatement's exactly)
    gi = rec.view(np.int32)[:, 11]
    assert set(gi[rec[:, 3] > 0].tolist()) >= set(rows[want].tolist())


def test_fresh_build_with_a_transparent_tail():
    """The last 1 000 of 40 000 Gaussians transparent: they sort to the end, where whole leaves, level-1 nodes and one whole workgroup of
    k_make_tree (512 slots) hold nothing that can be hit."""
    P = 40_000
    sc = _scene(P)
    sc["opacities"][-1000:] = 0.001
    tr = _tracer()
    _build(tr, _dev(sc))
    order, rec, soa, aos = _checked(tr, sc)
    assert (rec[-1000:, 3] == -1).all() and (rec[:-1000, 3] > 0).all()
    lay = bc.tree_layout(P)
    flag2 = bc.aos_boxes(aos)[3][lay.off[2]:lay.off[2] + lay.cnt[2]]
    # slots 39 000 .. hold nothing to hit: the level-1 nodes 610 .. 624, so the children 2 .. 7 of level-2 node 76 and all of 77 and 78, the
    # slots of k_make_tree's last two workgroups
    assert lay.cnt[2] == 79 and (flag2[77:] == 2).all() and flag2[76].tolist() == [0, 0, 2, 2, 2, 2, 2, 2] and (flag2[:76] == 0).all()


# ------------------------------------------------------------------------------------------------------------------ 2. both finishers
@pytest.mark.parametrize("P", [4097, 40_000])
def test_both_finishers_of_the_top_levels_write_the_same_tree(P):
    """The levels 4 and above are written by k_tree_finish when the tree is read (or built over) before a forward, and by the forward's
    prologue otherwise: the same bits either way, in both copies."""
    sc = _scene(P)
    a, b = _tracer(), _tracer()
    ta, tb = _dev(sc), _dev(sc)
    _build(a, ta)
    tree_a = _tree(a)                                         # read at once: k_tree_finish
    _build(b, tb)
    _forward(b, tb)                                           # the forward's prologue
    tree_b = _checked(b, sc)
    assert bc.tree_layout(P).levels >= 4
    for x, y, name in zip(tree_a, tree_b, ("order", "records", "SoA nodes", "AoS nodes")):
        np.testing.assert_array_equal(_bits(x, name), _bits(y, name), err_msg=name)
    violations = bc.check_tree(*tree_a, _params(sc))
    assert not violations, "\n".join(violations)


# ------------------------------------------------------------------------------------------------------------------ 3. re-armed top
def test_two_builds_in_a_row_re_arm_the_top_boxes():
    """The level-3 boxes are combined by atomic min / max into `top`, which whoever finishes the tree re-arms.  Scene X is 60 m wide, Y 5 m wide
    and 30 m away: a `top` that still held X would leave Y's upper boxes larger than the union of their children (I4)."""
    P = 40_000
    X = _scene(P, radius_scale=0.5)
    Y = dict(X)
    Y["means"] = (X["means"] * np.float32(5.0 / 60.0) + np.float32([30.0, 0.0, 0.0])).astype(np.float32)
    Y["scales"] = (X["scales"] * np.float32(0.1)).astype(np.float32)
    assert np.ptp(X["means"][:, 0]) > 55 and np.ptp(Y["means"][:, 0]) < 5.1 and Y["means"][:, 0].min() > X["means"][:, 0].max() - 5.0
    tx, ty = _dev(X), _dev(Y)
    tr = _tracer()
    _build(tr, tx)
    _checked(tr, X)                                           # (the read finishes the tree)
    _build(tr, tx)
    _build(tr, ty)                                            # at once: nothing between the two builds but finish_tree_now inside the second
    _checked(tr, Y)
    _forward(tr, ty)
    _build(tr, tx)                                            # behind a forward, whose prologue re-armed `top`
    _checked(tr, X)
    _build(tr, ty)
    _forward(tr, ty)
    _checked(tr, Y)                                           # finished by the forward, after a build that followed an unfinished one


# ------------------------------------------------------------------------------------------------------------------ 4. refit
def test_refit_keeps_the_order_and_builds_a_valid_tree_of_the_moved_parameters():
    P = 4097
    sc = _scene(P)
    tr = _tracer()
    _build(tr, _dev(sc))
    order0 = _checked(tr, sc)[0]
    moved = _moved(sc, np.random.default_rng(3), 1, step=0.5)
    assert (moved["opacities"] <= 1 / 255).sum() > 10         # (some of them cannot be hit any more: holes in the order)
    t = _dev(moved)
    st, h = _handle(tr)
    _capi.check(st._lib.lrt_refit(h, P, _capi.ptr(t["means"]), _capi.ptr(t["scales"]), _capi.ptr(t["rotations"]), _capi.ptr(t["opacities"]), 1.0,
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)), "lrt_refit")
    torch.cuda.synchronize()
    order1 = _checked(tr, moved)[0]
    np.testing.assert_array_equal(order0, order1)
    stale = bc.check_tree(*_tree(tr), _params(sc))            # the control: against the parameters before the move the same tree fails
    assert {"I1", "I2"} <= bc.tags(stale)


# ------------------------------------------------------------------------------------------------------------------ 5. carried builds
def test_carried_builds_with_holes_in_the_order():
    P = 40_000
    sc = _scene(P)
    tr = _tracer(carry_order=1, carry_max_age=1000)
    rng = np.random.default_rng(4)
    order0 = None
    for it in range(3):
        m = _moved(sc, rng, it, step=2e-3)
        if it == 2:                                           # 500 Gaussians, anywhere in the order, become transparent; 50 of them lose their centre as well
            gone = rng.choice(P, 500, replace=False)
            m["opacities"][gone] = 0.001
            m["means"][gone[:50]] = np.nan
        _build(tr, _dev(m))
        assert tr.optix_context.get_option("carry_age", DEV) == it
        order, rec, _, _ = _checked(tr, m)
        if it == 0:
            order0 = order
        np.testing.assert_array_equal(order, order0)          # carried: the order of the one sort
    holes = np.nonzero(rec[:, 3] == -1)[0]
    assert holes.size >= 500 and np.median(holes) < 0.9 * P   # in the middle of the order, not at its end


# ------------------------------------------------------------------------------------------------------------------ 6. outside the lagged box
@pytest.mark.parametrize("carry", [0, 1])
def test_a_scene_that_has_left_the_lagged_morton_box(carry):
    """lag_bounds (default): the Morton grid of a build lies over the box of the previous build's centres.  A scene 500 m away from it falls into
    one corner cell (every code clamped) -- or keeps the old order --: the grid only shapes the tree, which stays valid."""
    P = 4097
    X = _scene(P)
    far = dict(X)
    far["means"] = (X["means"] + np.float32([500.0, 0.0, 0.0])).astype(np.float32)
    tr = _tracer(carry_order=carry, lag_bounds=1)
    _build(tr, _dev(X))
    _checked(tr, X)
    _build(tr, _dev(far))
    assert tr.optix_context.get_option("carry_age", DEV) == carry
    _checked(tr, far)


# ------------------------------------------------------------------------------------------------------------------ 7. culled builds
CULL_P, CULL_HW, N_PLANT = 24_000, (8, 512), 96
SLABS = ((8, 3), (4, 0), (2, 1))


def _planted(o, d, cols, rows_, rng):
    """Small opaque Gaussians (scale 0.02, opacity 0.8) centred on the rays (rows_[i], cols[i]) at 5 .. 40 m, facing the sensor."""
    n = len(cols)
    dirs = d[rows_, cols].astype(np.float64)
    rng_ = rng.uniform(5.0, 40.0, n)
    means = o[rows_, cols].astype(np.float64) + rng_[:, None] * dirs
    rot = scenes._frame_quaternions(-dirs, rng.uniform(0, 2 * np.pi, n))
    return {"means": means.astype(np.float32), "scales": np.full((n, 2), 0.02, np.float32), "rotations": rot.astype(np.float32),
            "opacities": np.full((n, 1), 0.8, np.float32)}


def reach(sc, o, d, chunk=512):
    """Float64 brute force: the Gaussians that at least one of the rays hits (t > 0, |u| <= flim, |v| <= flim: QuadScene.candidates)."""
    qs = QuadScene(sc["means"], sc["scales"], sc["rotations"], sc["opacities"])
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    out = np.zeros(qs.mu.shape[0], bool)
    with np.errstate(all="ignore"):
        n_mu, u_mu, v_mu = (qs.n * qs.mu).sum(1), (qs.U * qs.mu).sum(1), (qs.V * qs.mu).sum(1)
        for a in range(0, o.shape[0], chunk):
            oc, dc = o[a:a + chunk], d[a:a + chunk]
            t = (n_mu - oc @ qs.n.T) / (dc @ qs.n.T)
            hit = (t > 0) & np.isfinite(t)
            u = oc @ qs.U.T + t * (dc @ qs.U.T) - u_mu
            hit &= np.abs(u) <= qs.flim
            u = oc @ qs.V.T + t * (dc @ qs.V.T) - v_mu
            hit &= np.abs(u) <= qs.flim
            out |= hit.any(0)
    return out


@functools.lru_cache(maxsize=None)
def _cull_case(n_slabs, r):
    """Scene, slab rays and the brute force's verdicts for the scene and for its drifted version; computed once per slab, never changed."""
    H, W = CULL_HW
    o, d = scenes.kitti_rays(H, W)
    a, b = column_slab(W, r, n_slabs)
    rng = np.random.default_rng(100 * n_slabs + r)
    q = N_PLANT // 4
    edge_cols = np.concatenate([np.full(q, a), np.full(q, b - 1), rng.integers(a, b, 2 * q)])
    edge_rows = np.concatenate([rng.integers(0, H, 2 * q), np.zeros(q, np.int64), np.full(q, H - 1)])
    out_cols = np.concatenate([np.full(N_PLANT // 2, (a - 1) % W), np.full(N_PLANT // 2, b % W)])
    out_rows = rng.integers(0, H, N_PLANT)
    base = _scene(CULL_P - 2 * N_PLANT, seed=41, radius_scale=0.3)
    parts = [{k: base[k] for k in KEYS}, _planted(o, d, edge_cols, edge_rows, rng), _planted(o, d, out_cols, out_rows, rng)]
    sc = {k: np.ascontiguousarray(np.concatenate([p[k] for p in parts], 0)) for k in KEYS}
    os_, ds_ = np.ascontiguousarray(o[:, a:b]), np.ascontiguousarray(d[:, a:b])
    edge = np.zeros(os_.shape[:2], bool)
    edge[0] = edge[-1] = True
    edge[:, 0] = edge[:, -1] = True
    drifted = _moved(sc, np.random.default_rng(5), 1, step=2e-3)
    res = {"scene": sc, "drifted": drifted, "o": os_, "d": ds_}
    for name, s_ in (("scene", sc), ("drifted", drifted)):
        by_edge, by_inner = reach(s_, os_[edge], ds_[edge]), reach(s_, os_[~edge], ds_[~edge])
        res["reach_" + name] = by_edge | by_inner
        res["edge_only_" + name] = by_edge & ~by_inner
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


@pytest.mark.parametrize("form", ["slab", "rays"])
@pytest.mark.parametrize("n_slabs,r", SLABS)
def test_culled_builds_keep_everything_a_ray_can_hit(n_slabs, r, form):
    """lrt_build_for_slab (cone and wedge) and lrt_build_for_rays (cone alone) on an azimuth slab: a valid tree over a subset that holds every
    Gaussian the float64 brute force finds hit by a ray of the set -- the planted ones on the slab's first and last column and top and bottom
    row included --, then the carried, speculatively sized build on the stale index with drifted parameters."""
    case = _cull_case(n_slabs, r)
    P = CULL_P
    ro, rd = torch.as_tensor(np.array(case["o"]), device=DEV), torch.as_tensor(np.array(case["d"]), device=DEV)
    cull = (ro, rd) if form == "slab" else (ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous())
    tr = _tracer()
    slots, cone_useless = [], form == "rays" and n_slabs == 2      # the cone around a 180-degree set of rays culls nothing (the wedge is what culls there)
    for step, name in enumerate(("scene", "drifted")):
        sc, can, edge_only = case[name], case["reach_" + name], case["edge_only_" + name]
        # what keeps the case honest: enough Gaussians that only edge rays reach
        assert edge_only.sum() >= 64, edge_only.sum()
        _build(tr, _dev(sc), cull=cull)
        assert tr.optix_context.get_option("carry_age", DEV) == step
        _, rec, soa, aos = _checked(tr, sc, culled=True)
        slots.append(rec.shape[0])
        live = rec[:, 3] > 0
        kept = np.zeros(P, bool)
        kept[rec.view(np.int32)[live, 11]] = True
        lost = np.nonzero(can & ~kept)[0]
        print(f"culled build {form} {n_slabs}/{r} {name}: slots {rec.shape[0]}, reachable {can.sum()}, edge-only {edge_only.sum()}, kept {kept.sum()}, left out {P - kept.sum()}, "
              f"depth {bc.tree_layout(rec.shape[0]).levels}, nodes {soa.shape[0]}")
        assert lost.size == 0, f"{lost.size} Gaussians that a ray of the set hits are not in the build: {lost[:8]} (edge-only among them: {(edge_only[lost]).sum()})"
        assert tr.optix_context.built_count(DEV) == live.sum() == kept.sum()
        if n_slabs == 8:
            assert P - kept.sum() >= 0.3 * P, kept.sum()
        if step == 1 and not cone_useless:
            # the speculative size, 1.25 x the slots of the build before + 4096: larger than that build, smaller than everything, its tail padding
            assert slots[0] < slots[1] < P, slots
            used = tr.optix_context.get_option("cull_last", DEV)
            assert 0 < used < slots[1], (used, slots)
            assert bc.padding_slots(rec)[used:].all()
            lay = bc.tree_layout(slots[1])
            flag1 = bc.aos_boxes(aos)[3][lay.off[1]:lay.off[1] + lay.cnt[1]].reshape(-1)
            assert (flag1[(used + 7) // 8:] == 2).all()
    if cone_useless:
        assert slots[0] == slots[1] >= P, slots


# ------------------------------------------------------------------------------------------------------------------ 8. more than 256 level-4 nodes
def test_a_tree_with_more_than_256_level_4_nodes():
    """P = 8 388 609, the smallest tree whose levels above 4 tree_finish_top walks through global memory instead of LDS.  The parameters are
    made on the device; only the nodes come back (38 MB per copy).  The levels 1 .. 3 are written per workgroup exactly as in the small cases,
    so level 1 is taken as it is and the levels from 2 on are checked against it: I4 .. I8."""
    P = 8_388_609
    g = torch.Generator(device=DEV)
    g.manual_seed(11)
    means = torch.rand((P, 3), device=DEV, generator=g) * 200.0 - 100.0
    scales = torch.rand((P, 2), device=DEV, generator=g) * 0.1 + 0.02
    rots = torch.nn.functional.normalize(torch.randn((P, 4), device=DEV, generator=g), dim=1)
    opac = torch.rand((P, 1), device=DEV, generator=g) * 0.9 + 0.05
    tr = _tracer()
    _build(tr, {"means": means, "scales": scales, "rotations": rots, "opacities": opac})
    lay = bc.tree_layout(P)
    assert lay.cnt[4] == 257 and lay.levels == 7 and lay.n_nodes == 149_803
    soa, aos = _read(tr, 2).reshape(-1, 64), _read(tr, 10).reshape(-1, 64)
    violations = bc.check_nodes(soa, aos, P, None, from_level=2)
    assert not violations, "\n".join(violations)
    slo, shi = bc.soa_boxes(soa)
    live1 = (slo[lay.off[1]:, :, 0] < 1e29).reshape(-1)
    assert live1[:lay.leaves].all() and not live1[lay.leaves:].any()          # every leaf holds something (opacity >= 0.05), the 7 child slots past the last leaf nothing
    lo, hi = means.min(0).values.cpu().numpy(), means.max(0).values.cpu().numpy()
    root_live = slo[0, :, 0] < 1e29
    assert root_live.sum() == lay.cnt[lay.levels - 1]
    assert (slo[0][root_live].min(0) <= lo).all() and (shi[0][root_live].max(0) >= hi).all()
    assert (slo[0][root_live].min(0) >= lo - 1.0).all() and (shi[0][root_live].max(0) <= hi + 1.0).all()      # (quads of at most 0.12 x 3.4 m half size)
