"""The build's own radix sort (lidar_rt_amd/csrc/lrt_radix.inc) tested as a SORT: order, stability and key / value pairing, exactly.

The image and gradient comparisons of tests/test_hip_parity.py cannot see a wrong order (traversal is exhaustive, hits are ordered by
(t, index): a mis-ranked digit or an unstable pass only makes the tree worse), and the comparisons between the tree builders share the sort.
Here every build's sorted order (lrt_debug_read 0) and sorted keys (lrt_debug_read 9) are read back and compared, element for element,
with the host predictor of tests/sort_ref.py (a stable argsort of the sorted bit range) fed with the keys of a rocPRIM build of the
same scene -- k_morton is the same kernel on the same bounds in both builds, so the Morton code is not restated on the host.  The
rocPRIM build itself is checked against the predictor first (the control): a wrongly restated bit range shows there, not on the kernel."""
import functools

import numpy as np
import pytest
import torch

from lidar_rt_amd import _capi, scenes
from lidar_rt_amd.diff_lidar_tracer import Tracer
from tests import sort_ref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tests.hip_util import DEFAULT_OPTS

LEGACY = _capi.has_legacy()
needs_legacy = pytest.mark.skipif(not LEGACY, reason="k_rs_hist (fused_hist = 0) exists in the -DLRT_LEGACY library only (tests/test_legacy_crosscheck_gpu.py)")

# one lane, the wave chunk (1280) and the tile (5120) +- 1, two tiles plus one key, both sides of LRT_BUILD_MERGE_LIMIT, hundreds of tiles
SIZES = [1, 2, 255, 256, 257, 1279, 1280, 1281, 5119, 5120, 5121, 10240, 10241, 40_000, 131_071, 131_072, 300_000]
assert sort_ref.RS_WAVE_CHUNK == 1280 and sort_ref.RS_TILE == 5120 and sort_ref.MERGE_LIMIT == 131_072
EXTRA_DEFAULT = 4                       # the library's morton_extra_bits
EXTRAS = [0, 3, 4, 11, 12]
# (P, morton_extra_bits) of the size cases and of the pass-count cases; the last one is the smallest build that reaches sb = 32 (20 + 12 bits:
# the 32-bit key is sorted from bit 0 on)
PASS_CASES = [(P, e) for P in (5121, 40_000) for e in EXTRAS if e != EXTRA_DEFAULT] + [(300_000, 12), (524_289, 12)]
SIZE_CASES = [(P, EXTRA_DEFAULT) for P in SIZES]
DISTS = ["equal", "corners", "axis", "sorted", "reversed", "dup_runs", "dup_scattered"]
DIST_SIZES = [5121, 40_000]


def test_the_cases_cover_full_and_one_bit_wide_last_passes():
    """sb of every parametrised case: 8, 16, 17, 24, 25 and 32 are reached, so the last 8-bit pass is full in some cases and one bit
    wide in others (and 2 .. 7 bits wide in the rest)."""
    sb = {(P, e): sort_ref.sorted_bits(P, e) for P, e in SIZE_CASES + PASS_CASES}
    assert {8, 16, 17, 24, 25, 32} <= set(sb.values()), sb
    assert any(v % 8 == 0 for v in sb.values()) and any(v % 8 == 1 for v in sb.values())
    assert sb[(1, 4)] == 8 and sb[(5121, 3)] == 16 and sb[(5121, 4)] == 17 and sb[(5121, 11)] == 24 and sb[(5121, 12)] == 25 and sb[(524_289, 12)] == 32
    assert {1, 2, 3, 4} == {(v + 7) // 8 for v in sb.values()}              # one to four passes


# ------------------------------------------------------------------------------------------------------------------ scenes
def _cloud(P, seed=None):
    sc = scenes.make_scene(P, seed=(17 + P) if seed is None else seed, radius_scale=0.5 if P > 100_000 else 0.25)
    return {k: sc[k] for k in ("means", "scales", "rotations", "opacities")}


def _take(sc, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in sc.items()}


@functools.lru_cache(maxsize=None)
def _scene(dist, P):
    """The key distributions, made through the geometry (the Morton grid is laid over the box of the centres)."""
    if dist == "cloud":
        return _cloud(P)
    if dist in ("sorted", "reversed"):          # the cloud in its own sorted order: the input of the sort is sorted already (or the other way round)
        order = _reference("cloud", P, EXTRA_DEFAULT)["val"].astype(np.int64)
        return _take(_cloud(P), order if dist == "sorted" else order[::-1])
    if dist in ("dup_runs", "dup_scattered"):   # every primitive 8 times: tie runs of 8 at consecutive indices, or P / 8 indices apart
        n = (P + 7) // 8
        idx = np.repeat(np.arange(n), 8)[:P] if dist == "dup_runs" else np.tile(np.arange(n), 8)[:P]
        return _take(_cloud(n, seed=23 + P), idx)
    sc = _cloud(P)
    rng = np.random.default_rng(29 + P)
    m = np.empty((P, 3), np.float32)
    if dist == "equal":                         # one cell holds everything
        m[:] = np.array([3.0, -2.0, 1.0], np.float32)
    elif dist == "corners":                     # two tight clusters at opposite corners of the box, in no index order
        far = rng.integers(0, 2, P).astype(bool)
        far[:2] = (False, True)
        m[:] = np.where(far[:, None], 40.0, -40.0) + rng.uniform(-0.004, 0.004, (P, 3))
    elif dist == "axis":                        # the y and z bits of every code are zero
        m[:] = 0.0
        m[:, 0] = rng.uniform(-40.0, 40.0, P)
    else:
        raise ValueError(dist)
    sc["means"] = m
    return sc


# ------------------------------------------------------------------------------------------------------------------ builds
def _read(tr, which, max_bytes):
    """lrt_debug_read: (bytes available, the first min(available, max_bytes) bytes)."""
    import ctypes as C
    st = tr.optix_context
    _, h = st.handle(torch.device("cuda:0"))
    buf = np.zeros(max(max_bytes, 8), np.uint8)
    st._lib.lrt_debug_read.restype = C.c_longlong
    got = int(st._lib.lrt_debug_read(h, which, buf.ctypes.data_as(C.c_void_p), C.c_longlong(max_bytes), None))
    assert got >= 0, (which, got, st._lib.lrt_last_error())
    return got, buf[:min(got, max_bytes)]


def _options(tr, own_sort, key32, extra, **more):
    for k, v in {**DEFAULT_OPTS, "carry_order": 0, "lag_bounds": 0, "own_sort": own_sort, "key32": key32, "morton_extra_bits": extra, **more}.items():
        tr.optix_context.set_option(k, v)


def _build(tr, sc):
    """One build; (sorted keys in the width the build wrote, sorted order)."""
    P = sc["means"].shape[0]
    t = {k: torch.as_tensor(v, device="cuda:0") for k, v in sc.items()}
    tr.build_from_gaussians(t["means"], t["scales"], t["rotations"], t["opacities"])
    torch.cuda.synchronize()
    nv, vals = _read(tr, 0, P * 4)
    nk, keys = _read(tr, 9, P * 8)
    assert nv == P * 4 and nk in (P * 4, P * 8), (P, nv, nk)
    return keys.view(np.uint32 if nk == P * 4 else np.uint64).copy(), vals.view(np.uint32).copy()


def _fresh_build(sc, own_sort, key32, extra, **more):
    tr = Tracer()
    _options(tr, own_sort, key32, extra, **more)
    return _build(tr, sc)


def _by_index(keys, vals):
    out = np.empty_like(keys)
    out[vals.astype(np.int64)] = keys
    return out


def _assert_permutation(vals, P):
    assert vals.shape == (P,)
    np.testing.assert_array_equal(np.sort(vals), np.arange(P, dtype=np.uint32))


@functools.lru_cache(maxsize=None)
def _reference(dist, P, extra):
    """The yardstick: a rocPRIM build (64-bit keys) of the scene on a fresh state, and the control: its order is what the predictor says
    for rocPRIM's bit range.  Computed once per case and shared; nothing changes it afterwards."""
    keys, vals = _fresh_build(_scene(dist, P), 0, 1, extra)
    assert keys.dtype == np.uint64, "rocPRIM builds keep 64-bit keys"
    _assert_permutation(vals, P)
    kbi = _by_index(keys, vals)
    lo, n = sort_ref.bit_range(P, extra, "rocprim")
    np.testing.assert_array_equal(vals, sort_ref.expected_order(kbi, lo, n), err_msg=f"control (rocPRIM against the predictor), bits [{lo}, {lo + n})")
    assert int(kbi.max()) < 1 << 63
    for a in (kbi, vals):
        a.setflags(write=False)
    return {"kbi": kbi, "val": vals}


def _check(dist, P, extra, keys, vals, own, key32):
    """The four exact properties of one build's (keys, vals) against the rocPRIM reference of the same scene."""
    ref = _reference(dist, P, extra)
    assert keys.dtype == (np.uint32 if (own and key32) else np.uint64), (keys.dtype, own, key32)
    _assert_permutation(vals, P)
    # pairing: every key travelled with its own value
    want = (ref["kbi"] >> np.uint64(31)).astype(np.uint32) if keys.dtype == np.uint32 else ref["kbi"]
    np.testing.assert_array_equal(_by_index(keys, vals), want, err_msg="a key left its value")
    # order: sorted on exactly the bit range, ties in index order (the 32-bit key's bits [32 - sb, 32) are the code's [63 - sb, 63))
    lo, n = sort_ref.bit_range(P, extra, "own" if own else "rocprim", 8)
    np.testing.assert_array_equal(vals, sort_ref.expected_order(ref["kbi"], lo, n), err_msg=f"order, bits [{lo}, {lo + n}) of the code")
    if keys.dtype == np.uint32:                 # (and the same through the 32-bit range rule)
        lo32, n32 = sort_ref.bit_range(P, extra, "own", 4)
        np.testing.assert_array_equal(vals, sort_ref.expected_order(want, lo32, n32))


# ------------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("key32", [0, 1])
@pytest.mark.parametrize("P,extra", SIZE_CASES + PASS_CASES, ids=[f"P{P}-extra{e}-sb{sort_ref.sorted_bits(P, e)}" for P, e in SIZE_CASES + PASS_CASES])
def test_own_sort_is_a_stable_sort_of_the_bit_range_and_moves_keys_with_values(P, extra, key32):
    keys, vals = _fresh_build(_scene("cloud", P), 1, key32, extra)
    _check("cloud", P, extra, keys, vals, own=True, key32=key32)


@pytest.mark.parametrize("key32", [0, 1])
@pytest.mark.parametrize("P", [131_071, 131_072])
def test_default_rule_switches_sorts_at_the_merge_limit(P, key32):
    """own_sort = 2: rocPRIM (whole digits, 64-bit keys) below LRT_BUILD_MERGE_LIMIT, the own sort (sb bits, key32 honoured) from it on."""
    own = sort_ref.uses_own_sort(P, 2)
    assert own == (P == 131_072)
    keys, vals = _fresh_build(_scene("cloud", P), 2, key32, EXTRA_DEFAULT)
    _check("cloud", P, EXTRA_DEFAULT, keys, vals, own=own, key32=key32)


@pytest.mark.parametrize("key32", [0, 1])
@pytest.mark.parametrize("P", DIST_SIZES)
@pytest.mark.parametrize("dist", DISTS)
def test_own_sort_on_degenerate_key_distributions(dist, P, key32):
    ref = _reference(dist, P, EXTRA_DEFAULT)
    lo, n = sort_ref.bit_range(P, EXTRA_DEFAULT, "own", 8)
    digits = (ref["kbi"] >> np.uint64(lo)) & np.uint64((1 << n) - 1)
    # the scene is what its name says (seen through the yardstick's keys)
    if dist == "equal":
        assert np.unique(ref["kbi"]).size == 1
    elif dist == "corners":
        assert np.unique(digits).size == 2 and int(digits.min()) == 0 and int(digits.max()) == (1 << n) - 1
    elif dist == "axis":
        assert np.unique(digits).size > min(P, 1 << (n // 3)) // 4
    elif dist == "sorted":
        assert np.all(digits[1:] >= digits[:-1])
    elif dist == "reversed":
        assert np.all(digits[1:] <= digits[:-1]) and digits[0] > digits[-1]
    else:
        assert np.unique(ref["kbi"]).size <= (P + 7) // 8
    keys, vals = _fresh_build(_scene(dist, P), 1, key32, EXTRA_DEFAULT)
    _check(dist, P, EXTRA_DEFAULT, keys, vals, own=True, key32=key32)
    if dist in ("equal", "sorted"):
        np.testing.assert_array_equal(vals, np.arange(P, dtype=np.uint32))


@pytest.mark.parametrize("key32", [0, 1])
@pytest.mark.parametrize("seq", [(300_000, 257, 5121, 300_000, 1, 131_072, 40_000, 40_000), (257, 5121, 40_000, 300_000, 40_000)],
                         ids=["shrinking-first", "growing-first"])
def test_one_state_reused_across_sizes(seq, key32):
    """Epochs, the ticket reset, the zero-on-exit histograms and the growth of the look-back status array: builds of many sizes on ONE
    state (every build sorts: carry_order = 0), each checked like a build on a fresh state; the same size twice at the end."""
    tr = Tracer()
    _options(tr, 1, key32, EXTRA_DEFAULT)
    for step, P in enumerate(seq):
        keys, vals = _build(tr, _scene("cloud", P))
        try:
            _check("cloud", P, EXTRA_DEFAULT, keys, vals, own=True, key32=key32)
        except AssertionError as e:
            raise AssertionError(f"build {step} of {seq} (P = {P}): {e}") from e


def test_sorted_keys_are_refused_after_a_carried_build():
    """lrt_debug_read 9 pairs with the order of the last full sort: after a build that carried the order (no sort ran) it is an error,
    not a stale buffer."""
    P = 5121
    sc = _scene("cloud", P)
    tr = Tracer()
    _options(tr, 1, 1, EXTRA_DEFAULT, carry_order=1)
    t = {k: torch.as_tensor(v, device="cuda:0") for k, v in sc.items()}
    for build in range(2):
        tr.build_from_gaussians(t["means"], t["scales"], t["rotations"], t["opacities"])
        torch.cuda.synchronize()
        import ctypes as C
        st = tr.optix_context
        _, h = st.handle(torch.device("cuda:0"))
        buf = np.zeros(P * 8, np.uint8)
        st._lib.lrt_debug_read.restype = C.c_longlong
        got = int(st._lib.lrt_debug_read(h, 9, buf.ctypes.data_as(C.c_void_p), C.c_longlong(buf.nbytes), None))
        if build == 0:
            assert got == P * 4                                             # the first build of a state sorts
        else:
            assert int(st.get_option("carry_age")) == 1                     # this one carried
            assert got == -3 and b"carried" in st._lib.lrt_last_error(), got     # LRT_ERR_STATE
            assert _read(tr, 0, P * 4)[0] == P * 4                          # the order itself is still there


@needs_legacy
@pytest.mark.parametrize("key32", [0, 1])
@pytest.mark.parametrize("P", SIZES if LEGACY else SIZES[:1])
def test_histogram_launch_of_its_own_gives_the_same_order(P, key32):
    """fused_hist = 0 (k_rs_hist counts the digit histograms in a launch of its own; cross-check library) against fused_hist = 1
    (k_morton counts them on the way): bit-identical keys and order, and both are what the predictor says."""
    sc = _scene("cloud", P)
    fused = _fresh_build(sc, 1, key32, EXTRA_DEFAULT, fused_hist=1)
    own = _fresh_build(sc, 1, key32, EXTRA_DEFAULT, fused_hist=0)
    np.testing.assert_array_equal(own[1], fused[1])
    np.testing.assert_array_equal(own[0], fused[0])
    _check("cloud", P, EXTRA_DEFAULT, own[0], own[1], own=True, key32=key32)
