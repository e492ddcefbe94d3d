"""GPU: the two kernels of the gathering gradient exchange (k_xchg_pack / k_xchg_apply behind lrt_xchg_pack / lrt_xchg_apply, include/lrt.h)
against the host predictors of tests/exchange_ref.py: the message as a data structure, rows wider than 64 floats, what an overflow leaves
behind, the order of the additions, the order the blocks land in, the edges of the index space and of the mask, repeated use, the refusals.
Every comparison is on float32 bit patterns.  tests/test_exchange_ref.py tests the predictors themselves without a GPU."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from lidar_rt_amd import _capi
from lidar_rt_amd.parallel import GradLayout
from tests import exchange_ref as xr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = np.float32
SENT = int(xr.SENTINEL)
LRT_ERR_ARG = -1
NAMES = ("means", "scales", "rotations", "opacities", "shs")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dense(lay):
    v = lay.views
    return [_capi.ptr(v[k]) for k in NAMES + ("accum",)]


def _lay_of(rows, P, M):
    """A GradLayout on the device holding the [P, 11 + 3M] float32 row matrix `rows`."""
    fields, accum = xr.fields_of(np.ascontiguousarray(rows, dtype=F32).view(np.int32), P, M)
    lay = GradLayout(P, M, DEV)
    for k in NAMES:
        lay.views[k].copy_(torch.from_numpy(fields[k]).reshape(lay.views[k].shape))
    lay.views["accum"].copy_(torch.from_numpy(accum))
    return lay


def _clone(lay):
    out = GradLayout(lay.P, lay.M, DEV)
    out.flat.copy_(lay.flat)
    return out


def _bits(lay):
    """[P, 11 + 3M] int32: the row bits of a device layout."""
    v = {k: t.cpu().numpy() for k, t in lay.views.items()}
    return xr.rows_of(v, v["accum"], lay.P, lay.M)


def _bufs(rows, P, M):
    return xr.fields_of(np.ascontiguousarray(rows, dtype=F32).view(np.int32), P, M)


def _ref_bits(bufs, P, M):
    return xr.rows_of(bufs[0], bufs[1], P, M)


@functools.lru_cache(maxsize=2)
def _scene(P, M):
    """Random rows for ALL P Gaussians (host matrix, device layout): a row taken from the wrong Gaussian is then a visible mistake."""
    rows = np.random.default_rng(1000 * M + P).standard_normal((P, xr.width(M)), dtype=F32)
    return rows, _lay_of(rows, P, M)


def _pack(lib, P, M, cap, lay, accum_t, with_rows, counters, parity):
    """One lrt_xchg_pack into a sentinel-filled message with a sentinel guard behind it."""
    words = int(lib.lrt_xchg_msg_words(P, M, cap, with_rows))
    assert words == xr.msg_words(P, M, cap, with_rows)
    msg = torch.full((words + xr.GUARD,), SENT, dtype=torch.int32, device=DEV)
    d = _dense(lay)
    _capi.check(lib.lrt_xchg_pack(0, P, M, cap, *d[:5], _capi.ptr(accum_t), _capi.ptr(msg), _capi.ptr(counters), parity, with_rows, _stream()), "lrt_xchg_pack")
    return msg


def _apply(lib, P, M, N, rank, cap, msgs, lay, status, zero_only):
    _capi.check(lib.lrt_xchg_apply(0, P, M, N, rank, cap, _capi.ptr(msgs), C.c_longlong(msgs.shape[1]), *_dense(lay),
                                   _capi.ptr(status) if status is not None else None, zero_only, _stream()), "lrt_xchg_apply")


def _pack_ranks(lib, P, M, cap, lays, rows, check=True):
    """Pack every rank's buffer on one counter pair: ([N, words + GUARD] device messages, the same on the host, the landing orders)."""
    N = len(lays)
    counters = torch.zeros(2, dtype=torch.int32, device=DEV)
    msgs = torch.stack([_pack(lib, P, M, cap, lays[r], lays[r].views["accum"], 1, counters, r & 1) for r in range(N)])
    host = msgs.cpu().numpy()
    orders = [xr.check_message(host[r], P, M, cap, 1, *_bufs(rows[r], P, M)) for r in range(N)] if check else None
    return msgs, host, orders


def _lists(host, P, M, cap):
    """The messages without their guard, as apply_ref wants them."""
    return [m[:xr.msg_words(P, M, cap, 1)] for m in host]


# ---- pack against check_message ------------------------------------------------------------------------------------------------------------
SIZES = (1, 17, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 70_001)
PACK_SHAPES = [(P, 16) for P in SIZES] + [(P, M) for P in (1025, 4097) for M in (1, 17, 18, 25, 39, 40)] + [(70_001, 40)]


def _masks(P):
    rng = np.random.default_rng(P)
    B = xr.n_blocks(P)
    ar = np.arange(P)
    b = min(1, B - 1)
    borders = np.array([g for g in (63, 64, 255, 256, 1023, 1024, 4095, 4096) if g < P], dtype=np.int64)
    return {"none": np.zeros(P, bool), "all": np.ones(P, bool), "first": ar == 0, "last": ar == P - 1, "borders": np.isin(ar, borders),
            "one_block": ar // xr.XB_G == b, "every_second": ar % 2 == 0, "random": rng.random(P) < 0.1}


def _accum_of(mask, seed):
    return np.where(mask, np.random.default_rng(seed).random(mask.size) + 0.1, 0.0).astype(F32)


@pytest.mark.parametrize("with_rows", [1, 0])
@pytest.mark.parametrize("P,M", PACK_SHAPES)
def test_pack_writes_a_valid_message_and_nothing_else(P, M, with_rows):
    lib = _capi.load()
    rows, lay = _scene(P, M)
    fields, _ = _bufs(rows, P, M)
    counters = torch.zeros(2, dtype=torch.int32, device=DEV)
    par = 0
    for name, mask in _masks(P).items():
        accum = _accum_of(mask, P + len(name))
        count = int(mask.sum())
        cap = P if name == "all" else count + 5                              # slack: idx and row words no entry owns must stay sentinels
        msg = _pack(lib, P, M, cap, lay, torch.from_numpy(accum).to(DEV), with_rows, counters, par)
        order = xr.check_message(msg.cpu().numpy(), P, M, cap, with_rows, fields, accum)
        live = np.unique(np.flatnonzero(mask) // xr.XB_G).tolist()
        assert sorted(order) == live, name
        c = counters.cpu().tolist()
        assert c[par] == count and c[par ^ 1] == 0, (name, c)                # this call's word holds the list length, the other is re-armed
        par ^= 1


def test_the_mask_rule_is_accum_greater_than_zero():
    lib = _capi.load()
    P, M = 4097, 1
    rows, lay = _scene(P, M)
    vals = np.array([np.nan, -0.0, 0.0, -1.0, np.inf, 1e-45, 1e-38], dtype=F32)      # 1e-45: the smallest subnormal; 1e-38 is subnormal too
    accum = vals[np.arange(P) % 7]                                                    # every value at every kind of border
    acc_t = torch.from_numpy(accum).to(DEV)
    cap = P
    counters = torch.zeros(2, dtype=torch.int32, device=DEV)
    msg = _pack(lib, P, M, cap, lay, acc_t, 1, counters, 0).cpu().numpy()
    off, n, idx, _ = xr.split(msg, P, M, cap, 1)
    got = np.sort(np.concatenate([idx[off[b]:off[b] + n[b]] for b in range(xr.n_blocks(P))]))
    dev_rule = torch.nonzero(acc_t > 0).squeeze(1).cpu().numpy()                      # what _exchange_lists sizes the capacity with: the contract
    assert np.array_equal(got, dev_rule)
    assert np.array_equal(got, np.flatnonzero(xr.touched(accum)))                     # and IEEE on the host says the same, subnormals included
    assert np.array_equal(got, np.flatnonzero(np.isin(np.arange(P) % 7, (4, 5, 6))))
    xr.check_message(msg, P, M, cap, 1, _bufs(rows, P, M)[0], accum)


@pytest.mark.parametrize("with_rows", [1, 0])
@pytest.mark.parametrize("P", [8193, 70_001])
def test_pack_beyond_the_capacity_writes_the_entries_that_fit_and_nothing_else(P, with_rows):
    lib = _capi.load()
    M = 16
    rows, lay = _scene(P, M)
    fields, _ = _bufs(rows, P, M)
    counters = torch.zeros(2, dtype=torch.int32, device=DEV)
    par = 0
    masks = _masks(P)
    for name in ("random", "every_second"):
        accum = _accum_of(masks[name], 3)
        count = int(masks[name].sum())
        for cap in (count // 2, 1):
            msg = _pack(lib, P, M, cap, lay, torch.from_numpy(accum).to(DEV), with_rows, counters, par).cpu().numpy()
            order = xr.check_message(msg, P, M, cap, with_rows, fields, accum)
            assert sorted(order) == np.unique(np.flatnonzero(masks[name]) // xr.XB_G).tolist()       # a permutation of the non-empty blocks
            assert xr.overflowed_blocks([msg[:-xr.GUARD]], P, M, cap, with_rows).any()
            assert counters.cpu().tolist()[par] == count                     # the counter runs on past the capacity: the true length
            par ^= 1


def test_sixty_four_packs_on_one_counter_pair():
    lib = _capi.load()
    P, M = 4097, 1
    rows, lay = _scene(P, M)
    fields, _ = _bufs(rows, P, M)
    rng = np.random.default_rng(64)
    counters = torch.zeros(2, dtype=torch.int32, device=DEV)
    fracs = (0.5, 0.01, 1.0, 0.1, 0.0, 0.9, 0.002)
    for i in range(64):
        frac = 0.0 if i == 32 else fracs[i % len(fracs)]                      # empty lists among them, one in the middle
        mask = rng.random(P) < frac
        accum = _accum_of(mask, i)
        count = int(mask.sum())
        cap = count + 2
        with_rows = 0 if i % 5 == 4 else 1
        msg = _pack(lib, P, M, cap, lay, torch.from_numpy(accum).to(DEV), with_rows, counters, i & 1)
        xr.check_message(msg.cpu().numpy(), P, M, cap, with_rows, fields, accum)
        c = counters.cpu().tolist()
        assert c[i & 1] == count and c[(i & 1) ^ 1] == 0, (i, c)
    assert counters.cpu().tolist() == [0, count]                              # after call 63 (parity 1): its length, and word 0 armed for call 64


# ---- apply from real packs against apply_ref -----------------------------------------------------------------------------------------------
def _make_ranks(P, M, N, seed, frac0=0.1, frac=0.1, carry=0.3, forced=True):
    """N partial buffers as row matrices: zero except the touched rows; neighbouring ranks overlap.  `forced`: some Gaussians are in all N
    lists and every rank has some that are in its list alone."""
    rng = np.random.default_rng(seed)
    masks = []
    for r in range(N):
        m = rng.random(P) < (frac0 if r == 0 else frac)
        if r > 0:
            m |= masks[r - 1] & (rng.random(P) < carry)
        masks.append(m)
    masks = np.array(masks)
    shared = alone = None
    if forced:
        pool = rng.permutation(P)
        n_all, n_ex = max(1, P // 50), max(1, P // 100)
        shared = pool[:n_all]
        alone = [pool[n_all + r * n_ex:n_all + (r + 1) * n_ex] for r in range(N)]
        masks[:, shared] = True
        for r in range(N):
            masks[:, alone[r]] = False
            masks[r, alone[r]] = True
    rows = []
    for r in range(N):
        x = np.where(masks[r][:, None], rng.standard_normal((P, xr.width(M)), dtype=F32), F32(0))
        x[:, -1] = np.where(masks[r], np.abs(x[:, -1]) + F32(0.1), F32(0))
        if forced:
            x[np.flatnonzero(masks[r])[::7], 3] = F32(-0.0)                   # 0 + (-0.0) = +0.0 in the kernel and in the predictor alike
        rows.append(x.astype(F32))
    return masks, rows, shared, alone


@pytest.mark.parametrize("P,M,N", [(17, 1, 2), (1025, 18, 3), (4097, 39, 4), (4097, 40, 8), (8193, 16, 1), (70_001, 25, 4)])
def test_apply_from_real_packs_gives_the_predictors_bits_on_every_replica(P, M, N):
    lib = _capi.load()
    masks, rows, shared, alone = _make_ranks(P, M, N, seed=P + N)
    assert masks[:, shared].all() and all(masks[:, alone[r]].sum() == alone[r].size and alone[r].size > 0 for r in range(N))
    counts = [int(m.sum()) for m in masks]
    cap = max(counts) + 3
    lays = [_lay_of(rows[r], P, M) for r in range(N)]
    msgs, host, _ = _pack_ranks(lib, P, M, cap, lays, rows)
    lists = _lists(host, P, M, cap)
    first = None
    for r in range(N):                                                       # apply on every rank
        lay = _clone(lays[r])
        status = torch.zeros(1 + N, dtype=torch.int32, device=DEV)
        _apply(lib, P, M, N, r, cap, msgs, lay, status, 0)
        want, st = xr.apply_ref(_bufs(rows[r], P, M), lists, P, M, N, r, cap, 0)
        assert st.tolist() == [0] + counts
        assert status.cpu().tolist() == st.tolist(), r
        got = _bits(lay)
        assert np.array_equal(got, _ref_bits(want, P, M)), r                  # the predictor's bits
        first = got if first is None else first
        assert np.array_equal(got, first), r                                  # and all replicas equal one another
    lay = _clone(lays[N - 1])                                                # status = NULL: the same sums
    _apply(lib, P, M, N, N - 1, cap, msgs, lay, None, 0)
    assert np.array_equal(_bits(lay), first)
    # zero_only over the N lists, on a buffer that is non-zero everywhere: exactly the rows of the lists are cleared
    full, flay = _scene(P, M)
    lay = _clone(flay)
    status = torch.zeros(1 + N, dtype=torch.int32, device=DEV)
    _apply(lib, P, M, N, 0, cap, msgs, lay, status, 1)
    want, st = xr.apply_ref(_bufs(full, P, M), lists, P, M, N, 0, cap, 1)
    got = _bits(lay)
    assert np.array_equal(got, _ref_bits(want, P, M))
    union = masks.any(axis=0)
    assert not got[union].any() and np.array_equal(got[~union], full.view(np.int32)[~union])
    assert status.cpu().tolist() == st.tolist() == [0] * (1 + N)


# ---- order ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_lists_are_added_in_rank_order(rot):
    """Column 0 of one Gaussian holds 1e8, 1, -1e8, 1 on ranks 0..3: rank order gives exactly 1.0, the reverse 0.0
    (tests/test_exchange_ref.py); the rotated arrangements take their value from the predictor."""
    lib = _capi.load()
    P, M, N, g = 2049, 1, 4, 1500
    vals = np.roll(np.array([1e8, 1.0, -1e8, 1.0], dtype=F32), rot)
    masks, rows, _, _ = _make_ranks(P, M, N, seed=5, forced=False)
    for r in range(N):
        if not masks[r, g]:
            rows[r][g] = np.random.default_rng(r).standard_normal(xr.width(M)).astype(F32)
            rows[r][g, -1] = 0.5
        rows[r][g, 0] = vals[r]
    cap = max(int((x[:, -1] > 0).sum()) for x in rows) + 1
    lays = [_lay_of(rows[r], P, M) for r in range(N)]
    msgs, host, _ = _pack_ranks(lib, P, M, cap, lays, rows)
    lists = _lists(host, P, M, cap)
    for r in range(N):
        lay = _clone(lays[r])
        _apply(lib, P, M, N, r, cap, msgs, lay, None, 0)
        want, _ = xr.apply_ref(_bufs(rows[r], P, M), lists, P, M, N, r, cap, 0)
        got = _bits(lay)
        assert np.array_equal(got, _ref_bits(want, P, M)), r
        if rot == 0:
            assert got[g, 0] == np.array(1.0, dtype=F32).view(np.int32), got[g, 0].view(F32)
    want_rev, _ = xr.apply_ref(_bufs(rows[N - 1], P, M), lists[::-1], P, M, N, 0, cap, 0)
    if rot == 0:
        assert want_rev[0]["means"][g, 0] == 0.0                              # the case can see a reversed order


@pytest.mark.parametrize("M", [1, 18])
def test_a_gaussian_that_ends_one_list_and_opens_the_next_gets_both_addends(M):
    """The barrier between lists, shown a schedule that needs it.  Entry k of a block belongs to wave k % 4, and a list of 16 j + 1 entries
    gives wave 0 one trip more than the others.  In every block here one list has 16 j + 1 entries, the last of them Gaussian g, and the
    other list holds g as its entry 1, 2 or 3: the wave that takes g there is idle while wave 0 still works on g.  Even blocks: list 0 is
    the long one (add, then add); odd blocks: list 1 (on rank 1 its clear of g, then list 0's add)."""
    lib = _capi.load()
    N, js = 2, (1, 2, 3, 5, 8, 16, 31, 63)
    P = len(js) * xr.XB_G
    rng = np.random.default_rng(M)
    masks = np.zeros((N, P), bool)
    meet = []
    for b, j in enumerate(js):
        long_, short = (0, 1) if b % 2 == 0 else (1, 0)
        base = b * xr.XB_G
        g = base + 16 * j
        masks[long_, base:g + 1] = True                                       # 16 j + 1 entries, g the last
        pos = 1 + b % 3
        masks[short, g - pos:g + 2] = True                                     # g is entry `pos`; one more behind it
        meet.append(g)
    rows = []
    for r in range(N):
        x = np.where(masks[r][:, None], rng.standard_normal((P, xr.width(M)), dtype=F32), F32(0))
        x[:, -1] = np.where(masks[r], F32(0.5), F32(0))
        rows.append(x.astype(F32))
    cap = int(masks.sum(axis=1).max())
    lays = [_lay_of(rows[r], P, M) for r in range(N)]
    msgs, host, _ = _pack_ranks(lib, P, M, cap, lays, rows)
    lists = _lists(host, P, M, cap)
    for m in lists:                                                           # the schedule above is what the messages hold
        off, n, idx, _ = xr.split(m, P, M, cap, 1)
        assert all(int(n[b]) == 16 * j + 1 and idx[off[b] + n[b] - 1] == meet[b] or idx[off[b] + 1 + b % 3] == meet[b] for b, j in enumerate(js))
    for r in range(N):
        want, _ = xr.apply_ref(_bufs(rows[r], P, M), lists, P, M, N, r, cap, 0)
        want = _ref_bits(want, P, M)
        assert np.array_equal(want[meet].view(F32), rows[0][meet] + rows[1][meet])
        for _ in range(4):                                                    # a few launches: each is a fresh draw of the waves' timing
            lay = _clone(lays[r])
            _apply(lib, P, M, N, r, cap, msgs, lay, None, 0)
            got = _bits(lay)
            bad = [g for g in meet if not np.array_equal(got[g], want[g])]
            assert not bad, (r, bad)
            assert np.array_equal(got, want), r


# ---- overflow ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,M,N", [(8193, 18, 2), (70_001, 16, 3)])
def test_an_overflow_skips_its_blocks_and_sums_the_others(P, M, N):
    """cap = half of rank 0's list.  The other lists are shorter than that capacity, so whatever order rank 0's blocks land in, the
    workgroup that lands first has its blocks fitted and a later one has not: both kinds of block exist (asserted from the header)."""
    lib = _capi.load()
    masks, rows, _, _ = _make_ranks(P, M, N, seed=P, frac0=0.2, frac=0.03, carry=0.1, forced=False)
    counts = [int(m.sum()) for m in masks]
    cap = counts[0] // 2
    assert max(counts[1:]) <= cap
    lays = [_lay_of(rows[r], P, M) for r in range(N)]
    msgs, host, _ = _pack_ranks(lib, P, M, cap, lays, rows)
    lists = _lists(host, P, M, cap)
    ovf = xr.overflowed_blocks(lists, P, M, cap, 1)
    blk = np.arange(P) // xr.XB_G
    live = np.zeros(xr.n_blocks(P), bool)
    live[np.unique(blk[masks.any(axis=0)])] = True
    assert (ovf & live).any() and (~ovf & live).any()                        # or this test could hide a failure
    row_ovf = ovf[blk]
    zero = np.zeros_like(rows[0])
    plain = functools.reduce(lambda a, b: a + b, rows, zero)                 # ((0 + rank 0) + rank 1) + ..: rows hold no -0.0 here, adding +0.0 changes no bit
    fitted = np.zeros(P, bool)                                               # the Gaussians of the entries the messages hold
    for m in lists:
        off, n, idx, _ = xr.split(m, P, M, cap, 1)
        for b in range(xr.n_blocks(P)):
            fit = 0 if off[b] >= cap else min(int(n[b]), cap - int(off[b]))
            fitted[idx[off[b]:off[b] + fit]] = True
    assert fitted.any() and (masks.any(axis=0) & ~fitted).any()
    for r in range(N):                                                       # the applying rank's buffer holds its own partial rows
        lay = _clone(lays[r])
        status = torch.zeros(1 + N, dtype=torch.int32, device=DEV)
        _apply(lib, P, M, N, r, cap, msgs, lay, status, 0)
        got = _bits(lay)
        before = rows[r].view(np.int32)
        assert np.array_equal(got[row_ovf], before[row_ovf]), r               # the skipped blocks: bit for bit what they were
        assert np.array_equal(got[~row_ovf], plain.view(np.int32)[~row_ovf]), r   # every other block: the rank-ordered sum
        want, st = xr.apply_ref(_bufs(rows[r], P, M), lists, P, M, N, r, cap, 0)
        assert np.array_equal(got, _ref_bits(want, P, M)), r
        assert status.cpu().tolist() == st.tolist() == [1] + counts          # flagged, and the true lengths
        # then zero_only with the same messages, as the next step would: the fitted entries are zero, nothing else changed
        status = torch.zeros(1 + N, dtype=torch.int32, device=DEV)
        _apply(lib, P, M, N, r, cap, msgs, lay, status, 1)
        got2 = _bits(lay)
        want2, st2 = xr.apply_ref(want, lists, P, M, N, r, cap, 1)
        assert np.array_equal(got2, _ref_bits(want2, P, M)), r
        assert not got2[fitted].any() and np.array_equal(got2[~fitted], got[~fitted]), r
        assert status.cpu().tolist() == st2.tolist() == [1] + [0] * N
    full, flay = _scene(P, M)                                                 # the same on a buffer that is non-zero everywhere
    lay = _clone(flay)
    _apply(lib, P, M, N, 0, cap, msgs, lay, None, 1)
    got = _bits(lay)
    assert not got[fitted].any() and np.array_equal(got[~fitted], full.view(np.int32)[~fitted])


# ---- block arrival order -------------------------------------------------------------------------------------------------------------------
def test_apply_does_not_care_in_which_order_the_blocks_landed():
    lib = _capi.load()
    P, M, N = 4097, 18, 3
    masks, rows, _, _ = _make_ranks(P, M, N, seed=77)
    ind = [np.flatnonzero(m) for m in masks]
    cap = max(i.size for i in ind) + 3
    words = xr.msg_words(P, M, cap, 1)
    assert words == int(lib.lrt_xchg_msg_words(P, M, cap, 1))
    results = {}
    for name, order in (("ascending", "ascending"), ("descending", "descending"), ("shuffled", 2024)):
        host = xr.make_message(P, M, cap, ind, rows, order, guard=xr.GUARD)
        landed = [xr.check_message(host[r], P, M, cap, 1, *_bufs(rows[r], P, M)) for r in range(N)]
        if name == "descending":
            assert all(o == sorted(o, reverse=True) and len(o) >= 4 for o in landed)
        if name == "shuffled":
            assert any(o != sorted(o) and o != sorted(o, reverse=True) for o in landed)
        msgs = torch.from_numpy(host).to(DEV)
        for r in range(N):
            lay = _lay_of(rows[r], P, M)
            status = torch.zeros(1 + N, dtype=torch.int32, device=DEV)
            _apply(lib, P, M, N, r, cap, msgs, lay, status, 0)
            assert status.cpu().tolist() == [0] + [i.size for i in ind]
            results[name, r] = _bits(lay)
    want, _ = xr.apply_ref(_bufs(rows[0], P, M), _lists(host, P, M, cap), P, M, N, 0, cap, 0)
    for key, got in results.items():
        assert np.array_equal(got, _ref_bits(want, P, M)), key               # the predictor's bits, in all three arrangements, on every rank


# ---- side stream ---------------------------------------------------------------------------------------------------------------------------
def test_pack_and_apply_on_a_side_stream_behind_a_long_fill():
    lib = _capi.load()
    P, M, N = 4097, 18, 2
    masks, rows, _, _ = _make_ranks(P, M, N, seed=9)
    cap = int(masks.sum(axis=1).max()) + 3
    lays = [_lay_of(rows[r], P, M) for r in range(N)]
    msgs, host, _ = _pack_ranks(lib, P, M, cap, lays, rows)
    lay = _clone(lays[0])
    _apply(lib, P, M, N, 0, cap, msgs, lay, None, 0)
    on_default = _bits(lay)
    # everything the side stream needs exists before it starts; nothing runs on the default stream meanwhile
    words = xr.msg_words(P, M, cap, 1)
    side_msgs = torch.full((N, words + xr.GUARD), SENT, dtype=torch.int32, device=DEV)
    counters = torch.zeros(2, dtype=torch.int32, device=DEV)
    status = torch.zeros(1 + N, dtype=torch.int32, device=DEV)
    side_lay = _clone(lays[0])
    big = torch.empty(1 << 26, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(8):
            big.fill_(1.0)                                                   # 2 GiB of stores queued in front
        for r in range(N):
            _capi.check(lib.lrt_xchg_pack(0, P, M, cap, *_dense(lays[r]), _capi.ptr(side_msgs[r]), _capi.ptr(counters), r & 1, 1, _stream()), "lrt_xchg_pack")
        _apply(lib, P, M, N, 0, cap, side_msgs, side_lay, status, 0)
    s.synchronize()
    side_host = side_msgs.cpu().numpy()
    for r in range(N):
        xr.check_message(side_host[r], P, M, cap, 1, *_bufs(rows[r], P, M))
    assert np.array_equal(_bits(side_lay), on_default)
    assert status.cpu().tolist() == [0] + masks.sum(axis=1).tolist()


# ---- the refusals --------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch():
    lib = _capi.load()
    P, M, N, cap = 1025, 1, 2, 8
    rows, flay = _scene(P, M)
    lay = _clone(flay)
    words = int(lib.lrt_xchg_msg_words(P, M, cap, 1))
    list_words = int(lib.lrt_xchg_msg_words(P, M, cap, 0))
    msgs = torch.full((N, words), SENT, dtype=torch.int32, device=DEV)       # every buffer is as long as the valid call needs
    counters = torch.zeros(2, dtype=torch.int32, device=DEV)
    status = torch.zeros(1 + N, dtype=torch.int32, device=DEV)
    d = _dense(lay)

    def pack(**o):
        a = dict(P=P, cap=cap, accum=d[5], msg=_capi.ptr(msgs[0]), counters=_capi.ptr(counters), parity=0); a.update(o)
        return lib.lrt_xchg_pack(0, a["P"], M, a["cap"], *d[:5], a["accum"], a["msg"], a["counters"], a["parity"], 1, _stream())

    def apply(**o):
        a = dict(P=P, N=N, rank=0, cap=cap, msgs=_capi.ptr(msgs), words=words, zero_only=0); a.update(o)
        return lib.lrt_xchg_apply(0, a["P"], M, a["N"], a["rank"], a["cap"], a["msgs"], C.c_longlong(a["words"]), *d, _capi.ptr(status), a["zero_only"], _stream())

    refused = [(pack, dict(parity=2)), (pack, dict(parity=-1)), (pack, dict(cap=0)), (pack, dict(P=-1)), (pack, dict(msg=None)), (pack, dict(counters=None)),
               (pack, dict(accum=None)),
               (apply, dict(cap=0)), (apply, dict(P=-1)), (apply, dict(rank=N)), (apply, dict(rank=-1)), (apply, dict(N=0)), (apply, dict(words=words - 1)),
               (apply, dict(words=list_words)), (apply, dict(msgs=None))]
    for f, o in refused:
        rc = f(**o)
        assert rc == LRT_ERR_ARG, (f.__name__, o, rc)
        assert ("lrt_xchg_" + f.__name__).encode() in lib.lrt_last_error(), (f.__name__, o, lib.lrt_last_error())
    # P = 0: success, no launch, nothing written
    assert pack(P=0) == 0 and apply(P=0) == 0 and apply(P=0, zero_only=1) == 0
    torch.cuda.synchronize()
    assert bool((msgs == SENT).all()) and counters.cpu().tolist() == [0, 0] and status.cpu().tolist() == [0] * (1 + N)
    assert np.array_equal(_bits(lay), rows.view(np.int32))                   # no refused call touched the gradient buffer
