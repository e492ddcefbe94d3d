"""The host predictors of tests/exchange_ref.py tested without a GPU: a hand case typed out, a case whose result depends on the order of the
additions, and negative controls of the message checker (a checker that can only pass protects nothing)."""
import numpy as np
import pytest

from tests import exchange_ref as xr

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def _rows(P, M, filled):
    """[P, 11 + 3M] float32, zero except the rows named in `filled` = {gaussian: value of every column}."""
    r = np.zeros((P, xr.width(M)), dtype=F32)
    for g, v in filled.items():
        r[g] = v
    return r


# ---- the hand case: P = 5, M = 1 (14 floats per row, one block), list 0 = {1, 3}, list 1 = {3, 4}: Gaussian 3 is shared ------------------
P5, M1 = 5, 1
R0 = _rows(P5, M1, {1: 1.0, 3: 2.0})
R1 = _rows(P5, M1, {3: 0.5, 4: 4.0})


def _hand_bufs():
    """Rank 0's buffer before the apply: its own partial rows, and values at Gaussians 0 and 4 that no correct apply may touch / must overwrite."""
    return xr.fields_of(_bits(_rows(P5, M1, {0: 7.0, 1: 1.0, 3: 2.0, 4: 9.0})), P5, M1)


def _flat(bufs):
    return xr.rows_of(bufs[0], bufs[1], P5, M1).view(F32)


def test_hand_case_sums_in_rank_order_and_reports_the_lengths():
    msgs = xr.make_message(P5, M1, 3, [[1, 3], [3, 4]], [R0, R1], "ascending")
    after, status = xr.apply_ref(_hand_bufs(), msgs, P5, M1, 2, 0, 3, zero_only=0)
    want = np.array([[7.0] * 14,            # in no list: untouched
                     [1.0] * 14,            # own row: cleared, then 0 + 1
                     [0.0] * 14,
                     [2.5] * 14,            # shared: 0 + 2 + 0.5
                     [13.0] * 14], dtype=F32)   # list 1 only: the 9 the buffer held stays under the sum (the caller keeps such rows zero)
    assert np.array_equal(_bits(_flat(after)), _bits(want))
    assert status.tolist() == [0, 2, 2]
    # applied by rank 1, whose buffer holds ITS partial rows: the same sums where the lists reach
    b1 = xr.fields_of(_bits(_rows(P5, M1, {0: 7.0, 3: 0.5, 4: 4.0})), P5, M1)
    after1, status1 = xr.apply_ref(b1, msgs, P5, M1, 2, 1, 3, zero_only=0)
    want1 = np.array([[7.0] * 14, [1.0] * 14, [0.0] * 14, [2.5] * 14, [4.0] * 14], dtype=F32)
    assert np.array_equal(_bits(_flat(after1)), _bits(want1)) and status1.tolist() == [0, 2, 2]


def test_hand_case_zero_only_clears_the_rows_of_all_lists():
    msgs = xr.make_message(P5, M1, 3, [[1, 3], [3, 4]], None, "ascending")
    after, status = xr.apply_ref(_hand_bufs(), msgs, P5, M1, 2, 0, 3, zero_only=1)
    want = np.array([[7.0] * 14, [0.0] * 14, [0.0] * 14, [0.0] * 14, [0.0] * 14], dtype=F32)
    assert np.array_equal(_bits(_flat(after)), _bits(want))
    assert status.tolist() == [0, 0, 0]


def test_hand_case_overflowed_block():
    # cap = 1: each pack fitted its first entry only (list 0: Gaussian 1, list 1: Gaussian 3); the header still says n = 2
    cap = 1
    B = xr.n_blocks(P5)
    msgs = np.full((2, xr.msg_words(P5, M1, cap, 1)), xr.SENTINEL, dtype=np.int32)
    for r, (g, rows) in enumerate(((1, R0), (3, R1))):
        off, n, idx, mrows = xr.split(msgs[r], P5, M1, cap, 1)
        off[0], n[0], idx[0] = 0, 2, g
        mrows[0] = _bits(rows[g])
    assert xr.overflowed_blocks(msgs, P5, M1, cap, 1).tolist() == [True] and B == 1
    before = _hand_bufs()
    after, status = xr.apply_ref(before, msgs, P5, M1, 2, 0, cap, zero_only=0)
    assert np.array_equal(_bits(_flat(after)), _bits(_flat(before)))           # skipped: bit for bit what it was
    assert status.tolist() == [1, 2, 2]                                        # flagged, the true lengths
    lists = np.ascontiguousarray(msgs[:, :xr.msg_words(P5, M1, cap, 0)])       # zero_only reads list-only messages
    after, status = xr.apply_ref(before, lists, P5, M1, 2, 0, cap, zero_only=1)
    want = np.array([[7.0] * 14, [0.0] * 14, [0.0] * 14, [0.0] * 14, [9.0] * 14], dtype=F32)   # the fitted entries 1 and 3; 4 did not fit
    assert np.array_equal(_bits(_flat(after)), _bits(want))
    assert status.tolist() == [1, 0, 0]


def test_an_overflow_in_another_list_skips_the_block_and_only_that_block():
    P, M, cap = 2049, 1, 3                                                     # three blocks
    rows = [_rows(P, M, {0: 1.0, 1030: 2.0, 2048: 3.0}), _rows(P, M, {0: 10.0, 1030: 20.0, 1031: 30.0, 1032: 40.0})]
    msgs = np.full((2, xr.msg_words(P, M, cap, 1)), xr.SENTINEL, dtype=np.int32)
    msgs[0] = xr.make_message(P, M, cap, [[0, 1030, 2048]], [rows[0]], "ascending")[0]
    off, n, idx, mrows = xr.split(msgs[1], P, M, cap, 1)                       # list 1: block 0 fits, block 1 (3 entries at offset 1) does not
    off[:], n[:] = (0, 1, 0), (1, 3, 0)
    idx[:] = (0, 1030, 1031); mrows[:] = _bits(rows[1][[0, 1030, 1031]])
    assert xr.overflowed_blocks(msgs, P, M, cap, 1).tolist() == [False, True, False]
    bufs = xr.fields_of(_bits(rows[0]), P, M)
    after, status = xr.apply_ref(bufs, msgs, P, M, 2, 0, cap, zero_only=0)
    got = xr.rows_of(after[0], after[1], P, M).view(F32)
    assert status.tolist() == [1, 3, 4]
    assert np.all(got[0] == 11.0) and np.all(got[2048] == 3.0)                 # the blocks that fit are summed
    assert np.all(got[1030] == 2.0) and np.all(got[1031] == 0.0)               # the skipped block is what it was


# ---- order ---------------------------------------------------------------------------------------------------------------------------------
def _order_case(vals):
    """Gaussian 2 of P = 5 is in four lists; column 0 of its row holds vals[r] on rank r, every other column r + 1."""
    rows = []
    for r, v in enumerate(vals):
        x = _rows(P5, M1, {2: float(r + 1)}); x[2, 0] = v; x[2, -1] = 0.5      # accum > 0
        rows.append(x)
    return xr.make_message(P5, M1, 2, [[2]] * 4, rows, "ascending"), rows


def test_the_order_sensitive_case_is_order_sensitive_in_the_predictor():
    vals = [1e8, 1.0, -1e8, 1.0]
    msgs, rows = _order_case(vals)
    bufs = xr.fields_of(_bits(rows[0]), P5, M1)
    after, _ = xr.apply_ref(bufs, msgs, P5, M1, 4, 0, 2, zero_only=0)
    fwd = after[0]["means"][2, 0]
    assert _bits(fwd) == _bits(F32(1.0))                   # 0 + 1e8, + 1 (lost), - 1e8 = 0, + 1
    rev_bufs = xr.fields_of(_bits(rows[3]), P5, M1)
    after_r, _ = xr.apply_ref(rev_bufs, msgs[::-1], P5, M1, 4, 0, 2, zero_only=0)
    rev = after_r[0]["means"][2, 0]
    assert _bits(rev) == _bits(F32(0.0))                   # 0 + 1, - 1e8 (the 1 is lost), + 1 (lost), + 1e8 = 0
    assert _bits(fwd) != _bits(rev)                        # so this case can see a wrong order
    assert after[0]["means"][2, 1] == after_r[0]["means"][2, 1] == 10.0          # an ordinary column cannot: 1 + 2 + 3 + 4 either way


# ---- negative controls of check_message ----------------------------------------------------------------------------------------------------
def _valid_message(cap_slack=5, block_order="descending"):
    P, M = 3000, 2                                                              # three blocks with different counts
    rng = np.random.default_rng(7)
    rows = rng.standard_normal((P, xr.width(M))).astype(F32)
    accum = np.where(rng.random(P) < np.linspace(0.05, 0.3, P), rng.random(P) + 0.1, 0.0).astype(F32)
    rows[:, -1] = accum
    fields, accum = xr.fields_of(_bits(rows), P, M)
    ind = np.flatnonzero(xr.touched(accum))
    cap = ind.size + cap_slack
    msg = xr.make_message(P, M, cap, [ind], [rows], block_order, guard=xr.GUARD)[0]
    return msg, P, M, cap, fields, accum


@pytest.mark.parametrize("block_order", ["ascending", "descending", 11])
def test_check_message_passes_a_valid_message_and_returns_the_landing_order(block_order):
    msg, P, M, cap, fields, accum = _valid_message(block_order=block_order)
    order = xr.check_message(msg, P, M, cap, 1, fields, accum)
    assert sorted(order) == [0, 1, 2]
    if block_order == "ascending":
        assert order == [0, 1, 2]
    if block_order == "descending":
        assert order == [2, 1, 0]
    lst = xr.make_message(P, M, cap, [np.flatnonzero(xr.touched(accum))], None, block_order, guard=xr.GUARD)[0]
    assert xr.check_message(lst, P, M, cap, 0, None, accum) == order


def _swap_idx(msg, P, M, cap):
    off, n, idx, _ = xr.split(msg, P, M, cap, 1)
    idx[off[1]], idx[off[1] + 1] = idx[off[1] + 1], idx[off[1]]


def _swap_idx_and_rows(msg, P, M, cap):                                        # rows still follow their index: only the order is wrong
    off, n, idx, rows = xr.split(msg, P, M, cap, 1)
    a, b = off[1], off[1] + 1
    idx[a], idx[b] = idx[b], idx[a]
    rows[[a, b]] = rows[[b, a]]


def _flip_row_bit(msg, P, M, cap):
    off, n, idx, rows = xr.split(msg, P, M, cap, 1)
    rows[off[2] + n[2] - 1, xr.width(M) - 2] ^= 1                               # the last bit of one float


def _swap_off(msg, P, M, cap):
    off, n, idx, _ = xr.split(msg, P, M, cap, 1)
    assert n[0] != n[2]
    off[0], off[2] = off[2], off[0]


def _write_unused_idx(msg, P, M, cap):
    off, n, idx, _ = xr.split(msg, P, M, cap, 1)
    idx[int(n.sum())] = 17                                                      # the first idx word no entry owns


def _write_unused_row(msg, P, M, cap):
    off, n, idx, rows = xr.split(msg, P, M, cap, 1)
    rows[cap - 1, 0] = 0


def _write_guard(msg, P, M, cap):
    msg[xr.msg_words(P, M, cap, 1)] = 0                                         # the first word past the message


def _wrong_count(msg, P, M, cap):
    off, n, idx, _ = xr.split(msg, P, M, cap, 1)
    n[1] -= 1


@pytest.mark.parametrize("corrupt", [_swap_idx, _swap_idx_and_rows, _flip_row_bit, _swap_off, _write_unused_idx, _write_unused_row, _write_guard,
                                     _wrong_count], ids=lambda f: f.__name__.strip("_"))
def test_check_message_raises_on_every_corruption(corrupt):
    msg, P, M, cap, fields, accum = _valid_message()
    xr.check_message(msg, P, M, cap, 1, fields, accum)                          # passes before
    corrupt(msg, P, M, cap)
    with pytest.raises(AssertionError):
        xr.check_message(msg, P, M, cap, 1, fields, accum)


def test_check_message_treats_entries_beyond_the_capacity_as_unwritten():
    full, P, M, cap_full, fields, accum = _valid_message(cap_slack=0, block_order="ascending")
    cap = cap_full // 2
    B, W = xr.n_blocks(P), xr.width(M)
    off, n, idx, rows = xr.split(full, P, M, cap_full, 1)
    msg = np.full(xr.msg_words(P, M, cap, 1) + xr.GUARD, xr.SENTINEL, dtype=np.int32)   # what a pack with the smaller capacity leaves
    o2, n2, i2, r2 = xr.split(msg, P, M, cap, 1)
    o2[:], n2[:], i2[:], r2[:] = off, n, idx[:cap], rows[:cap]
    assert xr.check_message(msg, P, M, cap, 1, fields, accum) == [0, 1, 2]
    assert xr.overflowed_blocks([msg[:-xr.GUARD]], P, M, cap, 1).tolist() == [False, True, True]
    i2[cap - 1] += 1                                                            # a wrong fitted entry is still seen
    with pytest.raises(AssertionError):
        xr.check_message(msg, P, M, cap, 1, fields, accum)
    i2[cap - 1] -= 1
    r2[cap - 1, 0] = xr.SENTINEL                                                # and so is a fitted row that was not written
    with pytest.raises(AssertionError):
        xr.check_message(msg, P, M, cap, 1, fields, accum)


def test_touched_is_the_ieee_rule():
    a = np.array([np.nan, -0.0, 0.0, -1.0, np.inf, 1e-45, 1e-38, -np.inf, 1.0], dtype=F32)
    assert xr.touched(a).tolist() == [False, False, False, False, True, True, True, False, True]


def test_make_message_builds_valid_messages_only():
    rows = [np.zeros((5, 14), F32)]
    for bad in ([5], [-1], [3, 3], [4, 2]):
        with pytest.raises(ValueError):
            xr.make_message(5, 1, 4, [bad], rows, "ascending")
    with pytest.raises(ValueError):
        xr.make_message(5, 1, 1, [[1, 2]], rows, "ascending")                   # does not fit the capacity
    with pytest.raises(ValueError):
        xr.make_message(2049, 1, 4, [[1, 2000]], None, [[0, 2]])                # not a permutation of the non-empty blocks {0, 1}
