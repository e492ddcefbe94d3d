"""Host predictors of the gathering gradient exchange (include/lrt.h: lrt_xchg_pack / lrt_xchg_apply), in plain numpy.

A message of `msg_words(P, M, cap, with_rows)` int32 words is  [off[B] | n[B] | idx[cap] | rows[cap][11 + 3M] (float bits)]  with
B = ceil(P / 1024): block b's touched Gaussians lie at [off[b], off[b] + n[b]), ascending; the blocks land in any order.  Everything here
works on int32 words and compares float32 values by their bit pattern, so -0.0 and NaN payloads are seen.  No torch device is needed:
tests/test_exchange_ref.py runs these predictors on the CPU, tests/test_exchange_kernels_gpu.py holds the kernels against them.
"""
import numpy as np

XB_G = 1024                                  # Gaussians per exchange block
FIELDS = (("means", 3), ("scales", 2), ("rotations", 4), ("opacities", 1))        # then shs (3M) and accum (1)
SENTINEL = np.int32(0x7FC5A5A5)              # a quiet NaN with a payload no input holds; as an index it is far outside any [0, P)
GUARD = 64                                   # sentinel words a test allocates behind a message


def width(M):
    return 11 + 3 * M


def n_blocks(P):
    return (P + XB_G - 1) // XB_G


def msg_words(P, M, cap, with_rows):
    return 2 * n_blocks(P) + cap + (cap * width(M) if with_rows else 0)


def touched(accum):
    """The rule of include/lrt.h, `accum > 0` under IEEE comparison: false for NaN, -0.0, +0.0 and negatives, true for +inf and subnormals."""
    a = np.asarray(accum, dtype=np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        return a > np.float32(0)


def rows_of(fields, accum, P, M):
    """[P, 11 + 3M] int32: the bit patterns of every Gaussian's row  [means 3 | scales 2 | rotations 4 | opacities 1 | shs 3M | accum 1]."""
    parts = [np.ascontiguousarray(fields[k], dtype=np.float32).reshape(P, w) for k, w in FIELDS]
    parts.append(np.ascontiguousarray(fields["shs"], dtype=np.float32).reshape(P, 3 * M))
    parts.append(np.ascontiguousarray(accum, dtype=np.float32).reshape(P, 1))
    return np.concatenate(parts, axis=1).view(np.int32)


def fields_of(rows, P, M):
    """Inverse of rows_of: ({means, scales, rotations, opacities, shs}, accum) as float32 arrays."""
    r = np.ascontiguousarray(rows).view(np.float32).reshape(P, width(M))
    out, o = {}, 0
    for k, w in FIELDS:
        out[k] = r[:, o:o + w].copy(); o += w
    out["shs"] = r[:, o:o + 3 * M].reshape(P, M, 3).copy(); o += 3 * M
    return out, r[:, o].copy()


def split(msg, P, M, cap, with_rows):
    """Views (off, n, idx, rows or None) into one message."""
    B = n_blocks(P)
    off, n, idx = msg[:B], msg[B:2 * B], msg[2 * B:2 * B + cap]
    rows = msg[2 * B + cap:2 * B + cap + cap * width(M)].reshape(cap, width(M)) if with_rows else None
    return off, n, idx, rows


def _fitted(off, n, cap):
    return 0 if off >= cap else min(n, cap - off)


def check_message(msg_words_array, P, M, cap, with_rows, fields, accum, sentinel=SENTINEL, guard=GUARD):
    """Assert the whole contract of ONE message from the source buffers alone; return the blocks in the order they landed.

    `msg_words_array`: int32, the message followed by at least `guard` words, all of it filled with `sentinel` before the pack.
    `fields` may be None for a list-only message (with_rows = 0)."""
    msg = np.asarray(msg_words_array)
    assert msg.dtype == np.int32 and msg.ndim == 1
    words = msg_words(P, M, cap, with_rows)
    assert guard >= GUARD and msg.size >= words + guard, "the test must allocate a sentinel guard behind the message"
    B, W = n_blocks(P), width(M)
    off, n, idx, rows = split(msg, P, M, cap, with_rows)
    t = touched(accum)
    assert t.size == P
    # n[b]: the number of touched Gaussians of block b, for every b
    want_n = np.add.reduceat(t.astype(np.int64), np.arange(0, P, XB_G)) if P > 0 else np.zeros(0, np.int64)
    bad = np.flatnonzero(n.astype(np.int64) != want_n)
    assert bad.size == 0, f"n[{bad[0]}] = {n[bad[0]]}, block {bad[0]} has {want_n[bad[0]]} touched Gaussians"
    total = int(want_n.sum())
    # the intervals of the non-empty blocks tile [0, total): sorted by offset, each starts where the one before ended
    live = np.flatnonzero(want_n > 0)
    order = live[np.argsort(off[live], kind="stable")]
    end = 0
    for b in order:
        assert int(off[b]) == end, f"block {b} lies at [{off[b]}, {off[b] + n[b]}): gap or overlap, the entries before it end at {end}"
        end += int(want_n[b])
    assert end == total
    # an empty block owns no entry; its offset must not make a list that fits look overflowed (apply reads off[b] + n[b] > cap for every b)
    empty = np.flatnonzero(want_n == 0)
    assert np.all((off[empty] >= 0) & (off[empty] <= total)), f"offset of an empty block outside [0, {total}]"
    # every word of idx / rows / guard: the fitted entries hold index and source row, every other word still holds the sentinel
    want = np.full(msg.size, sentinel, dtype=np.int32)
    want[:2 * B] = msg[:2 * B]
    w_idx = want[2 * B:2 * B + cap]
    w_rows = want[2 * B + cap:2 * B + cap + cap * W].reshape(cap, W) if with_rows else None
    src = rows_of(fields, accum, P, M) if with_rows else None
    glist = np.flatnonzero(t)                                   # ascending: block after block
    starts = np.concatenate(([0], np.cumsum(want_n)))
    for b in order:
        fit = _fitted(int(off[b]), int(want_n[b]), cap)
        g = glist[starts[b]:starts[b] + fit]
        w_idx[off[b]:off[b] + fit] = g
        if with_rows:
            w_rows[off[b]:off[b] + fit] = src[g]
    for b in order:                                             # named failures first: order inside a block, then the rows
        fit = _fitted(int(off[b]), int(want_n[b]), cap)
        got = idx[off[b]:off[b] + fit]
        assert np.array_equal(got, w_idx[off[b]:off[b] + fit]), f"idx of block {b}: {got[:8]}.. is not its touched Gaussians in ascending order"
        if with_rows:
            d = np.argwhere(rows[off[b]:off[b] + fit] != w_rows[off[b]:off[b] + fit])
            assert d.size == 0, f"rows[{off[b] + d[0][0]}][{d[0][1]}] is not the source row of Gaussian {w_idx[off[b] + d[0][0]]} (block {b})"
    d = np.flatnonzero(msg != want)
    if d.size:
        p = int(d[0])
        where = "header" if p < 2 * B else f"idx[{p - 2 * B}]" if p < 2 * B + cap else \
            f"rows word {p - 2 * B - cap} (entry {(p - 2 * B - cap) // W})" if p < words else f"guard word {p - words}"
        raise AssertionError(f"{d.size} words outside the fitted entries were written, the first at {where}: {msg[p]:#x}")
    return [int(b) for b in order]


def overflowed_blocks(msgs, P, M, cap, with_rows):
    """bool[B]: off[b] + n[b] > cap in any list."""
    B = n_blocks(P)
    ovf = np.zeros(B, dtype=bool)
    for m in msgs:
        off, n, _, _ = split(m, P, M, cap, with_rows)
        ovf |= off.astype(np.int64) + n.astype(np.int64) > cap
    return ovf


def apply_ref(bufs, msgs, P, M, N, rank, cap, zero_only):
    """What lrt_xchg_apply leaves: (bufs_after, status).  Computed in float32 from the messages as they are, not from any source buffer.

    `bufs`: (fields dict, accum) of the applying rank before the call; `msgs`: N int32 messages (with rows unless zero_only).
    status has 1 + N words: [0] = 1 on any overflowed block, [1 + r] = length of list r (zero_only = 0 only)."""
    fields, accum = bufs
    A = rows_of(fields, accum, P, M).view(np.float32).copy()
    with_rows = not zero_only
    msgs = [np.asarray(m) for m in msgs]
    assert len(msgs) == N and 0 <= rank < N
    parts = [split(m, P, M, cap, with_rows) for m in msgs]
    ovf = overflowed_blocks(msgs, P, M, cap, with_rows)
    status = np.zeros(1 + N, dtype=np.int64)
    status[0] = int(ovf.any())
    zero = np.float32(0.0)
    if zero_only:
        for off, n, idx, _ in parts:
            for b in range(n_blocks(P)):
                fit = _fitted(int(off[b]), int(n[b]), cap)
                A[idx[off[b]:off[b] + fit]] = zero
    else:
        for r in range(N):
            status[1 + r] = int(parts[r][1].astype(np.int64).sum())
        for b in np.flatnonzero(~ovf):
            off, n, idx, _ = parts[rank]
            A[idx[off[b]:off[b] + n[b]]] = zero                           # the own rows first
            for off, n, idx, rows in parts:                               # then list 0, 1, .. N-1: one float32 addition each
                g = idx[off[b]:off[b] + n[b]]
                A[g] = A[g] + rows[off[b]:off[b] + n[b]].view(np.float32)
    return fields_of(A.view(np.int32), P, M), status


def make_message(P, M, cap, lists_of_indices, rows, block_order, sentinel=SENTINEL, guard=0):
    """[N, msg_words + guard] int32: one valid message per list, its blocks placed in a given order.

    `lists_of_indices`: N ascending, duplicate-free index arrays; `rows`: N arrays [P, 11 + 3M] (float32 or their int32 bits) holding each
    rank's source rows, or None for list-only messages; `block_order`: "ascending", "descending", an int (seed of a shuffle) or N explicit
    sequences of the non-empty blocks.  Only valid messages are made (every index in [0, P), every interval inside [0, cap]); anything
    else raises ValueError, because the kernels trust the header.  Words no entry owns hold `sentinel`; empty blocks get off = 0."""
    N, B, W = len(lists_of_indices), n_blocks(P), width(M)
    with_rows = rows is not None
    words = msg_words(P, M, cap, with_rows)
    out = np.full((N, words + guard), sentinel, dtype=np.int32)
    rng = np.random.default_rng(block_order) if isinstance(block_order, (int, np.integer)) else None
    for r, ind in enumerate(lists_of_indices):
        ind = np.asarray(ind, dtype=np.int64).reshape(-1)
        if ind.size and (ind.min() < 0 or ind.max() >= P or np.any(np.diff(ind) <= 0)):
            raise ValueError("indices must be ascending, duplicate-free and inside [0, P)")
        if ind.size > cap or cap < 1:
            raise ValueError("the list does not fit the capacity: make_message builds valid messages only")
        cnt = np.bincount(ind // XB_G, minlength=B)
        live = np.flatnonzero(cnt)
        if isinstance(block_order, str):
            if block_order not in ("ascending", "descending"):
                raise ValueError(block_order)
            order = live if block_order == "ascending" else live[::-1]
        elif rng is not None:
            order = rng.permutation(live)
        else:
            order = np.asarray(block_order[r], dtype=np.int64)
            if sorted(order.tolist()) != live.tolist():
                raise ValueError("block_order must be a permutation of the non-empty blocks")
        off, n, idx, mrows = split(out[r], P, M, cap, with_rows)
        off[:] = 0; n[:] = cnt
        starts = np.concatenate(([0], np.cumsum(cnt)))
        src = np.ascontiguousarray(rows[r]).reshape(P, W).view(np.int32) if with_rows else None
        at = 0
        for b in order:
            g = ind[starts[b]:starts[b + 1]]
            off[b] = at
            idx[at:at + g.size] = g
            if with_rows:
                mrows[at:at + g.size] = src[g]
            at += g.size
    return out
