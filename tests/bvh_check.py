"""What a valid LBVH of this library IS, restated in numpy (tests only: no torch, no HIP, no code shared with csrc/lrt_build.inc).

The tree is implicit and 8-wide: 8 sorted slots per leaf, 8 leaves per level-1 node, 8 level-(l-1) nodes per level-l node; the levels are stored
top down (the root is node 0).  Every node exists twice, 64 words each:
  SoA (lrt_debug_read 2):  lo.x[8] lo.y[8] lo.z[8] hi.x[8] hi.y[8] hi.z[8] | first child (int) | leaf flag (int) | 14 unused words
  AoS (lrt_debug_read 10): child c = words 8 c .. 8 c + 7 = lo.x hi.x lo.y hi.y lo.z hi.z | pointer (int) | flags (int: 1 leaf, 2 empty)
A record (lrt_debug_read 1) is 16 words: n, opacity | mu, flim | a, Gaussian index (int) | b, 0; opacity = flim = -1 marks a slot that cannot be hit.

check_tree states the invariants I1 .. I8 of a build against the float64 quads of the Gaussians it was built from and returns the violations as
strings that begin with the invariant's name; reference_tree is a plain builder of a tree that satisfies them (tests/test_bvh_check.py mutates it
to show that the checker can fail)."""
from collections import namedtuple

import numpy as np

LEAF = 8
NODE_WORDS = 64
REC_WORDS = 16
EMPTY = np.float32(1e30)
ALPHA_MIN = np.float32(1.0) / np.float32(255.0)
PADDING_RECORD = np.array([0, 0, 1, -1, 0, 0, 0, -1, 0, 0, 0, 0, 0, 0, 0, 0], np.float32)
MAX_REPORTED = 4          # violations spelled out per invariant and kind; the rest is counted

Layout = namedtuple("Layout", "leaves levels cnt off n_nodes")
Quads = namedtuple("Quads", "corners hittable mu h pad R f")


# ----------------------------------------------------------------------------------------------------------------------- layout
def tree_layout(P_built):
    """Leaves, levels L, cnt[l] nodes of level l (cnt[0] = leaves), off[l] first node of level l (off[0] = None), nodes in all."""
    leaves = (int(P_built) + LEAF - 1) // LEAF
    cnt = [leaves]
    while True:
        cnt.append(max(1, (cnt[-1] + 7) // 8))
        if cnt[-1] == 1:
            break
    L = len(cnt) - 1
    off, o = [None] * (L + 1), 0
    for l in range(L, 0, -1):
        off[l] = o
        o += cnt[l]
    return Layout(leaves, L, cnt, off, o)


# ----------------------------------------------------------------------------------------------------------------------- quads
def quads64(means, scales, rotations, opacities, mod=1.0):
    """The proxy quads in float64 from the float32 parameters: corners (P, 4, 3) = mu +- ex R[:, 0] +- ey R[:, 1] with
    (ex, ey) = scales x (sqrt(2 ln(255 op)) + 0.01) -- the scale modifier does not enter --, the mask of the Gaussians that can be hit, and what
    the box bounds are made of: mu, h = |R[:, 0]| ex + |R[:, 1]| ey (the half extent per axis), pad = 1e-4 + 1e-5 (|mu| + h)."""
    m32, s32, q32 = np.asarray(means, np.float32).reshape(-1, 3), np.asarray(scales, np.float32).reshape(-1, 2), np.asarray(rotations, np.float32).reshape(-1, 4)
    o32 = np.asarray(opacities, np.float32).reshape(-1)
    mu, s, q, op = m32.astype(np.float64), s32.astype(np.float64), q32.astype(np.float64), o32.astype(np.float64)
    with np.errstate(all="ignore"):
        q = q / np.linalg.norm(q, axis=1, keepdims=True)
        w, x, y, z = q.T
        R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                      2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                      2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
        prod = 255.0 * op
        # within 1e-4 of the threshold the float32 product's rounding is what the logarithm sees (ln(1 + d) ~ d: a relative 6e-8 of the
        # product is a relative 6e-4 of the logarithm there, and all of it below 1 + 6e-8)
        near = np.abs(prod - 1.0) <= 1e-4
        prod = np.where(near, (o32 * np.float32(255.0)).astype(np.float64), prod)
        f = np.sqrt(2.0 * np.log(prod)) + 0.01
        ex, ey = s[:, 0] * f, s[:, 1] * f
        e0, e1 = R[:, :, 0] * ex[:, None], R[:, :, 1] * ey[:, None]
        corners = np.stack([mu + e0 + e1, mu + e0 - e1, mu - e0 + e1, mu - e0 - e1], 1)
        h = np.abs(e0) + np.abs(e1)
        pad = 1e-4 + 1e-5 * (np.abs(mu) + h)
        lo, hi = mu - h - pad, mu + h + pad
        finite = (np.isfinite(mu).all(1) & np.isfinite(s).all(1) & np.isfinite(q).all(1) & np.isfinite(op) & np.isfinite(f)
                  & np.isfinite(corners).all((1, 2)) & np.isfinite(lo).all(1) & np.isfinite(hi).all(1))
        hittable = (o32 > ALPHA_MIN) & finite & (ex > 0) & (ey > 0) & (np.abs(lo) < 1e30).all(1) & (np.abs(hi) < 1e30).all(1)
    return Quads(corners, hittable, mu, h, pad, R, f)


# ----------------------------------------------------------------------------------------------------------------------- views
def _as_words(a, width):
    a = np.ascontiguousarray(a)
    if a.dtype != np.float32:
        a = a.view(np.uint8).reshape(-1).view(np.float32)
    return a.reshape(-1, width)


def soa_boxes(nodes):
    """(lo, hi), each (n_nodes, 8 children, 3)."""
    b = nodes[:, :48].reshape(-1, 6, 8)
    return b[:, 0:3].transpose(0, 2, 1), b[:, 3:6].transpose(0, 2, 1)


def aos_boxes(nodes):
    """(lo, hi, pointer, flags): (n_nodes, 8, 3) twice, (n_nodes, 8) int32 twice."""
    c = nodes.reshape(-1, 8, 8)
    i = c.view(np.int32)
    return c[:, :, 0:6:2], c[:, :, 1:6:2], i[:, :, 6], i[:, :, 7]


def padding_slots(records):
    """Mask of the slots that hold exactly the padding record (0, 0, 1, -1 | 0, 0, 0, -1 | 0, 0, 0, 0 | 0, 0, 0, 0)."""
    return (_as_words(records, REC_WORDS).view(np.uint32) == PADDING_RECORD.view(np.uint32)).all(1)


class _Report:
    def __init__(self):
        self.out = []

    def add(self, tag, what, bad, describe):
        """bad: indices (tuple of arrays from np.nonzero, or one array) of the violations of one kind."""
        idx = bad if isinstance(bad, tuple) else (np.asarray(bad),)
        n = len(idx[0])
        if n == 0:
            return
        first = "; ".join(describe(*[int(a[k]) for a in idx]) for k in range(min(n, MAX_REPORTED)))
        self.out.append(f"{tag}: {what}: {n} violation{'s' if n > 1 else ''}: {first}" + (" ..." if n > MAX_REPORTED else ""))

    def say(self, tag, text):
        self.out.append(f"{tag}: {text}")


# ----------------------------------------------------------------------------------------------------------------------- nodes
def check_nodes(nodes_soa, nodes_aos, P_built, leaf_live=None, from_level=1):
    """I4 .. I8 on the two node arrays of a tree over P_built slots.  leaf_live[j]: leaf j holds a primitive that can be hit (from the records);
    None: level 1 is taken as it is (its non-empty children are the live leaves) and the levels from 2 on are checked against it."""
    rep = _Report()
    lay = tree_layout(P_built)
    soa, aos = _as_words(nodes_soa, NODE_WORDS), _as_words(nodes_aos, NODE_WORDS)
    if soa.shape[0] != lay.n_nodes or aos.shape[0] != lay.n_nodes:
        rep.say("I6", f"{soa.shape[0]} SoA / {aos.shape[0]} AoS nodes, the layout of {P_built} slots has {lay.n_nodes}")
        return rep.out
    slo, shi = soa_boxes(soa)
    alo, ahi, aptr, aflag = aos_boxes(aos)
    shead = soa.view(np.int32)[:, 48:50]
    L, cnt, off = lay.levels, lay.cnt, lay.off

    def lvl(a, l):
        return a[off[l]:off[l] + cnt[l]]

    def where(l):
        return lambda j, c, *_: f"level {l} node {j} (node {off[l] + j}) child {c}"

    # I5 (no NaN) and I7 on every node
    for name, a in (("SoA", soa[:, :48]), ("AoS", np.concatenate([alo, ahi], 2).reshape(-1, 48))):
        rep.add("I5", f"NaN in a box word of the {name} copy", np.nonzero(np.isnan(a).any(1))[0], lambda n: f"node {n}")
    same = (slo.view(np.uint32) == alo.view(np.uint32)) | (slo == alo)
    same &= (shi.view(np.uint32) == ahi.view(np.uint32)) | (shi == ahi)
    rep.add("I7", "the box of a child differs between the SoA and the AoS copy", np.nonzero(~same.all(2)), lambda n, c: f"node {n} child {c}")

    s_empty_all = (slo == EMPTY).all(2) & (shi == EMPTY).all(2)
    s_empty_any = (slo == EMPTY).any(2) | (shi == EMPTY).any(2) | (slo[:, :, 0] > shi[:, :, 0])
    a_empty_all = (alo == EMPTY).all(2) & (ahi == EMPTY).all(2) & (aptr == 0) & (aflag == 2)
    a_empty_any = (alo == EMPTY).any(2) | (ahi == EMPTY).any(2) | (aflag == 2) | (alo[:, :, 0] > ahi[:, :, 0])

    # live[l]: (cnt[l], 8) -- child c of node j of level l has a primitive below it that can be hit
    if leaf_live is None:
        live1 = ~lvl(s_empty_all, 1)
    else:
        ll = np.zeros(cnt[1] * 8, bool)
        ll[:lay.leaves] = np.asarray(leaf_live, bool)[:lay.leaves]
        live1 = ll.reshape(cnt[1], 8)
    live = {1: live1}
    for l in range(2, L + 1):
        below = np.zeros(cnt[l] * 8, bool)
        below[:cnt[l - 1]] = live[l - 1].any(1)
        live[l] = below.reshape(cnt[l], 8)

    for l in range(max(1, from_level), L + 1):
        lv = live[l]
        if not (l == 1 and leaf_live is None):
            # I5: empty exactly when nothing below can be hit, in both copies, with every word of the empty pattern
            rep.add("I5", "a child with nothing to hit below it is not empty in the SoA copy (six words 1e30)", np.nonzero(~lv & ~lvl(s_empty_all, l)), where(l))
            rep.add("I5", "a child with nothing to hit below it is not empty in the AoS copy (six words 1e30, pointer 0, flags 2)", np.nonzero(~lv & ~lvl(a_empty_all, l)), where(l))
            rep.add("I5", "a child with something to hit below it is empty (or half empty) in the SoA copy", np.nonzero(lv & lvl(s_empty_any, l)), where(l))
            rep.add("I5", "a child with something to hit below it is flagged empty (or half empty) in the AoS copy", np.nonzero(lv & lvl(a_empty_any, l)), where(l))
        # I6: pointers, flags, headers
        j, c = np.meshgrid(np.arange(cnt[l]), np.arange(8), indexing="ij")
        want_ptr = 8 * j + c + (0 if l == 1 else off[l - 1])
        want_flag = 1 if l == 1 else 0
        ne = ~lvl(a_empty_all, l) & lv
        rep.add("I6", f"AoS child pointer is not {'the leaf index 8 j + c' if l == 1 else 'off[l - 1] + 8 j + c'}", np.nonzero(ne & (lvl(aptr, l) != want_ptr)),
                lambda jj, cc, l=l: f"level {l} node {jj} child {cc}: {int(lvl(aptr, l)[jj, cc])}")
        rep.add("I6", f"AoS child flags are not {want_flag}", np.nonzero(ne & (lvl(aflag, l) != want_flag)),
                lambda jj, cc, l=l: f"level {l} node {jj} child {cc}: {int(lvl(aflag, l)[jj, cc])}")
        want_first = 8 * np.arange(cnt[l]) + (0 if l == 1 else off[l - 1])
        rep.add("I6", "SoA word 48 is not the first child", np.nonzero(lvl(shead, l)[:, 0] != want_first)[0], lambda jj, l=l: f"level {l} node {jj}: {int(lvl(shead, l)[jj, 0])}")
        rep.add("I6", f"SoA word 49 (leaf flag) is not {want_flag}", np.nonzero(lvl(shead, l)[:, 1] != want_flag)[0], lambda jj, l=l: f"level {l} node {jj}: {int(lvl(shead, l)[jj, 1])}")
        # I4: the box of child c of node j = the union of the non-empty children of node 8 j + c one level down, exactly
        if l >= 2:
            clo, chi, cem = lvl(slo, l - 1), lvl(shi, l - 1), lvl(s_empty_all, l - 1)
            ulo = np.where(cem[:, :, None], np.float32(np.inf), clo).min(1)
            uhi = np.where(cem[:, :, None], np.float32(-np.inf), chi).max(1)
            none = cem.all(1)
            ulo[none] = EMPTY
            uhi[none] = EMPTY
            wlo = np.full((cnt[l] * 8, 3), EMPTY, np.float32)
            whi = np.full((cnt[l] * 8, 3), EMPTY, np.float32)
            wlo[:cnt[l - 1]] = ulo
            whi[:cnt[l - 1]] = uhi
            bad = ~((lvl(slo, l).reshape(-1, 3) == wlo).all(1) & (lvl(shi, l).reshape(-1, 3) == whi).all(1)).reshape(cnt[l], 8)
            rep.add("I4", "the box of a child is not the union of the boxes one level down", np.nonzero(bad),
                    lambda jj, cc, l=l, wlo=wlo, whi=whi: (f"level {l} node {jj} child {cc}: [{lvl(slo, l)[jj, cc]}, {lvl(shi, l)[jj, cc]}], "
                                                         f"the union is [{wlo[8 * jj + cc]}, {whi[8 * jj + cc]}]"))

    # I8: a walk from node 0 by the AoS pointers and flags alone reaches every live leaf once and no other
    visits = np.zeros(max(lay.leaves, 1) + 1, np.int64)          # the last word collects leaf pointers out of range
    frontier, steps, lost = np.zeros(1, np.int64), 0, 0
    while frontier.size and steps <= L + 1:
        ptr, flag = aptr[frontier].reshape(-1).astype(np.int64), aflag[frontier].reshape(-1)
        leaf = ptr[flag == 1]
        ok = (leaf >= 0) & (leaf < lay.leaves)
        np.add.at(visits, np.where(ok, leaf, visits.size - 1), 1)
        inner = ptr[flag == 0]
        good = (inner > 0) & (inner < lay.n_nodes)
        lost += int((~good).sum()) + int(((flag != 0) & (flag != 1) & (flag != 2)).sum())
        frontier = inner[good]
        steps += 1
        if frontier.size > 8 * lay.n_nodes:
            break
    if frontier.size:
        rep.say("I8", f"the walk does not end: {frontier.size} nodes still open after {steps} levels")
    if lost:
        rep.say("I8", f"the walk meets {lost} inner pointers out of range (or flags that are none of 0, 1, 2)")
    if visits[-1]:
        rep.say("I8", f"the walk meets {int(visits[-1])} leaf pointers that are not below {lay.leaves}")
    leaf_want = live[1].reshape(-1)[:max(lay.leaves, 1)]
    if lay.leaves == 0:
        leaf_want = np.zeros(1, bool)
    got = visits[:-1]
    rep.add("I8", "a leaf with something to hit is not reached by the walk", np.nonzero(leaf_want & (got == 0))[0], lambda j: f"leaf {j}")
    rep.add("I8", "a leaf is reached more than once", np.nonzero(got > 1)[0], lambda j: f"leaf {j} ({int(got[j])} times)")
    rep.add("I8", "a leaf with nothing to hit is reached", np.nonzero(~leaf_want & (got > 0))[0], lambda j: f"leaf {j}")
    return rep.out


# ----------------------------------------------------------------------------------------------------------------------- the whole build
def check_tree(order, records, nodes_soa, nodes_aos, params, mod=1.0, quads=None):
    """The violations of I1 .. I8 (strings, each beginning with the invariant's name) of one build of the Gaussians `params` (means, scales,
    rotations, opacities).  order: the sorted order of an unculled build (lrt_debug_read 0), or None for a ray-culled build, whose slots hold a
    subset (I1 then: the indices of the slots that can be hit are distinct and the reference calls all of them hittable; every other slot is marked
    -1).  quads: quads64 of the same parameters, when the caller has them already."""
    rep = _Report()
    q = quads if quads is not None else quads64(params["means"], params["scales"], params["rotations"], params["opacities"], mod)
    P = q.hittable.shape[0]
    rec = _as_words(records, REC_WORDS)
    S = rec.shape[0]
    gi = rec.view(np.int32)[:, 11].astype(np.int64)
    lay = tree_layout(S)

    # ---- I1
    in_range = (gi >= 0) & (gi < max(P, 1)) if P > 0 else (gi == 0)
    rep.add("I1", f"record word 11 is not an index below {P}", np.nonzero(~in_range)[0], lambda k: f"slot {k}: {int(gi[k])}")
    g = np.where(in_range, gi, 0)
    live = (rec[:, 3] > 0) & (rec[:, 7] > 0)
    dead = (rec[:, 3] == -1) & (rec[:, 7] == -1)
    rep.add("I1", "words 3 and 7 of a record are neither both positive nor both -1", np.nonzero(~live & ~dead)[0], lambda k: f"slot {k}: {rec[k, 3]}, {rec[k, 7]}")
    ref_hit = q.hittable[g] & in_range if P > 0 else np.zeros(S, bool)
    padding = padding_slots(rec)
    if order is not None:
        order = np.asarray(order).reshape(-1).astype(np.int64)
        if S != P or order.shape[0] != P:
            rep.say("I1", f"{S} records and {order.shape[0]} entries of the order for {P} Gaussians")
        else:
            seen = np.bincount(g, minlength=P)
            rep.add("I1", "the record indices are not a permutation: an index is repeated or missing", np.nonzero(seen != 1)[0], lambda i: f"Gaussian {i} ({int(seen[i])} slots)")
            rep.add("I1", "a record's index is not the sorted order's", np.nonzero(gi != order)[0], lambda k: f"slot {k}: {int(gi[k])}, order {int(order[k])}")
            rep.add("I1", "a Gaussian that can be hit is marked -1", np.nonzero(ref_hit & ~live)[0], lambda k: f"slot {k} (Gaussian {int(gi[k])})")
            rep.add("I1", "a Gaussian that cannot be hit is not marked -1", np.nonzero(~ref_hit & ~dead)[0], lambda k: f"slot {k} (Gaussian {int(gi[k])})")
    else:
        kept = gi[live & in_range]
        seen = np.bincount(kept, minlength=max(P, 1))
        rep.add("I1", "a Gaussian is in two slots of the culled build", np.nonzero(seen > 1)[0], lambda i: f"Gaussian {i} ({int(seen[i])} slots)")
        rep.add("I1", "a Gaussian that cannot be hit is in the culled build as one that can", np.nonzero(live & ~ref_hit)[0], lambda k: f"slot {k} (Gaussian {int(gi[k])})")
        rep.add("I1", "a slot of the culled build that is no padding holds a Gaussian that can be hit, marked -1", np.nonzero(dead & ~padding & ref_hit)[0],
                lambda k: f"slot {k} (Gaussian {int(gi[k])})")
    if not in_range.all():
        return rep.out + check_nodes(nodes_soa, nodes_aos, S)

    # ---- I2, I3: the leaf boxes (the child slots of the level-1 nodes) against the float64 quads of the records that can be hit
    soa, aos = _as_words(nodes_soa, NODE_WORDS), _as_words(nodes_aos, NODE_WORDS)
    use = live & ref_hit
    if soa.shape[0] == lay.n_nodes and aos.shape[0] == lay.n_nodes and use.any():
        k = np.nonzero(use)[0]
        leaf = k // LEAF
        node, child = lay.off[1] + leaf // 8, leaf % 8
        far_lo = q.mu[g[k]] - q.h[g[k]] - 2 * q.pad[g[k]]
        far_hi = q.mu[g[k]] + q.h[g[k]] + 2 * q.pad[g[k]]
        ext_lo = np.full((lay.leaves, 3), np.inf)
        ext_hi = np.full((lay.leaves, 3), -np.inf)
        np.minimum.at(ext_lo, leaf, far_lo)
        np.maximum.at(ext_hi, leaf, far_hi)
        cmin, cmax = q.corners[g[k]].min(1), q.corners[g[k]].max(1)
        for name, (lo, hi) in (("SoA", soa_boxes(soa)), ("AoS", aos_boxes(aos)[:2])):
            blo, bhi = lo[node, child].astype(np.float64), hi[node, child].astype(np.float64)
            out = ~((cmin >= blo).all(1) & (cmax <= bhi).all(1))
            rep.add("I2", f"a corner of a quad lies outside its leaf's box ({name})", np.nonzero(out)[0],
                    lambda i, blo=blo, bhi=bhi: f"slot {int(k[i])} (Gaussian {int(g[k[i]])}, leaf {int(leaf[i])}): corners span [{cmin[i]}, {cmax[i]}], box [{blo[i]}, {bhi[i]}]")
            lv = np.unique(leaf)
            n1, c1 = lay.off[1] + lv // 8, lv % 8
            llo, lhi = lo[n1, c1].astype(np.float64), hi[n1, c1].astype(np.float64)
            loose = ~((llo >= ext_lo[lv]).all(1) & (lhi <= ext_hi[lv]).all(1))
            rep.add("I3", f"a leaf's box reaches further out than any of its quads by more than two pads ({name})", np.nonzero(loose)[0],
                    lambda i, llo=llo, lhi=lhi: f"leaf {int(lv[i])}: box [{llo[i]}, {lhi[i]}], quads with two pads [{ext_lo[lv[i]]}, {ext_hi[lv[i]]}]")

    # ---- I4 .. I8
    leaf_live = np.zeros(max(lay.leaves, 1) * LEAF, bool)
    leaf_live[:S] = live
    return rep.out + check_nodes(soa, aos, S, leaf_live.reshape(-1, LEAF).any(1)[:lay.leaves] if lay.leaves else np.zeros(0, bool))


def tags(violations):
    """The invariants named by a list of violations."""
    return {v.split(":", 1)[0] for v in violations}


# ----------------------------------------------------------------------------------------------------------------------- reference builder
def _outwards(x64, up):
    x = x64.astype(np.float32)
    wrong = (x.astype(np.float64) < x64) if up else (x.astype(np.float64) > x64)
    return np.where(wrong, np.nextafter(x, np.float32(np.inf if up else -np.inf)), x).astype(np.float32)


def reference_tree(order, params, mod=1.0, slots=None):
    """(records, nodes_soa, nodes_aos) of a valid tree over the Gaussians in `order` (the slots beyond len(order), up to `slots`, are padding):
    float64 quads, boxes padded as the library pads them and rounded outwards to float32.  For the CPU controls of the checker only."""
    q = quads64(params["means"], params["scales"], params["rotations"], params["opacities"], mod)
    order = np.asarray(order, np.int64).reshape(-1)
    n = order.shape[0]
    S = n if slots is None else int(slots)
    lay = tree_layout(S)
    rec = np.tile(PADDING_RECORD, (S, 1))
    hit = q.hittable[order]
    with np.errstate(all="ignore"):
        s = np.asarray(params["scales"], np.float64).reshape(-1, 2)[order] * mod
        rec[:n, 0:3] = q.R[order][:, :, 2]
        rec[:n, 3] = np.where(hit, np.asarray(params["opacities"], np.float32).reshape(-1)[order], -1)
        rec[:n, 4:7] = q.mu[order]
        rec[:n, 7] = np.where(hit, q.f[order] / mod, -1)
        rec[:n, 8:11] = q.R[order][:, :, 0] / s[:, :1]
        rec[:n, 12:15] = q.R[order][:, :, 1] / s[:, 1:]
        rec[:n, 15] = 0
    rec.view(np.int32)[:n, 11] = order
    # slot boxes -> leaf boxes -> levels
    slot_lo = np.full((max(lay.cnt[1], 1) * 64, 3), np.inf, np.float32)
    slot_hi = np.full((max(lay.cnt[1], 1) * 64, 3), -np.inf, np.float32)
    sel = np.nonzero(hit)[0]
    slot_lo[sel] = _outwards(q.mu[order[sel]] - q.h[order[sel]] - q.pad[order[sel]], False)
    slot_hi[sel] = _outwards(q.mu[order[sel]] + q.h[order[sel]] + q.pad[order[sel]], True)
    soa = np.zeros((lay.n_nodes, NODE_WORDS), np.float32)
    aos = np.zeros((lay.n_nodes, NODE_WORDS), np.float32)
    lo, hi = slot_lo.reshape(-1, LEAF, 3).min(1), slot_hi.reshape(-1, LEAF, 3).max(1)      # per child of level 1
    for l in range(1, lay.levels + 1):
        c, o = lay.cnt[l], lay.off[l]
        lo, hi = lo[:c * 8].reshape(c, 8, 3), hi[:c * 8].reshape(c, 8, 3)
        empty = lo[:, :, 0] > hi[:, :, 0]
        blo, bhi = np.where(empty[:, :, None], EMPTY, lo), np.where(empty[:, :, None], EMPTY, hi)
        soa[o:o + c, :48] = np.concatenate([blo.transpose(0, 2, 1), bhi.transpose(0, 2, 1)], 1).reshape(c, 48)
        base = 0 if l == 1 else lay.off[l - 1]
        soa.view(np.int32)[o:o + c, 48] = base + 8 * np.arange(c)
        soa.view(np.int32)[o:o + c, 49] = 1 if l == 1 else 0
        a = aos[o:o + c].reshape(c, 8, 8)
        a[:, :, 0:6:2], a[:, :, 1:6:2] = blo, bhi
        ai = aos.view(np.int32)[o:o + c].reshape(c, 8, 8)
        ai[:, :, 6] = np.where(empty, 0, base + 8 * np.arange(c)[:, None] + np.arange(8)[None, :])
        ai[:, :, 7] = np.where(empty, 2, 1 if l == 1 else 0)
        # the boxes of this level's nodes are the children of the next, padded to a multiple of eight
        nxt = lay.cnt[l + 1] * 8 if l < lay.levels else 0
        ulo = np.full((max(nxt, c), 3), np.inf, np.float32)
        uhi = np.full((max(nxt, c), 3), -np.inf, np.float32)
        ulo[:c], uhi[:c] = lo.min(1), hi.max(1)
        lo, hi = ulo, uhi
    return rec, soa, aos
