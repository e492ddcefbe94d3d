"""Near rays collect their hits lazily, slab by slab of depth (csrc/lrt_near.inc, near_collect: borders 1.5, 6, 24, 96, 384 m).  A quad is
taken by a slab when its plane depth t lies in [b_lo, b_hi); a node is entered when its box's exit depth tf >= b_lo, and a box with
tf >= b_hi asks for the next slab.  If a quad's t could reach b_hi while its leaf box's tf stayed below b_hi, the quad would belong to the
next slab, which never enters its box: the hit would be lost.

This file restates both depth formulas of near_collect in float32 (with and without FMA contraction of the dot products) and the box of
lrt_make_splat (csrc/lrt_math.h), and searches rays and axis-aligned quads whose depth falls on a slab border.  Without the build's box
padding such straddles exist; with it the exit depth of every box stays beyond its quad's depth by far more than the rounding, so no
slab can lose the hit.  `straddling_scene` turns the found cases into a scene (one near quad per ray within 0.2 m, so every ray is a near
ray) that tests/test_near_rays_gpu.py traces against the oracle.
"""
import numpy as np

F = np.float32
BORDERS = (1.5, 6.0, 24.0, 96.0, 384.0)
IDENT = np.array([1.0, 0.0, 0.0, 0.0], F)


def _fma(a, b, c):
    return F(np.float64(F(a)) * np.float64(F(b)) + np.float64(F(c)))


def _dot3(a, b, fma):
    if fma:
        return _fma(a[2], b[2], _fma(a[1], b[1], F(a[0] * b[0])))
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


def _rot(q):
    q = np.asarray(q, F)
    s = F(F(1.0) / F(np.sqrt(F(F(F(q[0] * q[0]) + F(q[1] * q[1])) + F(F(q[2] * q[2]) + F(q[3] * q[3]))))))
    w, x, y, z = (F(v * s) for v in q)
    one, two = F(1), F(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                     [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                     [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], F)


def quad_box(mu, sc, q, op, padded=True):
    """lrt_make_splat's world box of the quad (pad 1e-4 + 1e-5 (|mu| + h) per axis), float32."""
    R = _rot(q)
    f = F(F(np.sqrt(F(F(2.0) * F(np.log(F(F(op) * F(255.0))))))) + F(0.01))
    ex, ey = F(sc[0] * f), F(sc[1] * f)
    lo, hi = np.empty(3, F), np.empty(3, F)
    for i in range(3):
        h = F(F(abs(R[i, 0]) * ex) + F(abs(R[i, 1]) * ey))
        pad = F(F(1e-4) + F(F(1e-5) * F(abs(mu[i]) + h))) if padded else F(0)
        lo[i], hi[i] = F(F(mu[i] - h) - pad), F(F(mu[i] + h) + pad)
    return lo, hi


def quad_t(mu, q, o, d, fma):
    """near_collect's plane depth of the quad: (n . (mu - o)) / (n . d), n = third column of R."""
    n = _rot(q)[:, 2]
    c = np.array([F(mu[i] - o[i]) for i in range(3)], F)
    return F(_dot3(n, c, fma) / _dot3(n, d, fma))


def box_tn_tf(lo, hi, o, d):
    """near_collect's slab test of a node's child box: (tn, tf)."""
    inv = np.array([F(F(1) / d[i]) for i in range(3)], F)
    t0 = np.array([F(F(lo[i] - o[i]) * inv[i]) for i in range(3)], F)
    t1 = np.array([F(F(hi[i] - o[i]) * inv[i]) for i in range(3)], F)
    return F(np.max(np.minimum(t0, t1))), F(np.min(np.maximum(t0, t1)))


def search(n_rays=400, seed=0, scale=0.02, op=0.6):
    """Rays and axis-aligned quads (normal z) whose plane depth lies within a few ulps of a slab border.  Returns a list of cases
    (o, d, mu, border, t, tf unpadded, tf padded, tn padded), t for both FMA variants (they agree on an axis-aligned quad)."""
    rng = np.random.default_rng(seed)
    out = []
    for B in BORDERS:
        for _ in range(n_rays):
            o = rng.uniform(-0.3, 0.3, 3).astype(F)
            d = np.array([rng.uniform(-0.6, 0.6), rng.uniform(-0.6, 0.6), rng.uniform(0.4, 1.0)])
            d = (d / np.linalg.norm(d)).astype(F)
            z0 = F(o[2] + F(F(B) * d[2]))
            for k in range(-3, 4):
                z = F(z0)
                for _ in range(abs(k)):
                    z = np.nextafter(z, F(np.inf if k > 0 else -np.inf), dtype=F)
                mu = np.array([F(o[0] + F(F(B) * d[0])), F(o[1] + F(F(B) * d[1])), z], F)
                ts = {fma: quad_t(mu, IDENT, o, d, fma) for fma in (False, True)}
                lo0, hi0 = quad_box(mu, (scale, scale), IDENT, op, padded=False)
                lo1, hi1 = quad_box(mu, (scale, scale), IDENT, op, padded=True)
                out.append({"o": o, "d": d, "mu": mu, "B": F(B), "t": ts, "tf0": box_tn_tf(lo0, hi0, o, d)[1],
                            "tn1": box_tn_tf(lo1, hi1, o, d)[0], "tf1": box_tn_tf(lo1, hi1, o, d)[1]})
    return out


def straddles(cases, padded):
    """Cases in which the slab [.., B) excludes the quad (t >= B) while its box does not ask for the next slab (tf < B)."""
    key = "tf1" if padded else "tf0"
    return [c for c in cases if any(t >= c["B"] for t in c["t"].values()) and c[key] < c["B"]]


def straddling_scene(n=64, seed=0):
    """(scene, o (4, n/4, 3), d): per ray one quad on a slab border whose UNPADDED box would straddle it, and one near quad 0.1 m ahead."""
    cases = straddles(search(seed=seed), padded=False)
    rng = np.random.default_rng(seed + 1)
    idx = rng.choice(len(cases), n, replace=len(cases) < n)
    cs = [cases[i] for i in idx]
    o = np.stack([c["o"] for c in cs]).astype(F); d = np.stack([c["d"] for c in cs]).astype(F)
    off = np.array([0.004, -0.003, 0.0], F)              # rays pass a little off the quads' centres (not along a diagonal of the two triangles)
    means = np.concatenate([np.stack([c["mu"] for c in cs]) + off, (o + F(0.1) * d + off).astype(F)]).astype(F)
    P = means.shape[0]
    sc = {"means": means, "scales": np.full((P, 2), 0.02, F), "rotations": np.tile(IDENT, (P, 1)),
          "opacities": np.concatenate([np.full((n, 1), 0.6, F), np.full((n, 1), 0.5, F)]),
          "shs": np.zeros((P, 16, 3), F)}
    sc["shs"][:, 0, :] = rng.uniform(-0.5, 0.5, (P, 3)).astype(F)
    return sc, o.reshape(4, n // 4, 3), d.reshape(4, n // 4, 3)


def test_unpadded_boxes_would_straddle_a_slab_border():
    """The search does reach the borders: with boxes that fit their quads exactly, some quads would be lost (the guard has teeth)."""
    cases = search()
    assert len(straddles(cases, padded=False)) > 0
    assert {float(c["B"]) for c in straddles(cases, padded=False)} >= {1.5, 6.0}


def test_padded_boxes_never_straddle_a_slab_border():
    """With the build's padding every box is entered by the slab that takes its quad and asks for the next one whenever the quad lies
    beyond: tn <= t <= tf with a margin far above the rounding of t, at every border and with either FMA contraction."""
    cases = search()
    assert not straddles(cases, padded=True)
    for c in cases:
        for t in c["t"].values():
            assert c["tn1"] < t and c["tf1"] > t, c
            assert float(c["tf1"]) - float(t) >= 1e-4, (float(c["tf1"]) - float(t), c["B"])      # the pad, in depth units (|d| = 1)
