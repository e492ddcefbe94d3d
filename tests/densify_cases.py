"""Shared by tests/test_fused_densify.py and tests/test_fused_densify_gpu.py: the seeded assets of the fused densify-and-prune, built so that
the operator's float32 decisions MUST equal the float64 twin's, and the float32 torch expressions the accuracy gate measures against.

Every decision of the rule (include/lrt_densify.h) compares a computed value with a threshold.  ``build`` draws the rows, then checks on the CPU in
float64 -- with its own numpy restatement of the geometry, not the code under test -- that no row lies within a knife-edge margin of

    big_thr   (max_k exp(scaling_k)),   huge_thr  (the same of every output: the row's own scaling, or scaling - log 1.6 of a split row's children),
    opa_thr   (sigmoid(opacity)):       2^-20 relative -- sixteen times the float32 spacing, which covers expf's and the division's few ulps;
    the six box faces (every box sample of every output):   1e-4 m -- against float32 coordinates of a few metres (ulp 2.4e-7) and children
                                                            whose float32 rounding moves a sample by as much;
    grad_thr  (accum / denom):          2^-20 relative as well, EXCEPT the rows put exactly on it on purpose.  Step 1 is one IEEE float32 division
                                        in the operator and in the twin alike, so rows sit ON the threshold: equal to grad_thr is selected, one
                                        float32 below is not, 0 / 0 is not (NaN -> 0), x / 0 is (+inf -> FLT_MAX).

Offending draws are nudged away (scaling, opacity: shifted by 1e-3; box: the row moved by a few 1e-4 m) and the margins are ASSERTED afterwards."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from lidar_rt_amd import densify as dn

GRAD_THR, BIG_THR, HUGE_THR, OPA_THR = 2e-4, 0.05, 1.0, 0.003
BOX_MIN, BOX_MAX = (-2.0, -1.0, -1.0), (2.0, 1.0, 1.0)
REL_MARGIN = 2.0 ** -20
BOX_MARGIN = 1e-4
MIXES = ("none", "clone", "split", "pruned", "mixed")
EDGE_ROWS = {1: "on the threshold", 2: "one float32 below", 3: "0 / 0", 4: "x / 0"}     # in a "mixed" asset of at least 8 rows


def f32(x):
    return float(np.float32(x))


def rule(size_limit=True, box=False):
    return dn.make_rule(GRAD_THR, BIG_THR, HUGE_THR, OPA_THR, size_limit, BOX_MIN if box else None, BOX_MAX if box else None)


def _rotation64(q):
    q = q.astype(np.float64); q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


def _offsets64(R, sd, noise):
    """R (P, 3, 3), sd (P, S), noise (P, K, 3) -> (P, K, 3): R (sd * noise[:, :, :S]), the third component 0 for S == 2."""
    S = sd.shape[1]
    v = np.zeros(noise.shape, np.float64)
    v[..., :S] = sd[:, None, :] * noise[..., :S].astype(np.float64)
    return np.einsum("pij,pkj->pki", R, v)


def decisions64(c):
    """The quantities every decision compares, in float64 numpy: (g float32, max exp(s), the same of the outputs, sigmoid(opacity), box samples
    (P, slot, sample, 3) or None, hot, big)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.nan_to_num(c.accum.reshape(-1) / c.denom.reshape(-1), nan=0.0)                   # float32 / float32 -> float32
    assert g.dtype == np.float32
    hot = g >= np.float32(GRAD_THR)
    s = c.groups["scaling"].astype(np.float64)
    m = np.exp(s).max(1) if len(s) else np.zeros(0)
    big = m > f32(BIG_THR)
    split = hot & big
    m_out = np.where(split, np.exp(s - math.log(1.6)).max(1) if len(s) else m, m)
    sig = 1.0 / (1.0 + np.exp(-c.groups["opacity"].astype(np.float64).reshape(-1)))
    smp = None
    if c.box_noise is not None and len(s):
        R = _rotation64(c.groups["rotation"])
        xyz = c.groups["xyz"].astype(np.float64)
        child = xyz[:, None, :] + _offsets64(R, np.exp(s), c.split_noise)
        out_xyz = np.where(split[:, None, None], child.astype(np.float32).astype(np.float64), xyz[:, None, :])
        sd_out = np.where(split[:, None], np.exp((s - math.log(1.6)).astype(np.float32).astype(np.float64)), np.exp(s))
        smp = out_xyz[:, :, None, :] + _offsets64(R, sd_out, c.box_noise.reshape(-1, 4, 3)).reshape(-1, 2, 2, 3)
    return g, m, m_out, sig, smp, hot, big


def _near(v, thr):
    return np.abs(v / f32(thr) - 1.0) < 4 * REL_MARGIN


def build(P, seed, mix="mixed", S=2, sh_degree=3, box=False, size_limit=True, moments=True, single=None):
    """A seeded asset in float32 numpy.  mix: what the rows are made to be ("none": nothing selected or pruned; "clone" / "split": every row;
    "pruned": every output marked, so the guard holds the prune back; "mixed": about 10 % clone, 5 % split, 5 % pruned, with EDGE_ROWS);
    single: with mix "none", the one row that is selected (cloned when even, split when odd)."""
    assert mix in MIXES
    rng = np.random.default_rng(100_003 * seed + 17 * P + 3 * S + sh_degree + (1000 if box else 0))
    K = (sh_degree + 1) ** 2 - 1
    lo, hi = np.array(BOX_MIN), np.array(BOX_MAX)
    xyz = (rng.uniform(lo * 1.08, hi * 1.08, (P, 3)) if box else rng.normal(0, 20, (P, 3))).astype(np.float32)
    small = lambda n: rng.uniform(math.log(0.004), math.log(0.04), (n, S))
    large = lambda n: rng.uniform(math.log(0.07), math.log(0.9), (n, S))
    scaling = small(P)
    opacity = rng.uniform(-3.0, 4.0, (P, 1))
    g = rng.uniform(0.0, 0.5, P) * GRAD_THR                                  # cold
    denom = rng.integers(1, 9, P).astype(np.float32)
    hot_g = lambda n: rng.uniform(1.5, 20.0, n) * GRAD_THR
    if mix == "clone":
        g = hot_g(P)
    elif mix == "split":
        g, scaling = hot_g(P), large(P)
    elif mix == "pruned":
        opacity = rng.uniform(-9.0, -7.0, (P, 1))
        u = rng.uniform(size=P)
        g = np.where(u < 0.3, hot_g(P), g)
        scaling = np.where((u < 0.15)[:, None], large(P), scaling)
    elif mix == "mixed":
        u = rng.uniform(size=P)
        cl, sp, pr = u < 0.10, (u >= 0.10) & (u < 0.15), (u >= 0.15) & (u < 0.20)
        g = np.where(cl | sp, hot_g(P), g)
        scaling = np.where(sp[:, None], large(P), scaling)
        kind = rng.integers(0, 3, P)
        opacity = np.where((pr & (kind == 0))[:, None], rng.uniform(-9.0, -6.5, (P, 1)), opacity)
        scaling = np.where((pr & (kind >= 1))[:, None], rng.uniform(math.log(1.1), math.log(3.0), (P, S)), scaling)      # huge; hot ones split into children around the threshold
        g = np.where(pr & (kind == 2), hot_g(P), g)
    if single is not None:
        assert mix == "none" and 0 <= single < P
        g[single] = 5 * GRAD_THR
        if single % 2:
            scaling[single] = math.log(0.3)
    accum = (g * denom).astype(np.float32).reshape(P, 1)
    denom = denom.reshape(P, 1)
    if mix == "mixed" and P >= 8:
        t = np.float32(GRAD_THR)
        accum[1], denom[1] = t, 1.0
        accum[2], denom[2] = np.nextafter(t, np.float32(0)), 1.0
        accum[3], denom[3] = 0.0, 0.0
        accum[4], denom[4] = 1e-3, 0.0
    c = SimpleNamespace(P=P, S=S, K=K, mix=mix, box=box, size_limit=size_limit, rule=rule(size_limit, box))
    c.groups = {"xyz": xyz, "f_dc": rng.standard_normal((P, 1, 3)).astype(np.float32), "f_rest": rng.standard_normal((P, K, 3)).astype(np.float32),
                "opacity": opacity.astype(np.float32), "scaling": scaling.astype(np.float32), "rotation": rng.standard_normal((P, 4)).astype(np.float32)}
    c.moments = None
    if moments:
        c.moments = {n: ((0.01 * rng.standard_normal(t.shape)).astype(np.float32), (1e-4 * rng.uniform(size=t.shape)).astype(np.float32)) for n, t in c.groups.items()}
    c.accum, c.denom = accum, denom
    c.split_noise = rng.standard_normal((P, 2, 3)).astype(np.float32)
    c.box_noise = rng.standard_normal((P, 2, 2, 3)).astype(np.float32) if (box and size_limit) else None
    # nudge the draws off the knife edges, then assert the margins
    for _ in range(40):
        gq, m, m_out, sig, smp, hot, big = decisions64(c)
        bad_s = _near(m, BIG_THR) | _near(m, HUGE_THR) | _near(m_out, HUGE_THR)
        bad_o = _near(sig, OPA_THR)
        bad_x = np.zeros(P, bool)
        if smp is not None:
            d = np.minimum(np.abs(smp - lo), np.abs(smp - hi)).reshape(P, -1).min(1)
            bad_x = d < 2 * BOX_MARGIN
        if not (bad_s.any() or bad_o.any() or bad_x.any()):
            break
        c.groups["scaling"][bad_s] += np.float32(1e-3)
        c.groups["opacity"][bad_o] += np.float32(1e-3)
        c.groups["xyz"][bad_x] += np.float32(7e-4)
    assert_margins(c)
    return c


def assert_margins(c):
    gq, m, m_out, sig, smp, hot, big = decisions64(c)
    rel = lambda v, thr: np.abs(v / f32(thr) - 1.0)
    assert np.all(rel(m, BIG_THR) >= REL_MARGIN) and np.all(rel(m, HUGE_THR) >= REL_MARGIN) and np.all(rel(m_out, HUGE_THR) >= REL_MARGIN), "scaling on a knife edge"
    assert np.all(rel(sig, OPA_THR) >= REL_MARGIN), "opacity on a knife edge"
    edge = np.zeros(c.P, bool)
    if c.mix == "mixed" and c.P >= 8:
        edge[list(EDGE_ROWS)] = True
        assert gq[1] == np.float32(GRAD_THR) and gq[2] < np.float32(GRAD_THR) and gq[3] == 0 and gq[4] > 1e30
        assert hot[1] and not hot[2] and not hot[3] and hot[4]
    assert np.all(rel(gq[~edge].astype(np.float64), GRAD_THR) >= REL_MARGIN), "gradient on a knife edge"
    if smp is not None:
        lo, hi = np.array(BOX_MIN), np.array(BOX_MAX)
        assert np.all(np.abs(smp - lo) >= BOX_MARGIN) and np.all(np.abs(smp - hi) >= BOX_MARGIN), "box sample on a knife edge"


def leaf(a, device, offset=False):
    """A tensor holding ``a``; ``offset``: a view that starts one float into its storage (no 16-byte alignment)."""
    t = torch.as_tensor(a, device=device)
    if not offset:
        return t.clone()
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=device)
    buf[1:] = t.reshape(-1)
    v = buf[1:].view(t.shape)
    assert v.is_contiguous() and (t.numel() == 0 or v.data_ptr() % 16 != 0)
    return v


def tensors(c, device, offset=False):
    """(groups, moments, accum, denom, split_noise, box_noise) of a built case as torch tensors on ``device``."""
    L = lambda a: leaf(a, device, offset)
    return ({n: L(t) for n, t in c.groups.items()}, None if c.moments is None else {n: (L(m), L(v)) for n, (m, v) in c.moments.items()}, L(c.accum), L(c.denom),
            L(c.split_noise), None if c.box_noise is None else L(c.box_noise))


# ---- the float32 torch path of the values the gate covers: the expressions of GaussianAsset.densify_and_prune with the noise given --------------------

def rotation_matrix32(q):
    """training._rotation_matrix, restated."""
    q = q / q.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).view(-1, 3, 3)


def torch_children(xyz, scaling, rotation, split_noise, src, child):
    """(xyz, scaling) of the children (source rows ``src``, child index ``child``) as the torch path forms them in float32: the normal draw is
    std * noise (what torch.normal(0, std) is), offs = bmm(R, draw), xyz + offs, log(exp(scaling) / 1.6)."""
    stds = torch.exp(scaling[src])
    draw = stds * split_noise[src, child, :stds.shape[1]]
    if stds.shape[1] == 2:
        draw = torch.cat([draw, torch.zeros_like(draw[:, :1])], -1)
    offs = torch.bmm(rotation_matrix32(rotation[src]), draw.unsqueeze(-1)).squeeze(-1)
    return offs + xyz[src], torch.log(stds / (0.8 * 2))


def ulp32(x64):
    return np.spacing(np.maximum(np.abs(x64), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)


def distance(got, twin, scale=None):
    """tests/adam_cases.py's: the largest |got - twin| in float32 ulps of |twin| (of ``scale`` where that is larger)."""
    n = lambda x: x.detach().double().cpu().numpy() if torch.is_tensor(x) else np.asarray(x, np.float64)
    got, twin = n(got), n(twin)
    if twin.size == 0:
        return 0.0
    ref = np.abs(twin) if scale is None else np.maximum(np.abs(twin), n(scale))
    return float(np.max(np.abs(got - twin) / ulp32(ref)))


def bound(yard):
    return max(2.0 * yard, 1.0)
