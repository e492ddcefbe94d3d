"""The per-row gate of the tracer's Gaussian gradients (host only; the GPU cases are tests/test_row_gradients_gpu.py, the negative controls
tests/test_row_gate.py).

A relative L2 error over a gradient tensor is carried by its few largest rows: the last record of one bucket dropped, one axis of `d_scales`
1 % off on a few rows, a sign on the `d_rotations` of some hits or a lost fixup of one run leave it, and the share of elements beyond the
tolerance, where they were.  This gate looks at every Gaussian's row by itself.  Three sets of gradients of the same scene, rays and upstream
gradient enter: an implementation X, the float32 oracle and the float64 oracle.  Per tensor, flattened to (P, k):

    s_g    = max_j |f64[g, j]|                         the size of row g
    T      = max_g s_g                                 the size of the tensor
    e_X(g) = max_j |X[g, j] - f64[g, j]|               the error of row g
    c      = 4 max_g e_f32(g) / T                      the floor: the float32 ORACLE's own worst row (never X's), x 4 for another order of
                                                       summation inside a row (atomics, buckets, the ordered reduction against ray order)

    every row:   e_X(g) <= 1e-3 s_g + c T              (1e-3: the north-star gradient tolerance of BASELINE.json, per row)
    and          X[g, :] has a non-zero  <=>  f64[g, :] has one;  a column that is all-zero in f64 (an inactive SH coefficient) is all-zero in X.

The gate is only worth something where it can see: a row is SENSITIVE when s_g >= 10 c T (losing a tenth of it fails the rule), and at least
70 % of the touched rows of every tensor must be sensitive -- a condition on the reference, asserted, not a measurement.

Two float32 traces cannot agree on every ray (tests/event_gate.py): a ray whose composited sequence differs from the float64 oracle's, or
one of whose output channels 0..4, 8 leaves the float64 output by more than 1e-4 of the channel's scale, is MASKED: its upstream gradient is
zero in all three backwards.  At most 2 % of the rays of a case may be masked.  The hit weights `accum` are sums over ALL rays, which no upstream
gradient switches off: the Gaussians on a masked ray (in any of the three sequences) are left out of the `accum` rows, and counted."""
import numpy as np

from lidar_rt_amd import scenes
from oracle import oracle
from tests.test_oracle_backward import _small_scene

GRADS = ("means", "scales", "rotations", "opacities", "shs")
ROW_TOL = 1e-3            # BASELINE.json north star, gradients
MARGIN = 4.0              # on the float32 oracle's own worst row
SENSITIVE = 10.0          # a row is sensitive from 10 c T
MIN_SENSITIVE = 0.70
OUT_TOL = 1e-4
MAX_MASKED = 0.02
OUT_CH = [0, 1, 2, 3, 4, 8]
TRACE_CAP = 192
BG3 = ((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.3, 0.7, 0.2))


def rows(x, P):
    return np.asarray(x, np.float64).reshape(P, -1)


def row_stats(f32, f64):
    """(s_g, T, c, touched, sensitive) of one tensor, from the two oracles alone."""
    P = np.asarray(f64).shape[0]
    r64 = rows(f64, P); r32 = rows(f32, P)
    s = np.abs(r64).max(1)
    T = float(s.max())
    c = MARGIN * float(np.abs(r32 - r64).max(1).max()) / T if T > 0 else 0.0
    touched = (r64 != 0).any(1)
    return s, T, c, touched, touched & (s >= SENSITIVE * c * T)


def gate_tensor(x, f32, f64, skip=None):
    """The rule on one tensor -> (record, list of failures).  skip: rows left out (the `accum` rows on masked rays)."""
    P = np.asarray(f64).shape[0]
    rx, r64 = rows(x, P), rows(f64, P)
    assert rx.shape == r64.shape, (rx.shape, r64.shape)
    s, T, c, touched, sens = row_stats(f32, f64)
    use = np.ones(P, bool) if skip is None else ~np.asarray(skip, bool)
    bad = []
    if not np.isfinite(rx).all():
        bad.append(("not finite", int((~np.isfinite(rx)).any(1).sum()), int(np.nonzero((~np.isfinite(rx)).any(1))[0][0])))
        rx = np.nan_to_num(rx, nan=np.inf)
    e = np.abs(rx - r64).max(1)
    allow = ROW_TOL * s + c * T
    ratio = np.where(allow > 0, e / np.where(allow > 0, allow, 1.0), np.where(e > 0, np.inf, 0.0))
    out = use & (e > allow)
    if out.any():
        g = int(np.argmax(np.where(out, ratio, -1.0)))
        bad.append(("rows outside 1e-3 s + c T", int(out.sum()), {"row": g, "e": float(e[g]), "s": float(s[g]), "cT": c * T, "x": rx[g].tolist(), "f64": r64[g].tolist()}))
    nzx = (rx != 0).any(1)
    diff = use & (nzx != touched)
    if diff.any():
        bad.append(("rows with another zero pattern", int(diff.sum()), {"x_only": np.nonzero(diff & nzx)[0][:8].tolist(), "f64_only": np.nonzero(diff & touched)[0][:8].tolist()}))
    dead = ~(r64 != 0).any(0)
    if touched.any() and (rx[use][:, dead] != 0).any():
        bad.append(("non-zero in a column that is zero in the reference", int((rx[use][:, dead] != 0).sum()), np.nonzero(dead)[0][:8].tolist()))
    n_t = int((touched & use).sum())
    share = float((sens & use).sum() / n_t) if n_t else 0.0
    if share < MIN_SENSITIVE:
        bad.append(("blind: sensitive share of the touched rows below 70 %", share, n_t))
    rec = {"c": c, "T": T, "worst": float(ratio[use].max()) if use.any() else 0.0, "sensitive": share, "touched": n_t}
    return rec, bad


def check(case, path, x, f32, f64, accum_skip=None, report=None):
    """x / f32 / f64: {"means", "scales", "rotations", "opacities", "shs", "accum"}.  Prints one ROWGRAD line per tensor, asserts the rule."""
    failures = []
    for k in GRADS + ("accum",):
        rec, bad = gate_tensor(x[k], f32[k], f64[k], accum_skip if k == "accum" else None)
        line = f"ROWGRAD|{case}|{path}|{k}|{rec['c']:.3e}|{rec['worst']:.3f}|{rec['sensitive']:.3f}"
        print(line)
        if report is not None:
            report.append(line)
        failures += [(k,) + b for b in bad]
    assert not failures, (case, path, failures)


def accepted(x, f32, f64, accum_skip=None):
    """The rule as a predicate (the negative controls): the tensors that refuse x."""
    return [k for k in GRADS + ("accum",) if gate_tensor(x[k], f32[k], f64[k], accum_skip if k == "accum" else None)[1]]


# ---------------------------------------------------------------------------------------------------------------------------------------
# scenes
def scene(P, H, W, seed, variant=None, M=None):
    """tests.test_oracle_backward._small_scene with gradient on the D2 / D3 channels too, and the variants of the deep scene."""
    sc, o, d, dL = _small_scene(P, H, W, seed)
    dL[..., 4:9] = np.random.default_rng(seed + 1000).normal(size=(H, W, 5)) / 8
    if variant == "by-distance":          # the near, heavily hit Gaussians share buckets
        order = np.argsort(np.linalg.norm(sc["means"], axis=1), kind="stable")
        sc = {k: np.ascontiguousarray(v[order]) for k, v in sc.items()}
    elif variant == "unhittable":         # alpha <= 0.003 < 1/255: never composited
        sc["opacities"] = sc["opacities"].copy(); sc["opacities"][::5] = 0.003
    if M is not None:
        have = sc["shs"].shape[1]
        extra = np.random.default_rng(seed + 2000).normal(size=(sc["shs"].shape[0], max(M - have, 0), 3)) * 0.1
        sc["shs"] = np.ascontiguousarray(np.concatenate([sc["shs"], extra], 1)[:, :M])
    # what the GPU is given is float32: the oracles see exactly those numbers
    sc = {k: np.asarray(v, np.float32).astype(np.float64) for k, v in sc.items()}
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)
    return sc, f(o), f(d), f(dL)


SCENES = {"p570": (600, 6, 24, 7, None), "p585-ragged": (600, 5, 37, 8, None), "deep": (2000, 8, 64, 9, None),
          "deep-by-distance": (2000, 8, 64, 9, "by-distance"), "deep-unhittable": (2000, 8, 64, 9, "unhittable")}


def s10k_case(cols=None):
    sc, o, d = scenes.s10k()
    dL = scenes.upstream_grad(16, 256).astype(np.float64)
    dL[..., 4:9] = np.random.default_rng(5).normal(size=(16, 256, 5)).astype(np.float32) / 4096          # as tests/test_hip_parity.s10k
    if cols is not None:
        o, d, dL = o[:, :cols], d[:, :cols], dL[:, :cols]
    f = lambda a: np.ascontiguousarray(np.asarray(a, np.float32).astype(np.float64))
    return {k: f(v) for k, v in sc.items()}, f(o), f(d), f(dL)


class Reference:
    """Both oracles of one case: outputs, hit weights, composited sequences; the backwards per ray mask (computed once per mask)."""

    def __init__(self, sc, o, d, dL, deg, bg, mod=1.0):
        from tests.event_gate import trace_sequences
        self.sc, self.o, self.d, self.dL, self.deg, self.bg, self.mod = sc, o, d, np.asarray(dL, np.float64), deg, np.asarray(bg, np.float64), mod
        self.H, self.W = o.shape[:2]; self.HW = self.H * self.W
        self.P = sc["means"].shape[0]
        self.out, self.accum, self.seq, self.trunc = {}, {}, {}, {}
        for prec in ("f32", "f64"):
            orc = self._oracle(prec)
            tr = orc.forward_trace(o, d, sc["shs"], deg, self.bg, cap=TRACE_CAP)
            fw = orc.forward(o, d, sc["shs"], deg, self.bg)
            np.testing.assert_array_equal(tr["out"], fw["out"])
            self.out[prec] = np.asarray(fw["out"], np.float64); self.accum[prec] = np.asarray(fw["accum"], np.float64).reshape(-1, 1)
            self.seq[prec], self.trunc[prec] = trace_sequences(tr, self.HW, TRACE_CAP)
        self.scale = np.abs(self.out["f64"].reshape(-1, 9)[:, OUT_CH]).max(0) + 1e-12
        self.scale[:3] = self.scale[:3].max()               # one scale for the three colour channels (tests/test_ray_grads_gpu._check_against_dense)
        self._bw = {}
        # the float32 oracle's own event rays: the yardstick of how many a float32 trace may have
        self.f32_events = self.event_rays(self.out["f32"], self.seq["f32"])

    def _oracle(self, prec):
        return oracle.Oracle(self.sc["means"], self.sc["scales"], self.sc["rotations"], self.sc["opacities"], prec, self.mod)

    def output_edges(self, out):
        e = np.abs(np.asarray(out, np.float64).reshape(-1, 9)[:, OUT_CH] - self.out["f64"].reshape(-1, 9)[:, OUT_CH]) / self.scale
        return (e > OUT_TOL).any(1)

    def sequence_events(self, seqs):
        same = lambda a, b: len(a) == len(b) and np.array_equal(np.asarray(a, np.int64), np.asarray(b, np.int64))
        return np.array([not same(seqs[r], self.seq["f64"][r]) for r in range(self.HW)]) | self.trunc["f64"]

    def event_rays(self, out, seqs):
        return self.output_edges(out) | self.sequence_events(seqs)

    def masked_dL(self, mask):
        dLm = self.dL.reshape(self.HW, 9).copy(); dLm[mask] = 0.0
        return dLm.reshape(self.H, self.W, 9)

    def backward(self, mask):
        """{"f32", "f64"} -> gradients + accum, for the upstream gradient with the rays of `mask` zeroed."""
        key = np.packbits(mask).tobytes()
        if key not in self._bw:
            dLm = self.masked_dL(mask)
            res = {}
            for prec in ("f32", "f64"):
                g = self._oracle(prec).backward(self.o, self.d, self.sc["shs"], self.deg, self.bg, self.out[prec], dLm)
                res[prec] = {k: np.asarray(v, np.float64) for k, v in g.items()}
                res[prec]["accum"] = self.accum[prec]
            self._bw[key] = res
        return self._bw[key]

    def accum_skip(self, mask, seqs_x=None):
        skip = np.zeros(self.P, bool)
        for r in np.nonzero(mask)[0]:
            for s in (self.seq["f32"][r], self.seq["f64"][r]) + ((seqs_x[r],) if seqs_x is not None else ()):
                skip[np.asarray(s, np.int64)] = True
        return skip
