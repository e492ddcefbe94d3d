"""Shared by tests/test_fused_adam.py and tests/test_fused_adam_gpu.py: the seeded inputs, the float64 yardstick run and the accuracy gate.

Inputs (the operator's contract for its tests): a gradient is exactly 0 or has a magnitude in [1e-6, 1e2], so (1 - beta2) g^2 stays a normal
float32 and nothing depends on how denormals are treated; moments start at zero or come from earlier steps of the same test.

The gate: per tensor (parameter, exp_avg, exp_avg_sq) the LARGEST distance from the float64 twin over all elements of all groups, each
element's distance counted in float32 ulps of the twin's value.  exp_avg and the parameter are sums of terms of both signs: where they cancel,
the value's own ulp says nothing about an error that its terms brought along (both float32 paths are then "hundreds of ulps" off, by luck of the
draw), so for these two the ulp is that of the sum of the terms' magnitudes, which the twin carries along (A_m: the exp_avg recursion on |g|;
A_p: |p0| plus the |update| of every step) -- the value's own ulp wherever nothing cancelled.  The operator's distance may be at most 2 x that
of the float32 torch path on the same inputs, with a floor of one ulp: a float32 result cannot be asked to lie nearer to the float64 value than
its own spacing."""
import numpy as np
import torch

from lidar_rt_amd import optim

SHAPES = ((3,), (1, 3), (15, 3), (1,), (2,), (4,))                       # xyz, f_dc, f_rest, opacity, scaling, rotation
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
LRS = (1.6e-4, 2.5e-3, 1.25e-4, 5e-2, 5e-3, 1e-3)                         # training_setup's, extent 1
EPS = 1e-15
BETAS = (0.9, 0.999)


def gradient(shape, rng):
    """Signed, log-uniform magnitudes in [1e-6, 1e2]; one element in ten is exactly 0."""
    g = 10.0 ** rng.uniform(-6, 2, shape) * rng.choice([-1.0, 1.0], shape)
    g[rng.uniform(size=shape) < 0.1] = 0.0
    return g.astype(np.float32)


def values(P, seed):
    """The six parameter tensors of P Gaussians (float32 numpy)."""
    rng = np.random.default_rng(1000 * seed + P)
    return [rng.standard_normal((P,) + s).astype(np.float32) for s in SHAPES]


def gradients(P, seed, n_steps):
    rng = np.random.default_rng(7000 * seed + P + 1)
    return [[gradient((P,) + s, rng) for s in SHAPES] for _ in range(n_steps)]


def leaf(a, device, offset=False):
    """A leaf tensor holding ``a``; ``offset``: a view that starts one float into its storage (no 16-byte alignment)."""
    t = torch.as_tensor(a, device=device)
    if offset:
        buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=device)
        buf[1:] = t.reshape(-1)
        t = buf[1:].view(t.shape)
        assert t.is_contiguous() and t.data_ptr() % 16 != 0
    else:
        t = t.clone()
    return t.detach().requires_grad_(True)


def groups_of(params):
    return [{"params": [p], "lr": lr, "name": n} for p, lr, n in zip(params, LRS, NAMES)]


def ulp32(x64: np.ndarray) -> np.ndarray:
    """Spacing of float32 at |x| (that of the smallest normal below it), float64."""
    return np.spacing(np.maximum(np.abs(x64), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)


def _np64(x):
    return x.detach().double().cpu().numpy() if torch.is_tensor(x) else np.asarray(x, np.float64)


def distance(got, twin, scale=None) -> float:
    """Largest |got - twin| over the elements, in float32 ulps of the twin's value (``scale``: of that magnitude, where it is larger)."""
    got, twin = _np64(got), _np64(twin)
    if twin.size == 0:
        return 0.0
    ref = np.abs(twin) if scale is None else np.maximum(np.abs(twin), _np64(scale))
    return float(np.max(np.abs(got - twin) / ulp32(ref)))


def bound(yard: float) -> float:
    return max(2.0 * yard, 1.0)


class Twin:
    """The float64 run: ``optim.adam_reference`` on float64 copies, step after step."""

    def __init__(self, params, moments=None, step0=0):
        self.p = [p.detach().double().clone() for p in params]
        self.m = [torch.zeros_like(p) for p in self.p] if moments is None else [m.detach().double().clone() for m, _ in moments]
        self.v = [torch.zeros_like(p) for p in self.p] if moments is None else [v.detach().double().clone() for _, v in moments]
        self.t = [float(step0)] * len(self.p)
        self.A_p = [p.abs() for p in self.p]                   # the sums of the magnitudes of the terms (see the module text)
        self.A_m = [m.abs() for m in self.m]

    def step(self, grads, rows=None, lrs=LRS):
        for k, g in enumerate(grads):
            if g is None:
                continue
            self.t[k] += 1.0
            p0 = self.p[k]
            self.p[k], self.m[k], self.v[k] = optim.adam_reference(self.p[k], g, self.m[k], self.v[k], step=self.t[k], lr=lrs[k], betas=BETAS, eps=EPS, rows=rows)
            a_m = BETAS[0] * self.A_m[k] + (1.0 - BETAS[0]) * torch.as_tensor(g).to(p0).abs()
            self.A_m[k] = a_m if rows is None else torch.where(optim._row_flags(rows.to(p0.device), p0), a_m, self.A_m[k])
            self.A_p[k] = self.A_p[k] + (self.p[k] - p0).abs()


def set_grads(params, grads, offset=False):
    for p, g in zip(params, grads):
        p.grad = None if g is None else (leaf(g, p.device, offset).detach() if offset else torch.as_tensor(g, device=p.device).clone())


def state_of(opt, params):
    return [(opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) for p in params]


def distances(opt, params, twin):
    """(parameter, exp_avg, exp_avg_sq): the largest distance over all groups."""
    st = state_of(opt, params)
    return (max(distance(p, t, a) for p, t, a in zip(params, twin.p, twin.A_p)), max(distance(s[0], t, a) for s, t, a in zip(st, twin.m, twin.A_m)),
            max(distance(s[1], t) for s, t in zip(st, twin.v)))
