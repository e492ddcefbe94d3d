"""The cases of the beam-ray tests (tests/test_beam_rays.py, tests/test_beam_rays_gpu.py) and their float64 reference, computed once per case.

A case is a case of tests/sweep_cases.py (poses, a twist kind, an inclination kind, random upstream gradients) plus a beam table ``(H, 2)``:
``zero``, ``small`` (|offset| <= 1e-3), ``large`` (|offset| <= 0.3) or ``one_row`` (a single non-zero row).  The inclinations of sweep_cases lie
in [-0.44, 0.04], so the nominal elevation plus an offset of at most 0.3 stays inside (-pi/2, pi/2): a condition on the inputs, asserted in
``make``, not a filter.  ``reference(case)`` is the twin's rays, float64 autograd of the twin, ``A`` (F, 18): the sum over the rays of the
absolute per-ray contributions to the pose and twist gradients of a frame, and ``A_beams`` (H, 2): the same over the frames and columns of a row.
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from lidar_rt_amd import beams as bm
from tests import sweep_cases as sc

SIZES = [(1, 1), (3, 70), (5, 37), (64, 256)]                  # below a wave, a ragged last workgroup, several workgroups
FRAMES = [1, 3]
INCS = ["bounds", "table"]
TWISTS = ["none", "zero", "large"]
TABLES = ["zero", "small", "large", "one_row"]


def table(kind, H, rng):
    t = np.zeros((H, 2), np.float32)
    if kind == "small":
        t = rng.uniform(-1e-3, 1e-3, size=(H, 2)).astype(np.float32)
    elif kind == "large":
        t = rng.uniform(-0.3, 0.3, size=(H, 2)).astype(np.float32)
    elif kind == "one_row":
        t[int(rng.integers(H))] = rng.uniform(0.01, 0.05, size=2).astype(np.float32) * rng.choice([-1.0, 1.0], size=2).astype(np.float32)
    else:
        assert kind == "zero", kind
    return t


@functools.lru_cache(maxsize=None)
def case(H, W, F, inc="bounds", twist="large", tab="small"):
    c = sc.make(H, W, F, inc, "kitti", twist, "default", seed=7)
    rng = np.random.default_rng(100000 + 1000 * H + 10 * W + F + TABLES.index(tab))
    t = table(tab, H, rng)
    incl = np.asarray(c.kw["inclination"], np.float64)
    assert max(abs(float(incl.min())), abs(float(incl.max()))) + float(np.abs(t[:, 0]).max()) < math.pi / 2          # the condition on the inputs
    c.key = f"{c.key}_{tab}"
    c.table_kind = tab
    c.beams = torch.from_numpy(t)
    return c


def all_cases():
    """Every size with every table and every twist kind; F and the inclination rotate so that every value of each meets every size and table."""
    out = []
    for i, (H, W) in enumerate(SIZES):
        for j, tab in enumerate(TABLES):
            for k, tw in enumerate(TWISTS):
                out.append(case(H, W, FRAMES[(i + j + k) % 2], INCS[(i + j + k // 2) % 2], tw, tab))
    return out


def all_cases_small():
    return [c for c in all_cases() if c.H * c.W <= 5 * 37] + [case(64, 256, 1, "table", "large", "large")]


_REF = {}


def reference(c):
    """The twin on a case, once: o, d (F, H, W, 3) float64; d_pose (F, 3, 4), d_twist (F, 6) or None, d_beams (H, 2) float64 autograd;
    A (F, 18), A_beams (H, 2); beams_f, A_beams_f (F, H, 2): one frame's part of d_beams and of A_beams; scale (of the origins)."""
    r = _REF.get(c.key)
    if r is None:
        pose = c.pose.clone().to(torch.float64).requires_grad_(True)
        twist = None if c.twist is None else c.twist.clone().to(torch.float64).requires_grad_(True)
        beams = c.beams.clone().to(torch.float64).requires_grad_(True)
        o, d = bm.beam_rays_reference(pose, twist, beams=beams, **c.kw)
        ((o * c.g_o.to(torch.float64)).sum() + (d * c.g_d.to(torch.float64)).sum()).backward()
        _, _, contrib = bm.beam_rays_reference(c.pose, c.twist, beams=c.beams, **c.kw, per_ray=True, g_o=c.g_o, g_d=c.g_d)
        scale = max(1.0, float(c.pose[:, :, 3].abs().max()) + (0.0 if c.twist is None else float(c.twist[:, :3].abs().max())))
        r = SimpleNamespace(o=o.detach(), d=d.detach(), d_pose=pose.grad.clone(), d_twist=None if twist is None else twist.grad.clone(),
                            d_beams=beams.grad.clone(), A=contrib[..., :18].abs().sum((1, 2)), A_beams=contrib[..., 18:].abs().sum((0, 2)),
                            total=contrib[..., :18].sum((1, 2)), total_beams=contrib[..., 18:].sum((0, 2)), beams_f=contrib[..., 18:].sum(2), A_beams_f=contrib[..., 18:].abs().sum(2),
                            scale=scale)
        _REF[c.key] = r
    return r
