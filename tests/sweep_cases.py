"""The cases of the sweep-ray tests (tests/test_sweep_rays.py, tests/test_sweep_rays_gpu.py) and their float64 reference, computed once per case.

A case: F poses with a rotation and a translation of about 1 km, a twist kind, an inclination kind, a convention, a tau kind and random upstream
gradients.  ``reference(case)`` is the twin's rays, float64 autograd of the twin for those gradients, and ``A``: the sum over the rays of the
absolute per-ray contributions to each of the 18 gradient entries of a frame.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import torch

from lidar_rt_amd import sweep as sw

SIZES = [(1, 1), (3, 70), (5, 37), (64, 256), (66, 1030)]      # below a wave, a ragged last workgroup, several workgroups, the KITTI-360 shape
FRAMES = [1, 3]
INCS = ["bounds", "table"]
CONVENTIONS = ["kitti", "waymo_yaw"]
TWISTS = ["none", "zero", "below", "above", "large", "wide"]
TAUS = ["default", "explicit"]
KITTI_INC = (-0.4363323, 0.0349066)                             # -25 deg .. +2 deg


def _rot(phi):
    phi = np.asarray(phi, np.float64)
    t = np.linalg.norm(phi)
    K = np.array([[0, -phi[2], phi[1]], [phi[2], 0, -phi[0]], [-phi[1], phi[0], 0]])
    return np.eye(3) + np.sin(t) / t * K + (1 - np.cos(t)) / t ** 2 * (K @ K)


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def make(H, W, F, inc="bounds", conv="kitti", twist="large", tau="default", seed=0):
    rng = np.random.default_rng(1000 * H + 10 * W + F + seed)
    pose = np.zeros((F, 3, 4))
    for f in range(F):
        pose[f, :, :3] = _rot(_unit(rng) * rng.uniform(0.3, 2.5))
        pose[f, :, 3] = np.array([812.3, -655.1, 37.4]) + rng.normal(size=3) * 5.0
    if tau == "default":
        tau_arr = None
        tmax = float(sw.column_times(W).to(torch.float32).abs().max()) or 0.5    # one column: tau = 0, every twist gives the pose itself
    else:
        tau_arr = rng.uniform(-0.7, 0.7, size=W).astype(np.float32)              # not monotonic
        tau_arr[rng.integers(W)] = 0.7
        tmax = 0.7
    th = np.sqrt(sw.SERIES_TH2)
    xi = None
    if twist != "none":
        xi = np.zeros((F, 6))
        for f in range(F):
            if twist == "below":                                                # every column's |tau phi| below the threshold, the outermost just
                xi[f] = np.concatenate([_unit(rng) * 1.5, _unit(rng) * th * (1 - 1e-6) / tmax])
            elif twist == "above":                                              # the outermost columns just above it
                xi[f] = np.concatenate([_unit(rng) * 1.5, _unit(rng) * th * (1 + 1e-3) / tmax])
            elif twist == "large":
                xi[f] = np.concatenate([_unit(rng) * 3.0, _unit(rng) * 0.5])
            elif twist == "wide":                                               # most columns in the closed branch
                xi[f] = np.concatenate([_unit(rng) * 3.0, _unit(rng) * 2.5])
    if inc == "bounds":
        inclination = list(KITTI_INC)
    else:
        inclination = np.sort(rng.uniform(-0.31, 0.04, size=H)).astype(np.float32).tolist()
        if H == 2:
            inclination = [-0.3, 0.04]
    kw = dict(H=H, W=W, inclination=inclination, data_type="KITTI", sensor2ego=None, tau=tau_arr)
    if conv == "waymo_yaw":
        s2e = np.eye(4, dtype=np.float32)
        s2e[:3, :3] = _rot([0.0, 0.0, 0.7]).astype(np.float32)
        kw.update(data_type="Waymo", sensor2ego=torch.tensor(s2e))
    n = (F, H, W, 3)
    return SimpleNamespace(key=f"{H}x{W}_F{F}_{inc}_{conv}_{twist}_{tau}", F=F, H=H, W=W, kw=kw, twist_kind=twist,
                           pose=torch.tensor(pose, dtype=torch.float32), twist=None if xi is None else torch.tensor(xi, dtype=torch.float32),
                           g_o=torch.tensor(rng.normal(size=n), dtype=torch.float32), g_d=torch.tensor(rng.normal(size=n), dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def case(H, W, F, inc="bounds", conv="kitti", twist="large", tau="default"):
    return make(H, W, F, inc, conv, twist, tau)


def all_cases():
    """Every size with every twist kind; F, the inclination, the convention and tau rotate so that every value of each meets every size."""
    out = []
    for i, (H, W) in enumerate(SIZES):
        for j, tw in enumerate(TWISTS):
            k = i + j
            out.append(case(H, W, FRAMES[k % 2], INCS[(k // 2 + j) % 2], CONVENTIONS[(i + j // 2) % 2], tw, TAUS[(k + j // 3) % 2]))
    return out


def all_cases_small():
    return [c for c in all_cases() if c.H * c.W <= 64 * 256]


_REF = {}


def reference(c):
    """The twin on a case, once: o, d (F, H, W, 3) float64; d_pose (F, 3, 4), d_twist (F, 6) float64 autograd; A (F, 18); scale (of the origins)."""
    r = _REF.get(c.key)
    if r is None:
        pose = c.pose.clone().to(torch.float64).requires_grad_(True)
        twist = None if c.twist is None else c.twist.clone().to(torch.float64).requires_grad_(True)
        o, d = sw.sweep_rays_reference(pose, twist, **c.kw)
        ((o * c.g_o.to(torch.float64)).sum() + (d * c.g_d.to(torch.float64)).sum()).backward()
        _, _, contrib = sw.sweep_rays_reference(c.pose, c.twist, **c.kw, per_ray=True, g_o=c.g_o, g_d=c.g_d)
        scale = max(1.0, float(c.pose[:, :, 3].abs().max()) + (0.0 if c.twist is None else float(c.twist[:, :3].abs().max())))
        r = SimpleNamespace(o=o.detach(), d=d.detach(), d_pose=pose.grad.clone(), d_twist=None if twist is None else twist.grad.clone(),
                            A=contrib.abs().sum((1, 2)), total=contrib.sum((1, 2)), scale=scale)
        _REF[c.key] = r
    return r


def ulp32(x32: torch.Tensor) -> torch.Tensor:
    """The spacing of float32 at x32 (float64 tensor)."""
    return torch.from_numpy(np.spacing(np.abs(x32.detach().cpu().numpy().astype(np.float32))).astype(np.float64))


def forward_excess(got32, ref64, scale):
    """max of |got - float32(ref)| - (ulp32(float32(ref)) + 2^-45 scale): not positive when the forward bound holds."""
    r32 = ref64.detach().cpu().to(torch.float32)
    err = (got32.detach().cpu().to(torch.float64) - r32.to(torch.float64)).abs()
    return float((err - (ulp32(r32) + 2.0 ** -45 * scale)).max())


def backward_excess(got, ref64, A):
    """max of |got - ref| - (2^-23 |ref| + 2^-34 A): not positive when the backward bound holds."""
    ref64, A = ref64.detach().cpu().reshape(-1), A.detach().cpu().reshape(-1)
    err = (got.detach().cpu().to(torch.float64).reshape(-1) - ref64).abs()
    return float((err - (2.0 ** -23 * ref64.abs() + 2.0 ** -34 * A)).max())
