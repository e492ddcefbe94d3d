"""The ray-gradient half of lidar_rt_amd/csrc/lrt_math.h (lrt_hit_ray_backward, lrt_sh_basis_vjp), compiled for the host
(tests/host_check/ray_grad_check.cpp), against float64 autograd: per hit, per basis vector, and summed per ray on a small scene
against autograd of the dense forward through ray_o / ray_d."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import dense_torch
from tests.test_oracle_backward import _small_scene

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_check", "ray_grad_check.cpp")
LIB = os.path.join(HERE, "host_check", "libray_grad_check.so")


@pytest.fixture(scope="module")
def rg():
    hdr = os.path.join(HERE, "..", "lidar_rt_amd", "csrc", "lrt_math.h")
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", LIB, SRC])
    return C.CDLL(LIB)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _random_hits(n, seed):
    """n random hits: rotations, scales, scale modifiers, a non-unit direction at oblique incidence (|n.d| / |d| in [0.15, 1])."""
    rng = np.random.default_rng(seed)
    hits = []
    while len(hits) < n:
        q = rng.normal(size=4) * rng.uniform(0.5, 2.0)
        R = dense_torch.rotmat(torch.tensor(q)).numpy()
        nrm = R[:, 2]
        d = rng.normal(size=3); d *= rng.uniform(0.3, 3.0) / np.linalg.norm(d)
        if abs(nrm @ d) / np.linalg.norm(d) < 0.15:
            continue
        o = rng.normal(size=3) * 5.0
        sc = rng.uniform(0.05, 0.6, size=2)
        mod = rng.choice([1.0, 0.7, 1.4])
        t0 = rng.uniform(1.0, 30.0) / np.linalg.norm(d)
        # the mean lies near the ray: the hit point is within ~1.5 sigma of it in the quad's plane
        off = R[:, 0] * sc[0] * mod * rng.normal() + R[:, 1] * sc[1] * mod * rng.normal()
        mu = o + t0 * d - off + nrm * rng.normal() * 0.1
        hits.append(dict(o=o, d=d, mu=mu, sc=sc, q=q, mod=mod, dG=rng.normal(), dD=rng.normal()))
    return hits


def _hit_autograd(h):
    o = torch.tensor(h["o"], requires_grad=True); d = torch.tensor(h["d"], requires_grad=True)
    mu, sc, q = (torch.tensor(h[k]) for k in ("mu", "sc", "q"))
    R = dense_torch.rotmat(q)
    n = R[:, 2]
    t = (n * (mu - o)).sum() / (n * d).sum()
    x = o + t * d
    pm = x - mu
    u = (pm * R[:, 0]).sum() / (h["mod"] * sc[0]); v = (pm * R[:, 1]).sum() / (h["mod"] * sc[1])
    G = torch.exp(-0.5 * (u * u + v * v))
    (h["dG"] * G + h["dD"] * t).backward()
    return t.item(), np.concatenate([o.grad.numpy(), d.grad.numpy()])


def test_hit_ray_backward_matches_autograd(rg):
    got, ref = [], []
    for h in _random_hits(3000, seed=3):
        t, want = _hit_autograd(h)
        out = np.zeros(6, np.float32)
        rg.rg_hit(_p(_f32(h["o"])), _p(_f32(h["d"])), C.c_float(t), _p(_f32(h["mu"])), _p(_f32(h["sc"])), _p(_f32(h["q"])),
                  C.c_float(h["mod"]), C.c_float(h["dG"]), C.c_float(h["dD"]), _p(out))
        got.append(out); ref.append(want)
    got, ref = np.array(got, np.float64), np.array(ref)
    for sl in (slice(0, 3), slice(3, 6)):
        rel = np.linalg.norm(got[:, sl] - ref[:, sl]) / np.linalg.norm(ref[:, sl])
        assert rel <= 1e-4, rel
    # and hit by hit, against the size of that hit's gradient
    per = np.linalg.norm(got - ref, axis=1) / (np.linalg.norm(ref, axis=1) + 1e-12)
    assert np.quantile(per, 0.99) <= 1e-4, np.quantile(per, 0.99)


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_sh_basis_vjp_matches_autograd(rg, deg):
    rng = np.random.default_rng(10 + deg)
    nb = (deg + 1) ** 2
    if deg == 0:      # the constant band: no gradient
        out = np.ones(3, np.float32)
        rg.rg_sh_vjp(0, _p(_f32([0.3, -1.0, 2.0])), _p(_f32(rng.normal(size=16))), _p(out))
        assert np.all(out == 0)
        return
    got, ref = [], []
    for _ in range(1000):
        d = rng.normal(size=3) * rng.uniform(0.2, 5.0)
        g = rng.normal(size=16); g[nb:] = 0.0
        dt = torch.tensor(d, requires_grad=True)
        (dense_torch.sh_basis(deg, dt) * torch.tensor(g[:nb])).sum().backward()
        out = np.zeros(3, np.float32)
        rg.rg_sh_vjp(deg, _p(_f32(d)), _p(_f32(g)), _p(out))
        got.append(out); ref.append(dt.grad.numpy())
    got, ref = np.array(got, np.float64), np.array(ref)
    assert np.linalg.norm(got - ref) / np.linalg.norm(ref) <= 1e-4


@pytest.mark.parametrize("bg", [(0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.3, 0.7, 0.2)])
@pytest.mark.parametrize("deg", [0, 3])
def test_per_ray_sum_matches_autograd_of_the_dense_forward(rg, bg, deg):
    sc, o, d, dL = _small_scene()
    H, W = o.shape[:2]
    P, M = sc["means"].shape[0], sc["shs"].shape[1]
    out9 = np.zeros((H * W, 9), np.float32)
    go = np.zeros((H * W, 3), np.float32); gd = np.zeros((H * W, 3), np.float32)
    rg.rg_trace(P, _p(_f32(sc["means"])), _p(_f32(sc["scales"])), _p(_f32(sc["rotations"])), _p(_f32(sc["opacities"][:, 0])),
                C.c_float(1.0), H * W, _p(_f32(o.reshape(-1, 3))), _p(_f32(d.reshape(-1, 3))), M, deg, _p(_f32(sc["shs"])),
                _p(_f32(bg)), _p(_f32(dL.reshape(-1, 9))), _p(out9), _p(go), _p(gd))

    t = {k: torch.tensor(v) for k, v in sc.items()}
    ro = torch.tensor(o.reshape(-1, 3), requires_grad=True); rd = torch.tensor(d.reshape(-1, 3), requires_grad=True)
    out = dense_torch.render(ro, rd, t["means"], t["scales"], t["rotations"], t["opacities"][:, 0], t["shs"], deg,
                             torch.tensor(bg), 2.0)
    (out * torch.tensor(dL).reshape(-1, 9)).sum().backward()
    ref = out.detach().numpy().copy(); ref[:, :3] -= ref[:, 8:9] * np.array(bg)     # the host forward counts the background once
    assert np.abs(out9 - ref).max() <= 1e-4 * np.abs(ref).max()
    for got, want in ((go, ro.grad.numpy()), (gd, rd.grad.numpy())):
        assert np.abs(want).max() > 0
        rel = np.linalg.norm(got - want) / np.linalg.norm(want)
        assert rel <= 1e-4, rel
