"""Ray gradients (lrt_backward_rays; `Tracer` with ray_o / ray_d that require grad) on every backward path, against float64 autograd
of the dense forward (tests/dense_torch.py with the background counted twice, D1), and the properties the feature promises: the
Gaussian gradients, outputs and weights do not change, repeated backwards give the same bits, no ray gradient is computed unless asked
for, an expanded origin receives the sum, the sharded tracer refuses."""
import numpy as np
import pytest
import torch

from lidar_rt_amd import scenes
from lidar_rt_amd.diff_lidar_tracer import Tracer
from tests import dense_torch
from tests.test_oracle_backward import _small_scene

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tests.hip_util import settings, rel_l2, DEV, DEFAULT_OPTS
    from tests.test_hip_parity import _facing

GRADS = ("means", "scales", "rotations", "opacities", "shs")
# (options, Tracer arguments, steps, what runs): as tests/test_deferred_accum_gpu.PATHS, plus the packet forward behind the default
# backward (no colour record: re-trace), the deterministic and deferred-weight options and the speculative backward (2nd step)
PATHS = [({}, {}, 1, "bucketed"), ({"bwd_mode": 0}, {}, 1, "re-trace"),
         ({"hit_cap": 8, "hit_cap_auto": 0}, {}, 1, "record overflow -> re-trace"), ({"c4_waves": 16}, {}, 1, "16 waves"),
         ({"fwd_mode": 0, "bwd_mode": 0}, {}, 1, "packet kernel both ways"), ({"fwd_mode": 0}, {}, 1, "packet forward"),
         ({}, {"deterministic": True}, 1, "deterministic"), ({}, {"deferred_accum": True}, 1, "deferred_accum"),
         ({}, {}, 2, "speculative backward")]


def _run(sc, o, d, deg, bg, dL, opts=None, tracer_kw=None, steps=1, want_rays=True, twice=False, expand_o=False):
    tr = Tracer(**(tracer_kw or {}))
    for k, v in {**DEFAULT_OPTS, "hit_cap_auto": 1, **(opts or {})}.items():
        tr.optix_context.set_option(k, v)
    for k in ("deterministic", "deferred_accum"):
        tr.optix_context.set_option(k, 1 if getattr(tr, k) else 0)          # the state is per device: reset what an earlier run set
    t = {k: torch.as_tensor(np.asarray(v, np.float32), device=DEV).requires_grad_(True) for k, v in sc.items()}
    H, W = o.shape[:2]
    for _ in range(steps):
        for v in t.values():
            v.grad = None
        if expand_o:
            src = torch.as_tensor(np.asarray(o[0, 0], np.float32), device=DEV).requires_grad_(want_rays)
            ro = src.expand(H, W, 3)
        else:
            ro = torch.as_tensor(np.asarray(o, np.float32), device=DEV).requires_grad_(want_rays)
        rd = torch.as_tensor(np.asarray(d, np.float32), device=DEV).requires_grad_(want_rays)
        tr.build_from_gaussians(t["means"], t["scales"], t["rotations"], t["opacities"])
        out, acc = tr(ro, rd, None, t["means"], torch.zeros_like(t["means"]), shs=t["shs"], opacities=t["opacities"],
                      scales=t["scales"], rotations=t["rotations"], tracer_settings=settings(bg, deg))
        g = torch.as_tensor(np.asarray(dL, np.float32), device=DEV)
        out.backward(g, retain_graph=twice)
        res = {"out": out.detach().cpu().numpy(), "accum": acc.detach().cpu().numpy(),
               "grads": {k: t[k].grad.detach().cpu().numpy() for k in GRADS}}
        leaf_o = src if expand_o else ro
        res["ro"] = None if leaf_o.grad is None else leaf_o.grad.cpu().numpy()
        res["rd"] = None if rd.grad is None else rd.grad.cpu().numpy()
        if twice:
            r1 = (res["ro"].copy(), res["rd"].copy())
            leaf_o.grad = None; rd.grad = None
            out.backward(g)
            res["twice"] = (r1, (leaf_o.grad.cpu().numpy(), rd.grad.cpu().numpy()))
    torch.cuda.synchronize()
    return res


def _dense(sc, o, d, deg, bg, dL, batch=256):
    """float64 autograd of the dense forward with the background counted twice: (out (N, 9) counted ONCE, dL/dray_o, dL/dray_d)."""
    t = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in sc.items()}
    o = np.asarray(o, np.float64).reshape(-1, 3); d = np.asarray(d, np.float64).reshape(-1, 3); dL = np.asarray(dL, np.float64).reshape(-1, 9)
    outs, gos, gds = [], [], []
    for i in range(0, o.shape[0], batch):
        ro = torch.tensor(o[i:i + batch], requires_grad=True); rd = torch.tensor(d[i:i + batch], requires_grad=True)
        out = dense_torch.render(ro, rd, t["means"], t["scales"], t["rotations"], t["opacities"][:, 0], t["shs"], deg,
                                 torch.tensor(np.asarray(bg, np.float64)), 2.0)
        (out * torch.tensor(dL[i:i + batch])).sum().backward()
        out = out.detach().numpy().copy(); out[:, :3] -= out[:, 8:9] * np.asarray(bg, np.float64)
        outs.append(out); gos.append(ro.grad.numpy()); gds.append(rd.grad.numpy())
    return np.concatenate(outs), np.concatenate(gos), np.concatenate(gds)


def _check_against_dense(h, ref, what):
    out64, go64, gd64 = ref
    ch = [0, 1, 2, 3, 4, 8]                                     # (5..7: the normals the product writes, D3; not in dense_torch)
    out, out64 = h["out"].reshape(-1, 9)[:, ch], out64[:, ch]
    scale = np.abs(out64).max(0) + 1e-12
    scale[:3] = scale[:3].max()                                 # one scale for the three colour channels (one can be ~0 everywhere)
    edge = (np.abs(out - out64) / scale > 1e-4).any(1)          # knife edges: the fp32 trace took another hit set than the fp64 one
    assert edge.mean() <= 0.02, (what, edge.mean(), (np.abs(out - out64) / scale > 1e-4).mean(0))
    keep = ~edge
    for got, want, name in ((h["ro"], go64, "ray_o"), (h["rd"], gd64, "ray_d")):
        got = got.reshape(-1, 3)
        assert np.abs(want[keep]).max() > 0, (what, name)
        err = rel_l2(got[keep], want[keep])
        assert err <= 1e-3, (what, name, err)


@pytest.fixture(scope="module")
def s10k():
    sc, o, d = scenes.s10k()
    dL = scenes.upstream_grad(16, 256)
    return sc, o, d, dL, _dense(sc, o, d, 3, scenes.BG_DEFAULT, dL)


@pytest.mark.parametrize("bg", [(0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.3, 0.7, 0.2)])
@pytest.mark.parametrize("deg", [0, 3])
def test_small_scene_ray_grads_match_float64_autograd(bg, deg):
    sc, o, d, dL = _small_scene()
    ref = _dense(sc, o, d, deg, bg, dL)
    for opts, kw, steps, what in PATHS:
        _check_against_dense(_run(sc, o, d, deg, bg, dL, opts, kw, steps), ref, what)


@pytest.mark.parametrize("opts,kw,steps,what", PATHS, ids=[p[3] for p in PATHS])
def test_s10k_ray_grads_match_float64_autograd(s10k, opts, kw, steps, what):
    sc, o, d, dL, ref = s10k
    _check_against_dense(_run(sc, o, d, 3, scenes.BG_DEFAULT, dL, opts, kw, steps), ref, what)


def test_near_rays_bucketed_equals_retrace():
    """A sensor 0.1 m from a surface: the near-ray replay (stale-slot rule, outside dense_torch) owns those rays' gradients in the
    re-tracing backward, the forward's record in the bucketed one."""
    ang = np.linspace(-0.02, 0.02, 16)
    d = np.stack([np.ones(16), 0.011 + ang, 0.004 + ang[::-1] * 0.5], -1).reshape(1, 16, 3).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.zeros((1, 16, 3), np.float32)
    sc = _facing([0.1] + list(np.linspace(1.0, 9.0, 17)), [0.05] * 18)
    rng = np.random.default_rng(5)
    dL = np.zeros((1, 16, 9), np.float32); dL[..., :4] = rng.normal(size=(1, 16, 4))
    bg = np.zeros(3, np.float32)
    a = _run(sc, o, d, 0, bg, dL, {})
    b = _run(sc, o, d, 0, bg, dL, {"bwd_mode": 0})
    for k in ("ro", "rd"):
        assert np.abs(b[k]).max() > 0
        assert rel_l2(a[k], b[k]) <= 1e-4, (k, rel_l2(a[k], b[k]))


def test_two_backwards_of_one_forward_give_the_same_bits(s10k):
    sc, o, d, dL, _ = s10k
    for opts in ({}, {"bwd_mode": 0}):
        r1, r2 = _run(sc, o, d, 3, scenes.BG_DEFAULT, dL, opts, twice=True)["twice"]
        np.testing.assert_array_equal(r1[0], r2[0]); np.testing.assert_array_equal(r1[1], r2[1])


def test_ray_grads_leave_everything_else_bit_identical(s10k):
    """Under the deterministic option (every other result is then bit-reproducible itself): the same outputs, weights and Gaussian
    gradients with and without ray gradients.  In the re-tracing backward (float atomics) the outputs."""
    sc, o, d, dL, _ = s10k
    a = _run(sc, o, d, 3, scenes.BG_DEFAULT, dL, {}, {"deterministic": True}, want_rays=False)
    b = _run(sc, o, d, 3, scenes.BG_DEFAULT, dL, {}, {"deterministic": True}, want_rays=True)
    assert a["ro"] is None and a["rd"] is None                      # not asked for: no gradient
    assert b["ro"] is not None and b["rd"] is not None
    np.testing.assert_array_equal(a["out"], b["out"]); np.testing.assert_array_equal(a["accum"], b["accum"])
    for k in GRADS:
        np.testing.assert_array_equal(a["grads"][k], b["grads"][k])
    a = _run(sc, o, d, 3, scenes.BG_DEFAULT, dL, {"bwd_mode": 0}, want_rays=False)
    b = _run(sc, o, d, 3, scenes.BG_DEFAULT, dL, {"bwd_mode": 0}, want_rays=True)
    assert a["ro"] is None and b["ro"] is not None
    np.testing.assert_array_equal(a["out"], b["out"])
    for k in GRADS:
        assert rel_l2(a["grads"][k], b["grads"][k]) < 2e-6, k


def test_expanded_origin_receives_the_summed_gradient(s10k):
    sc, o, d, dL, _ = s10k
    dense = _run(sc, o, d, 3, scenes.BG_DEFAULT, dL)
    ex = _run(sc, o, d, 3, scenes.BG_DEFAULT, dL, expand_o=True)
    assert ex["ro"].shape == (3,)
    want = dense["ro"].reshape(-1, 3).astype(np.float64).sum(0)
    np.testing.assert_allclose(ex["ro"], want, rtol=1e-4, atol=1e-6 * np.abs(want).max())
    np.testing.assert_array_equal(ex["rd"], dense["rd"])


def test_sharded_tracer_refuses_ray_gradients():
    from lidar_rt_amd.parallel import ShardedTracer
    sc, o, d, dL = _small_scene()
    st = ShardedTracer(rank=0, world=1)
    f = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=DEV)
    ro = f(o).requires_grad_(True)
    with pytest.raises(ValueError):
        st.forward(ro, f(d), f(sc["means"]), f(sc["scales"]), f(sc["rotations"]), f(sc["opacities"]), f(sc["shs"]), 3,
                   f(scenes.BG_DEFAULT))
