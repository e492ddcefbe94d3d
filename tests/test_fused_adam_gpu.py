"""The fused Adam step on the MI355X (`optim.GaussianAdam` through `liblrt_adam.so`): accuracy against the float64 twin with torch's fused
float32 Adam as the comparison path (tests/adam_cases.py states the gate), the bit-level promises of the row mask, the contract edges, the
training loop under the two switches, a bit-exact resume and the absence of a host wait.

Shapes: P in {1, 5, 255, 256, 257, 1000} (one row, fewer rows than a 16-byte vector of the width-1 group, one row short of a workgroup's 256,
exactly 256, one more, four workgroups with a short last one), the six group shapes of an asset in one call, once with every tensor starting
one float into its storage (the 4-byte path)."""
import io
import types

import numpy as np
import pytest
import torch

from lidar_rt_amd import optim, scenes, training
from tests import adam_cases as ac

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROWS = [1, 5, 255, 256, 257, 1000]
bits = lambda t: t.detach().cpu().numpy().tobytes()


def masks_for(P):
    """name -> row mask (None: the dense call): all ones, all zeros, every other row, a single row at each of 0, 255, 256 and P - 1."""
    m = {"none": None, "ones": torch.ones(P, dtype=torch.bool, device=DEV), "zeros": torch.zeros(P, dtype=torch.bool, device=DEV),
         "every_other": (torch.arange(P, device=DEV) % 2 == 0)}
    for r in sorted({0, 255, 256, P - 1}):
        if r < P:
            one = torch.zeros(P, dtype=torch.uint8, device=DEV); one[r] = 1           # uint8 masks are taken as they are
            m[f"row_{r}"] = one
    return m


def fresh(P, seed, offset, cls=optim.GaussianAdam, step0=0):
    """Parameters and an optimizer over them; ``step0`` = 1000: after one real step (moments from it) the counts are loaded as 1000."""
    params = [ac.leaf(v, DEV, offset) for v in ac.values(P, seed)]
    if cls is torch.optim.Adam:
        opt = torch.optim.Adam(ac.groups_of(params), lr=0.0, eps=ac.EPS, fused=True)
    else:
        opt = optim.GaussianAdam(ac.groups_of(params), lr=0.0, eps=ac.EPS)
        if offset:                                                                   # moments that start one float into their storage, too
            for p in params:
                opt.state[p] = {"step": torch.zeros((), dtype=torch.float32, device=DEV), "exp_avg": ac.leaf(np.zeros(p.shape, np.float32), DEV, True).detach(),
                                "exp_avg_sq": ac.leaf(np.zeros(p.shape, np.float32), DEV, True).detach()}
    if step0:
        ac.set_grads(params, ac.gradients(P, seed + 50, 1)[0], offset and cls is not torch.optim.Adam)
        opt.step()
        sd = opt.state_dict()
        for st in sd["state"].values():
            st["step"] = torch.tensor(float(step0), dtype=torch.float32, device=DEV)
        if offset and cls is not torch.optim.Adam:                                   # load_state_dict would hand out aligned copies of the moments
            for p in params:
                opt.state[p]["step"] = torch.tensor(float(step0), dtype=torch.float32, device=DEV)
        else:
            opt.load_state_dict(sd)
    return params, opt


def check_alignment(params, opt, offset):
    for p in params:
        for t in (p, p.grad, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]):
            assert (t.data_ptr() % 16 != 0) == offset, (offset, t.data_ptr() % 16)


# ---- 1. accuracy ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("step0", [0, 1000])
@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "one_float_in"])
@pytest.mark.parametrize("P", ROWS)
def test_accuracy_dense_and_masked_against_the_float64_twin(P, offset, step0):
    grads = ac.gradients(P, 11, 5)
    # the dense case: the operator, torch's fused float32 Adam and the twin on the same inputs; the bound comes from here
    mine_p, mine = fresh(P, 11, offset, step0=step0)
    ref_p, ref = fresh(P, 11, False, torch.optim.Adam, step0=step0)
    for a, b in zip(mine_p, ref_p):                                                  # both start from the same bits (step0: after the same first step within rounding)
        if step0 == 0:
            assert bits(a) == bits(b)
    start = lambda params, opt: ac.Twin(params, moments=ac.state_of(opt, params) if step0 else None, step0=step0)
    tw_mine, tw_ref = start(mine_p, mine), start(ref_p, ref)                         # each path against the twin of ITS start (equal for step0 = 0)
    limit = {}
    for k, g in enumerate(grads, 1):
        ac.set_grads(mine_p, g, offset); ac.set_grads(ref_p, g)
        mine.step(); ref.step()
        if k == 1:
            check_alignment(mine_p, mine, offset)
        tw_mine.step(g); tw_ref.step(g)
        if k in (1, 5):
            d_mine, d_ref = ac.distances(mine, mine_p, tw_mine), ac.distances(ref, ref_p, tw_ref)
            limit[k] = tuple(ac.bound(d) for d in d_ref)
            print(f"FUSEDADAM|P {P}|{'one float in' if offset else 'aligned'}|from step {step0}|{k} steps|dense|torch fused p/m/v {d_ref[0]:.3f} {d_ref[1]:.3f} {d_ref[2]:.3f}"
                  f"|operator {d_mine[0]:.3f} {d_mine[1]:.3f} {d_mine[2]:.3f}|ratio {' '.join(f'{a / b:.2f}' if b else 'n/a' for a, b in zip(d_mine, d_ref))}")
            assert all(a <= b for a, b in zip(d_mine, limit[k])), (P, offset, step0, k, d_mine, d_ref)
            assert all(float(mine.state[p]["step"]) == step0 + k for p in mine_p)
    # the masked cases against the twin under the same mask, with the dense case's bound
    for name, rows in masks_for(P).items():
        if rows is None:
            continue
        par, opt = fresh(P, 11, offset, step0=step0)
        tw = start(par, opt)
        for k, g in enumerate(grads, 1):
            ac.set_grads(par, g, offset)
            opt.step(rows=rows); tw.step(g, rows=rows)
            if k in (1, 5):
                d = ac.distances(opt, par, tw)
                assert all(a <= b for a, b in zip(d, limit[k])), (P, offset, step0, name, k, d, limit[k])
        if name != "zeros":
            on = rows.bool()
            assert not torch.equal(par[2].detach()[on], torch.as_tensor(ac.values(P, 11)[2], device=DEV)[on])     # the flagged rows did move


# ---- 2. bits ----------------------------------------------------------------------------------------------------------------------------------------

def run_steps(P, offset, rows_of_step, seed=12):
    par, opt = fresh(P, seed, offset)
    snaps = []
    for g, rows in zip(ac.gradients(P, seed, len(rows_of_step)), rows_of_step):
        ac.set_grads(par, g, offset)
        opt.step(rows=rows)
        snaps.append([(bits(p), bits(opt.state[p]["exp_avg"]), bits(opt.state[p]["exp_avg_sq"])) for p in par])
    return par, opt, snaps


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "one_float_in"])
@pytest.mark.parametrize("P", ROWS)
def test_bits(P, offset):
    M = masks_for(P)
    _, _, dense = run_steps(P, offset, [None, None])
    _, _, again = run_steps(P, offset, [None, None])
    assert dense == again                                                            # two calls on equal inputs give equal bits
    _, _, ones = run_steps(P, offset, [M["ones"], M["ones"].to(torch.uint8)])
    assert ones == dense                                                             # an all-ones mask equals the dense call bit for bit
    if not offset:
        _, _, other = run_steps(P, True, [None, None])
        assert other == dense                                                        # the 4-byte path gives the 16-byte path's bits
    for name, rows in M.items():
        if rows is None or name == "ones":
            continue
        par, opt, part = run_steps(P, offset, [None, rows])
        keep = (rows == 0).cpu().numpy()
        for i, p in enumerate(par):
            for k, t in enumerate((p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])):
                now = t.detach().cpu().numpy().reshape(P, -1)
                old = np.frombuffer(part[0][i][k], np.float32).reshape(P, -1)
                full = np.frombuffer(dense[1][i][k], np.float32).reshape(P, -1)
                assert now[keep].tobytes() == old[keep].tobytes(), (name, i, k)     # unflagged rows: byte-identical before and after
                assert now[~keep].tobytes() == full[~keep].tobytes(), (name, i, k)  # flagged rows: the dense call's bits
            assert float(opt.state[p]["step"]) == 2.0                                 # an all-zeros mask changes nothing except the step tensors
        if name == "zeros":
            assert part[1] == part[0]


# ---- 3. contract edges ------------------------------------------------------------------------------------------------------------------------------

def test_a_group_without_a_gradient_is_left_alone_while_the_others_step():
    P = 257
    par, opt = fresh(P, 13, False)
    g1, g2 = ac.gradients(P, 13, 2)
    ac.set_grads(par, g1); opt.step()
    before = [(bits(p), bits(opt.state[p]["exp_avg"]), bits(opt.state[p]["exp_avg_sq"])) for p in par]
    g2[2] = None; g2[5] = None
    ac.set_grads(par, g2); opt.step(rows=masks_for(P)["every_other"])
    for i, p in enumerate(par):
        now = (bits(p), bits(opt.state[p]["exp_avg"]), bits(opt.state[p]["exp_avg_sq"]))
        if i in (2, 5):
            assert now == before[i] and float(opt.state[p]["step"]) == 1.0
        else:
            assert now[0] != before[i][0] and now[1] != before[i][1] and float(opt.state[p]["step"]) == 2.0


def test_invalid_calls_raise_with_a_message_and_a_valid_call_follows():
    P = 300
    par, opt = fresh(P, 14, False)
    g = ac.gradients(P, 14, 1)[0]
    ac.set_grads(par, g)
    start = [bits(p) for p in par]
    with pytest.raises(optim.AdamError, match=r"lrt_adam_step failed \(-1\): lrt_adam_step: group 0 has 300 rows, the row mask 299"):
        opt.step(rows=torch.ones(P - 1, dtype=torch.bool, device=DEV))
    with pytest.raises(optim.AdamError, match="rows must be on cuda:0"):
        opt.step(rows=torch.ones(P, dtype=torch.bool))
    # a non-contiguous parameter
    q = torch.zeros(P, 6, device=DEV)[:, ::2].requires_grad_(True)
    o2 = optim.GaussianAdam([{"params": [q], "lr": 1e-3, "name": "strided"}], lr=0.0, eps=ac.EPS)
    q.grad = torch.ones(P, 3, device=DEV)
    with pytest.raises(optim.AdamError, match=r"lrt_adam_step: group strided: the parameter must be a contiguous float32 tensor.*not contiguous"):
        o2.step()
    # a float64 parameter on the device: no quiet fall-back to PyTorch there
    d = torch.zeros(P, 3, device=DEV, dtype=torch.float64, requires_grad=True)
    o3 = optim.GaussianAdam([{"params": [d], "lr": 1e-3, "name": "double"}], lr=0.0, eps=ac.EPS)
    d.grad = torch.ones_like(d)
    with pytest.raises(optim.AdamError, match=r"group double: the parameter must be a contiguous float32 tensor.*torch.float64"):
        o3.step()
    assert float(d.detach().abs().sum()) == 0.0
    # nine groups in one call
    nine = [torch.zeros(P, 2, device=DEV, requires_grad=True) for _ in range(9)]
    o4 = optim.GaussianAdam([{"params": [t], "lr": 1e-3, "name": f"g{i}"} for i, t in enumerate(nine)], lr=0.0, eps=ac.EPS)
    for t in nine:
        t.grad = torch.ones_like(t)
    with pytest.raises(optim.AdamError, match=r"lrt_adam_step: 9 groups \(1 .. 8 in one call\)"):
        o4.step()
    assert all(float(t.detach().abs().sum()) == 0.0 for t in nine) and all(float(o4.state[t]["step"]) == 0.0 for t in nine)
    # nothing moved, no count advanced; the valid call that follows works and is the first step
    assert [bits(p) for p in par] == start and all(float(opt.state[p]["step"]) == 0.0 for p in par if p in opt.state and len(opt.state[p]))
    opt.step(rows=torch.ones(P, dtype=torch.bool, device=DEV))
    tw = ac.Twin([torch.as_tensor(v) for v in ac.values(P, 14)]); tw.step(g)
    assert all(float(opt.state[p]["step"]) == 1.0 for p in par)
    assert all(ac.distance(opt.state[p]["exp_avg_sq"], v) <= 0.5 + 1e-6 for p, v in zip(par, tw.v))
    torch.cuda.synchronize()


# ---- 4. the loop -------------------------------------------------------------------------------------------------------------------------------------

def loop_setup():
    """Scene, rays, options and frame of tests/test_training.py::test_short_optimisation_run_on_the_gpu."""
    sc = scenes.make_scene(8000, seed=21, radius_scale=0.25)
    o, d = scenes.kitti_rays(16, 256)
    t = lambda a: torch.as_tensor(a, device=DEV)

    def asset(noise):
        r = np.random.default_rng(1)
        op = sc["opacities"]
        a = training.GaussianAsset.from_tensors(
            t(sc["means"] + noise * r.normal(size=sc["means"].shape).astype(np.float32)), t(sc["shs"][:, :1]), t(sc["shs"][:, 1:]),
            t(np.log(sc["scales"])), t(sc["rotations"]), t(np.log(op / (1 - op)) - 3.0 * float(noise > 0)), extent=15.0)
        a.active_sh_degree = 3
        return a
    opt = training.default_options()
    opt.position_lr_init, opt.position_lr_final = 0.002, 0.0002
    bg = torch.tensor([0.0, 0.0, 1.0], device=DEV)
    frames = training.RangeFrames()
    from lidar_rt_amd.renderer import raytracing
    args = types.SimpleNamespace(dynamic=False, opt=opt, pipe=types.SimpleNamespace())
    with torch.no_grad():
        pk = raytracing(0, [asset(0.0)], (t(o), t(d), torch.zeros(3, device=DEV)), bg, args)
    mask = pk["raydrop"].squeeze(-1) < 0.6
    frames.add_frame(0, t(o), t(d), pk["depth"].squeeze(-1).detach(), pk["intensity"].squeeze(-1).detach(), mask)
    return asset, opt, bg, frames


@pytest.fixture(scope="module")
def loop():
    return loop_setup()


def test_the_short_optimisation_run_under_the_three_settings(loop):
    asset, opt0, bg, frames = loop
    for name, kw in (("default", {}), ("fused_adam", dict(fused_adam=True)), ("fused_adam + sparse_adam", dict(fused_adam=True, sparse_adam=True))):
        opt = types.SimpleNamespace(**vars(opt0))
        for k, v in kw.items():
            setattr(opt, k, v)
        scene = training.GaussianScene([asset(0.05)])
        scene.training_setup(opt)
        g = scene.gaussians_assets[0]
        assert type(g.optimizer) is (optim.GaussianAdam if kw else torch.optim.Adam)
        hist = [training.training_step(scene, frames, 0, it, opt, bg) for it in range(1, 61)]
        first, last = float(torch.stack([h["loss"] for h in hist[:5]]).mean()), float(torch.stack([h["loss"] for h in hist[-5:]]).mean())
        touched = float((g.denom > 0).float().mean())
        print(f"FUSEDADAM|loop|{name}|first five {first:.6f}|last five {last:.6f}|ratio {last / first:.4f}|rows hit at least once in 60 iterations {touched:.3f}")
        assert np.isfinite(last) and last < 0.7 * first, (name, first, last)
        assert float(g.denom.sum()) > 0 and float(g.xyz_gradient_accum.sum()) > 0
        if "sparse_adam" in kw:
            # rows no ray ever hit kept their parameters and have no moments; the others moved
            never = (g.denom == 0).reshape(-1)
            x0 = asset(0.05)._xyz.detach()
            assert int(never.sum()) > 0 and torch.equal(g._xyz.detach()[never], x0[never]) and not torch.equal(g._xyz.detach()[~never], x0[~never])
            assert float(g.optimizer.state[g._xyz]["exp_avg_sq"][never].abs().sum()) == 0.0
            # densify + prune on the live optimiser: every group was just replaced and has no gradient (the mask still has the old length) --
            # the iteration must pass, and the following one must step
            opt.densify_from_iter, opt.densification_interval = 0, 1
            info = training.training_step(scene, frames, 0, 61, opt, bg)
            assert info["points"] == g._xyz.shape[0] and sum(info["densify"]) >= 0
            steps = [float(g.optimizer.state[p]["step"]) for p in g._params().values()]
            opt.densify_until_iter = 0                                               # no densification in the next iteration: it steps
            x1 = g._xyz.detach().clone()
            training.training_step(scene, frames, 0, 62, opt, bg)
            assert [float(g.optimizer.state[p]["step"]) for p in g._params().values()] == [s + 1 for s in steps]
            assert not torch.equal(g._xyz.detach(), x1)


# ---- 5. resume ----------------------------------------------------------------------------------------------------------------------------------------

def test_a_resumed_deterministic_run_repeats_the_uninterrupted_one_bit_for_bit(loop):
    from lidar_rt_amd import renderer
    asset, opt0, bg, frames = loop
    opt = types.SimpleNamespace(**vars(opt0)); opt.fused_adam = True; opt.sparse_adam = True
    saved = (renderer.deterministic, renderer.deferred_accum)
    renderer.deterministic, renderer.deferred_accum = True, True                     # what `train --deterministic` sets

    def state(scene):
        g = scene.gaussians_assets[0]
        out = {n: bits(p) for n, p in g._params().items()}
        for n, p in g._params().items():
            st = g.optimizer.state[p]
            out[n + ".m"], out[n + ".v"], out[n + ".step"] = bits(st["exp_avg"]), bits(st["exp_avg_sq"]), float(st["step"])
        out["accum"], out["denom"] = bits(g.xyz_gradient_accum), bits(g.denom)
        return out
    try:
        a = training.GaussianScene([asset(0.05)]); a.training_setup(opt)
        for it in range(1, 7):
            training.training_step(a, frames, 0, it, opt, bg)
        b = training.GaussianScene([asset(0.05)]); b.training_setup(opt)
        for it in range(1, 4):
            training.training_step(b, frames, 0, it, opt, bg)
        buf = io.BytesIO(); b.save(3, buf); buf.seek(0)
        params, it0 = torch.load(buf, map_location=DEV, weights_only=False)
        c = training.GaussianScene([training.GaussianAsset(extent=15.0)]); c.restore(params, opt)
        c.gaussians_assets[0].active_sh_degree = 3
        assert type(c.gaussians_assets[0].optimizer) is optim.GaussianAdam and it0 == 3
        for it in range(4, 7):
            training.training_step(c, frames, 0, it, opt, bg)
        sa, sc_ = state(a), state(c)
        assert sa.keys() == sc_.keys() and all(sa[k] == sc_[k] for k in sa), [k for k in sa if sa[k] != sc_[k]]
        assert sa["xyz.step"] == 6.0 and sa != state(b)
    finally:
        renderer.deterministic, renderer.deferred_accum = saved


# ---- 6. no wait -----------------------------------------------------------------------------------------------------------------------------------------

def test_a_step_on_warm_state_does_not_wait_for_the_device():
    P = 1000
    par, opt = fresh(P, 15, False)
    g = ac.gradients(P, 15, 3)
    rows = masks_for(P)["every_other"]
    ac.set_grads(par, g[0]); opt.step(rows=rows)                                     # warm: state, host mirror, the loaded library
    grads = [[torch.as_tensor(x, device=DEV) for x in gk] for gk in g[1:]]
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for gk in grads:
            for p, x in zip(par, gk):
                p.grad = x
            opt.step(rows=rows)
        for p, x in zip(par, grads[0]):
            p.grad = x
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert all(float(opt.state[p]["step"]) == 4.0 for p in par)
