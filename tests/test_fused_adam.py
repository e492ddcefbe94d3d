"""The fused Adam step without a GPU: the sixth product library (`liblrt_adam.so`: a source list and hash of its own that moves no other hash,
exports, resource gate, argument errors before the device is touched), the arithmetic header compiled for the host, the float64 twin
`optim.adam_reference` against `torch.optim.Adam` in float64, `optim.GaussianAdam` on CPU tensors (dense against torch's float32 Adam, the
row mask's semantics, the contract edges) and the two switches of the training loop."""
import ctypes as C
import io
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from lidar_rt_amd import build as lrt_build, optim, resources, training
from tests import adam_cases as ac

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


# ---- build ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def adam_lib():
    return lrt_build.build_adam()


def test_the_library_has_a_source_list_of_its_own_and_moves_no_other_hash():
    assert lrt_build.ADAM_SOURCES == ["lrt_adam.hip"] and "lrt_adam_math.h" in lrt_build.ADAM_HEADERS
    others = (lrt_build.SOURCES + lrt_build.HEADERS + lrt_build.LOSS_SOURCES + lrt_build.LOSS_HEADERS + lrt_build.GRIDCD_SOURCES + lrt_build.GRIDCD_HEADERS
              + lrt_build.INIT_SOURCES + lrt_build.INIT_HEADERS + lrt_build.METRICS_SOURCES + lrt_build.METRICS_HEADERS)
    assert not any("lrt_adam" in f for f in others)
    # the other libraries' hashes at the commit this library was added on: committed profiles are keyed by them
    assert lrt_build.source_hash() == "2c98b54882a7ff74"          # moved twice since: the non-finite-input fixes in lrt_chamfer.hip; a comment of include/lrt.h (lrt_xchg_apply, zero_only on an overflowed block)
    assert lrt_build.loss_source_hash() == "cc56b0c83f72d5ca"
    assert lrt_build.gridcd_source_hash() == "fd279d9f7ff67722"
    assert lrt_build.init_source_hash() == "0fd7105f5d08ab22"
    assert lrt_build.metrics_source_hash() == "9e8267ef6335030b"
    assert "lrt_adam" not in open(lrt_build.EXT_SRC).read()
    assert lrt_build.adam_source_hash() not in (lrt_build.source_hash(), lrt_build.loss_source_hash(), lrt_build.gridcd_source_hash(), lrt_build.init_source_hash(),
                                                lrt_build.metrics_source_hash())
    assert os.path.basename(lrt_build.ADAM_LIB) == "liblrt_adam.so"
    assert lrt_build.ADAM_LIB not in (lrt_build.LIB, lrt_build.LOSS_LIB, lrt_build.GRIDCD_LIB, lrt_build.INIT_LIB, lrt_build.METRICS_LIB)
    assert "build_adam(force, verbose)" in open(lrt_build.__file__).read()              # _build_product builds it
    assert "csrc/liblrt_adam.so" in open(os.path.join(REPO, "setup.py")).read()


def test_the_library_builds_and_exports_what_its_header_declares(adam_lib):
    assert os.path.exists(adam_lib) and not lrt_build.adam_is_stale()
    assert open(lrt_build.ADAM_STAMP).read().strip() == lrt_build.adam_source_hash()
    hdr = open(os.path.join(REPO, "include", "lrt_adam.h")).read()
    declared = set(re.findall(r"\b(lrt_adam_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(optim.EXPORTS), declared ^ set(optim.EXPORTS)
    lib = optim.load()
    for n in declared:
        assert hasattr(lib, n), n
    exported = set(re.findall(r"\blrt_adam_[a-z_]+\b", subprocess.run(["nm", "-D", "--defined-only", adam_lib], capture_output=True, text=True, check=True).stdout))
    assert exported == declared, exported ^ declared
    assert lib.lrt_adam_abi_version() == int(re.search(r"#define\s+LRT_ADAM_ABI_VERSION\s+(\d+)", hdr).group(1)) == optim.ABI_VERSION
    assert int(re.search(r"#define\s+LRT_ADAM_MAX_GROUPS\s+(\d+)", hdr).group(1)) == optim.MAX_GROUPS == 8


def test_the_kernel_passes_the_resource_gate(adam_lib):
    res = resources.kernel_resources(adam_lib)
    own = sorted(n for n in res if resources.is_own_kernel(n))
    assert own == ["k_adam_step"], own                                                  # ONE kernel: the dense step is the masked one without a mask
    assert all(any(re.search(g_, n) for g_ in resources.GATED) for n in own)
    assert resources.violations(res) == []
    r = res["k_adam_step"]
    assert r["vgpr_spill"] == 0 and r["scratch_bytes"] == 0 and not r["dynamic_stack"], r
    resources.check(adam_lib)


def test_argument_errors_come_before_the_device_and_launch_nothing(adam_lib):
    lib = optim.load()
    buf = (C.c_char * 4096)()
    p = (C.addressof(buf) + 15) // 16 * 16
    err = lambda: lib.lrt_adam_last_error()
    grp = lambda **kw: optim._Group(**{**dict(param=p, grad=p, exp_avg=p, exp_avg_sq=p, rows=10, width=3, lr=1e-3, bias_correction1=0.1, bias_correction2_sqrt=0.03), **kw})
    nodev = 1 << 20                                                                     # a device that does not exist: what passes the checks ends there

    def call(groups, mask=None, mask_rows=0, b1=0.9, b2=0.999, eps=1e-15, n=None):
        arr = (optim._Group * max(1, len(groups)))(*groups)
        return lib.lrt_adam_step(nodev, len(groups) if n is None else n, C.cast(arr, C.c_void_p), mask, mask_rows, b1, b2, eps, None)
    assert call([], n=0) < 0 and b"0 groups (1 .. 8 in one call)" in err()
    assert call([grp()] * 9) < 0 and b"9 groups (1 .. 8 in one call)" in err()
    assert lib.lrt_adam_step(nodev, 1, None, None, 0, 0.9, 0.999, 1e-15, None) < 0 and b"null group table" in err()
    for f in ("param", "grad", "exp_avg", "exp_avg_sq"):
        assert call([grp(), grp(**{f: None})]) < 0 and b"group 1: null parameter / gradient / moment pointer" in err()
    assert call([grp(width=0)]) < 0 and b"width 0" in err()
    assert call([grp(rows=-1)]) < 0 and b"-1 rows" in err()
    assert call([grp(), grp(rows=11)], mask=p, mask_rows=10) < 0 and b"group 1 has 11 rows, the row mask 10" in err()
    assert call([grp()], mask=p, mask_rows=-1) < 0 and b"a mask of -1 rows" in err()
    assert call([grp()], b1=1.0) < 0 and b"beta1 = 1" in err()
    assert call([grp()], eps=float("nan")) < 0 and b"eps" in err()
    assert call([grp(bias_correction1=0.0)]) < 0 and b"bias_correction1 = 0" in err()
    assert call([grp(lr=float("nan"))]) < 0 and b"lr = nan" in err()
    # every argument in order (groups of different lengths are fine without a mask): only now the device is looked for
    assert call([grp(), grp(rows=11)]) < 0 and b"no HIP device" in err()
    assert call([grp()] * 8, mask=p, mask_rows=10) < 0 and b"no HIP device" in err()


# ---- the arithmetic header on the host -------------------------------------------------------------------------------------------------------------

def test_the_arithmetic_header_against_the_same_text_in_double(tmp_path):
    exe = str(tmp_path / "adam_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "host_check", "adam_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "ADAMCHECK ok" in r.stdout, r.stdout + r.stderr
    rows = [l for l in r.stdout.splitlines() if l.startswith("ADAMCHECK|")]
    assert len(rows) == 8 and sum("step 1000|" in l for l in rows) == 4 and sum("|lr 0|" in l for l in rows) == 2     # steps 1 and 1000, lr = 0 among the rates
    assert sum(int(re.search(r"\|(\d+) elements", l).group(1)) for l in rows) >= 4000


# ---- the twin -------------------------------------------------------------------------------------------------------------------------------------------

def test_the_twin_against_torch_adam_in_float64():
    """Five consecutive steps with fresh gradients of both signs.  Bound: a few float64 ulps -- of the value for exp_avg_sq, whose terms are all
    positive; for exp_avg and the parameter, whose terms cancel, of the sum of the terms' magnitudes (A_m = the exp_avg recursion on |g|;
    A_p = |p0| + the sum over the steps of step_size * A_m / denom).  Both sides round every operation once (2^-53 relative to a result no
    larger than A): the moment lines have at most 4 operations on each side, so a step adds at most 8 * 2^-53 A = 4 * 2^-52 A and the
    earlier steps' differences are carried over with a factor below 1; the parameter line adds its own 6 operations on top of what it
    inherits from both moments.  8 k 2^-52 A after k steps for all three."""
    P = 300
    params = [torch.as_tensor(v).double().requires_grad_(True) for v in ac.values(P, 1)]
    ref = torch.optim.Adam(ac.groups_of(params), lr=0.0, eps=ac.EPS)
    tw = ac.Twin(params)
    b1, b2 = ac.BETAS
    A_m = [torch.zeros_like(p) for p in tw.p]
    A_p = [p.abs().clone() for p in tw.p]
    e = 2.0 ** -52
    for k, grads in enumerate(ac.gradients(P, 1, 5), 1):
        ac.set_grads(params, [g.astype(np.float64) for g in grads])
        ref.step()
        tw.step([g.astype(np.float64) for g in grads])
        bc1, bc2s = optim.bias_corrections(float(k), b1, b2)
        for i, p in enumerate(params):
            st = ref.state[p]
            A_m[i] = b1 * A_m[i] + (1 - b1) * torch.as_tensor(grads[i]).double().abs()
            A_p[i] = A_p[i] + (ac.LRS[i] / bc1) * A_m[i] / (tw.v[i].sqrt() / bc2s + ac.EPS)
            assert float(st["step"]) == k
            assert torch.all((st["exp_avg_sq"] - tw.v[i]).abs() <= 8 * k * e * tw.v[i]), (k, i)
            assert torch.all((st["exp_avg"] - tw.m[i]).abs() <= 8 * k * e * A_m[i]), (k, i)
            assert torch.all((p.detach() - tw.p[i]).abs() <= 8 * k * e * A_p[i]), (k, i)
    assert all(float((p.detach() - torch.as_tensor(v0).double()).abs().max()) > 0 for p, v0 in zip(params, ac.values(P, 1)))
    # the mask of the twin: a row whose flag is 0 keeps all three
    rows = torch.arange(P) % 3 == 0
    g = torch.as_tensor(ac.gradients(P, 2, 1)[0][2])
    full = optim.adam_reference(tw.p[2], g, tw.m[2], tw.v[2], step=6.0, lr=1e-3)
    part = optim.adam_reference(tw.p[2], g, tw.m[2], tw.v[2], step=6.0, lr=1e-3, rows=rows)
    for a, b, old in zip(full, part, (tw.p[2], tw.m[2], tw.v[2])):
        assert a.dtype == torch.float64 and torch.equal(b[rows], a[rows]) and torch.equal(b[~rows], old[~rows])
    with pytest.raises(optim.AdamError, match="row mask of 5 rows"):
        optim.adam_reference(tw.p[2], g, tw.m[2], tw.v[2], step=6.0, lr=1e-3, rows=torch.ones(5, dtype=torch.bool))


# ---- GaussianAdam on CPU tensors ---------------------------------------------------------------------------------------------------------------------

def make(P, seed, cls, dtype=torch.float32):
    params = [torch.as_tensor(v).to(dtype).requires_grad_(True) for v in ac.values(P, seed)]
    if cls is torch.optim.Adam:
        return params, torch.optim.Adam(ac.groups_of(params), lr=0.0, eps=ac.EPS)
    return params, optim.GaussianAdam(ac.groups_of(params), lr=0.0, eps=ac.EPS)


@pytest.mark.parametrize("P", [1, 257])
def test_dense_steps_on_cpu_against_torch_float32_under_the_gate(P):
    mine_p, mine = make(P, 3, optim.GaussianAdam)
    ref_p, ref = make(P, 3, torch.optim.Adam)
    tw = ac.Twin(mine_p)
    for k, grads in enumerate(ac.gradients(P, 3, 5), 1):
        ac.set_grads(mine_p, grads); ac.set_grads(ref_p, grads)
        mine.step(); ref.step(); tw.step(grads)
        if k in (1, 5):
            d_mine, d_ref = ac.distances(mine, mine_p, tw), ac.distances(ref, ref_p, tw)
            print(f"FUSEDADAM|cpu|P {P}|{k} steps|torch float32 p/m/v {d_ref[0]:.3f} {d_ref[1]:.3f} {d_ref[2]:.3f}|GaussianAdam {d_mine[0]:.3f} {d_mine[1]:.3f} {d_mine[2]:.3f}")
            for a, b in zip(d_mine, d_ref):
                assert a <= ac.bound(b), (P, k, d_mine, d_ref)
    st = mine.state[mine_p[0]]
    assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and st["step"].dtype == torch.float32 and st["step"].shape == () and float(st["step"]) == 5.0
    assert st["step"].device == mine_p[0].device and st["exp_avg"].dtype == torch.float32


def test_a_parameter_without_a_gradient_is_skipped_and_its_step_does_not_move():
    P = 40
    params, opt = make(P, 4, optim.GaussianAdam)
    g1, g2 = ac.gradients(P, 4, 2)
    ac.set_grads(params, g1); opt.step()
    before = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in params]
    g2[1] = None; g2[4] = None
    ac.set_grads(params, g2); opt.step()
    for i, p in enumerate(params):
        st = opt.state[p]
        if i in (1, 4):
            assert float(st["step"]) == 1.0 and torch.equal(p.detach(), before[i][0]) and torch.equal(st["exp_avg"], before[i][1]) and torch.equal(st["exp_avg_sq"], before[i][2])
        else:
            assert float(st["step"]) == 2.0 and not torch.equal(st["exp_avg"], before[i][1])
    # a parameter that never had a gradient has no state at all, as in torch
    q = torch.zeros(3, 2, requires_grad=True)
    o2 = optim.GaussianAdam([{"params": [q], "lr": 1e-3, "name": "q"}], lr=0.0, eps=ac.EPS)
    o2.step()
    assert len(o2.state) == 0
    # the skipped groups resume with THEIR step count: bias corrections of step 2, not 3
    g3 = ac.gradients(P, 5, 1)[0]
    tw = ac.Twin([params[1]], moments=[(opt.state[params[1]]["exp_avg"], opt.state[params[1]]["exp_avg_sq"])], step0=1)
    ac.set_grads(params, g3); opt.step()
    tw.step([g3[1]], lrs=[ac.LRS[1]])
    assert float(opt.state[params[1]]["step"]) == 2.0 and float(opt.state[params[0]]["step"]) == 3.0
    # one step from a common state: exp_avg is the float64 value rounded once; the parameter as the host check bounds it (11 half-ulps of A_p)
    assert ac.distance(opt.state[params[1]]["exp_avg"], tw.m[0]) <= 0.5 + 1e-6 and ac.distance(params[1], tw.p[0], tw.A_p[0]) <= 5.5


def test_per_group_learning_rates_and_a_changed_xyz_rate_between_steps():
    P = 64
    params, opt = make(P, 6, optim.GaussianAdam)
    ref_p, ref = make(P, 6, torch.optim.Adam)
    tw = ac.Twin(params)
    lrs = list(ac.LRS)
    for k, grads in enumerate(ac.gradients(P, 6, 3)):
        lrs[0] = ac.LRS[0] * (0.5 ** k)                                     # what update_learning_rate does
        for o in (opt, ref):
            for g in o.param_groups:
                if g["name"] == "xyz":
                    g["lr"] = lrs[0]
        before = [p.detach().clone() for p in params]
        ac.set_grads(params, grads); ac.set_grads(ref_p, grads)
        opt.step(); ref.step(); tw.step(grads, lrs=lrs)
        d_mine, d_ref = ac.distances(opt, params, tw), ac.distances(ref, ref_p, tw)
        assert all(a <= ac.bound(b) for a, b in zip(d_mine, d_ref)), (k, d_mine, d_ref)       # the twin took the changed rates: so did the optimizer
        if k == 0:
            # the first step of Adam moves every element with a gradient by lr (m / sqrt(v) = +-1 up to rounding): each group's own rate shows
            for i, p in enumerate(params):
                moved = (p.detach() - before[i]).abs()[torch.as_tensor(grads[i]) != 0]
                assert torch.allclose(moved, torch.full_like(moved, lrs[i]), rtol=1e-3, atol=2e-7), i
    x_last = (params[0].detach() - before[0]).abs().max()
    assert float(x_last) < 0.5 * ac.LRS[0]                                   # the third step of xyz ran at a quarter of the first rate
    # lr = 0 leaves the parameter's bits and moves the moments
    for g in opt.param_groups:
        g["lr"] = 0.0
    before = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in params]
    ac.set_grads(params, ac.gradients(P, 7, 1)[0]); opt.step()
    for p, (p0, m0, v0) in zip(params, before):
        assert p.detach().numpy().tobytes() == p0.numpy().tobytes()
        assert not torch.equal(opt.state[p]["exp_avg"], m0) and not torch.equal(opt.state[p]["exp_avg_sq"], v0)


def test_sparse_semantics_on_cpu():
    P = 300
    bits = lambda t: t.detach().numpy().tobytes()
    grads = ac.gradients(P, 8, 3)

    def run(rows_of_step):
        params, opt = make(P, 8, optim.GaussianAdam)
        snaps = []
        for grads_k, rows in zip(grads, rows_of_step):
            ac.set_grads(params, grads_k)
            opt.step(rows=rows)
            snaps.append([(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in params])
        return params, opt, snaps
    _, _, dense = run([None, None, None])
    ones = torch.ones(P, dtype=torch.bool)
    _, _, allon = run([ones, ones.to(torch.uint8), ones])
    for a, b in zip(dense, allon):                                                  # an all-ones mask equals rows=None bit for bit
        for ta, tb in zip(a, b):
            assert all(bits(x) == bits(y) for x, y in zip(ta, tb))
    rows = torch.zeros(P, dtype=torch.bool); rows[::2] = True; rows[255] = True; rows[P - 1] = True
    params, opt, part = run([None, rows, None])
    for i in range(6):
        for k in range(3):                                                          # parameter, exp_avg, exp_avg_sq
            kept, old = part[1][i][k], part[0][i][k]
            assert bits(kept[~rows]) == bits(old[~rows]), (i, k)                     # unmasked rows: bit for bit
            assert bits(kept[rows]) == bits(dense[1][i][k][rows]), (i, k)            # masked rows: the dense result bit for bit
            assert not torch.equal(kept[rows], old[rows])
        assert float(opt.state[params[i]]["step"]) == 3.0                            # the step count advances whatever the mask
    # the third, dense step of the partly stepped run continues from the kept moments of the unseen rows
    assert not torch.equal(part[2][2][1][~rows], dense[2][2][1][~rows]) and torch.equal(part[2][2][1][rows], dense[2][2][1][rows])
    none = torch.zeros(P, dtype=torch.bool)
    params, opt, z = run([None, none, None])
    assert all(bits(x) == bits(y) for a, b in zip(z[0], z[1]) for x, y in zip(a, b)) and float(opt.state[params[0]]["step"]) == 3.0
    # a mask of the wrong length raises and nothing moves
    params, opt, s = run([None])
    ac.set_grads(params, grads[1])
    with pytest.raises(optim.AdamError, match=r"has 300 rows, the row mask 299"):
        opt.step(rows=torch.ones(P - 1, dtype=torch.bool))
    assert all(bits(p) == bits(s[0][i][0]) and float(opt.state[p]["step"]) == 1.0 for i, p in enumerate(params))
    with pytest.raises(optim.AdamError, match="bool or uint8"):
        opt.step(rows=torch.ones(P))
    opt.step(rows=torch.ones(P, dtype=torch.bool))                                   # and the optimizer still steps


def test_a_float64_cpu_tensor_runs_the_rule_in_float64():
    P = 50
    params, opt = make(P, 9, optim.GaussianAdam, dtype=torch.float64)
    tw = ac.Twin(params)
    for grads in ac.gradients(P, 9, 3):
        ac.set_grads(params, [g.astype(np.float64) for g in grads]); opt.step(); tw.step(grads)
    for i, p in enumerate(params):
        assert p.dtype == torch.float64 and ac.distance(p, tw.p[i]) <= 1e-6 and ac.distance(opt.state[p]["exp_avg_sq"], tw.v[i]) <= 1e-6


# ---- the training loop ---------------------------------------------------------------------------------------------------------------------------------

def make_asset(P=200, seed=0, **kw):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return training.GaussianAsset.from_tensors(r(P, 3) * 5, r(P, 1, 3), r(P, 15, 3) * 0.1, r(P, 2) * 0.3 - 2.0, r(P, 4), r(P, 1), extent=10.0, **kw)


def options(**kw):
    opt = training.default_options()
    for k, v in kw.items():
        setattr(opt, k, v)
    return opt


def fake_grads(a, seed):
    g = torch.Generator().manual_seed(seed)
    for p in a._params().values():
        p.grad = torch.randn(p.shape, generator=g) * 0.01


def test_the_switches_are_off_by_default_and_build_the_old_optimizer():
    opt = training.default_options()
    assert opt.fused_adam is False and opt.sparse_adam is False
    a = make_asset(); a.training_setup(opt)
    assert type(a.optimizer) is torch.optim.Adam
    bare = types.SimpleNamespace(**{k: v for k, v in vars(opt).items() if k not in ("fused_adam", "sparse_adam")})      # options from before the switches
    b = make_asset(); b.training_setup(bare)
    assert type(b.optimizer) is torch.optim.Adam
    for kw in (dict(fused_adam=True), dict(sparse_adam=True), dict(fused_adam=True, sparse_adam=True)):                  # sparse implies fused
        c = make_asset(); c.training_setup(options(**kw))
        assert type(c.optimizer) is optim.GaussianAdam
    import sys
    r = subprocess.run([sys.executable, "-m", "lidar_rt_amd.train", "--help"], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "--fused-adam" in r.stdout and "--sparse-adam" in r.stdout


def test_training_setup_builds_the_six_groups_with_their_names_and_rates():
    opt = options(fused_adam=True)
    a = make_asset(); a.training_setup(opt)
    assert isinstance(a.optimizer, optim.GaussianAdam) and isinstance(a.optimizer, torch.optim.Optimizer)
    names = [g["name"] for g in a.optimizer.param_groups]
    assert names == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"]
    lrs = {g["name"]: g["lr"] for g in a.optimizer.param_groups}
    assert lrs["f_rest"] == pytest.approx(opt.feature_lr / 20) and lrs["xyz"] == pytest.approx(opt.position_lr_init * 10.0)
    assert lrs["f_dc"] == opt.feature_lr and lrs["opacity"] == opt.opacity_lr and lrs["scaling"] == opt.scaling_lr and lrs["rotation"] == opt.rotation_lr
    assert a.optimizer.defaults["eps"] == 1e-15 and a.optimizer.defaults["lr"] == 0.0 and all(g["eps"] == 1e-15 for g in a.optimizer.param_groups)
    assert [g["params"][0] for g in a.optimizer.param_groups] == [a._params()[n] for n in names] or all(
        g["params"][0] is a._params()[n] for g, n in zip(a.optimizer.param_groups, names))
    assert a.update_learning_rate(0) == pytest.approx(opt.position_lr_init * 10.0)
    assert a.update_learning_rate(opt.position_lr_max_steps) == pytest.approx(opt.position_lr_final * 10.0)
    mid = a.update_learning_rate(opt.position_lr_max_steps // 2)
    assert mid == pytest.approx(10.0 * np.sqrt(opt.position_lr_init * opt.position_lr_final), rel=1e-6)
    assert lrs != {g["name"]: g["lr"] for g in a.optimizer.param_groups}            # the schedule reached the optimizer's xyz group


def test_prune_append_and_reset_keep_the_state_consistent():
    opt = options(fused_adam=True)
    a = make_asset(300); a.training_setup(opt)
    fake_grads(a, 1); a.optimizer.step()
    m0 = a.optimizer.state[a._xyz]["exp_avg"].clone()
    mask = torch.zeros(300, dtype=torch.bool); mask[::3] = True
    a.prune_points(mask)
    assert a._xyz.shape[0] == 200 and a.denom.shape == (200, 1) and a.max_radii2D.shape == (200,)
    for name, p in a._params().items():
        st = a.optimizer.state[p]
        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape, name
    assert torch.equal(a.optimizer.state[a._xyz]["exp_avg"], m0[~mask])
    a._append(a._select(torch.arange(200) < 10))
    assert a._xyz.shape[0] == 210 and torch.all(a.optimizer.state[a._xyz]["exp_avg"][200:] == 0)
    a.reset_opacity()
    assert float(a.get_opacity.detach().max()) <= 0.01 + 1e-6 and torch.all(a.optimizer.state[a._opacity]["exp_avg"] == 0)
    # an iteration in which every group was just replaced: nothing has a gradient, nothing steps -- also with a mask of the OLD length
    a.optimizer.step(rows=torch.ones(300, dtype=torch.bool))
    assert all(float(a.optimizer.state[p]["step"]) == 1.0 for p in a._params().values())
    fake_grads(a, 2); a.optimizer.step(rows=torch.ones(210, dtype=torch.bool))      # the rebuilt optimiser still steps, from the moved state's count
    assert all(float(a.optimizer.state[p]["step"]) == 2.0 for p in a._params().values())
    assert len(a.optimizer.state) == 6


@pytest.mark.parametrize("first,second", [("adam", "fused"), ("fused", "adam")])
def test_a_checkpoint_moves_between_the_two_optimizers(first, second):
    o = {"adam": options(), "fused": options(fused_adam=True)}
    kind = {"adam": torch.optim.Adam, "fused": optim.GaussianAdam}
    a = make_asset(60, 1); a.training_setup(o[first])
    for k in range(3):
        fake_grads(a, 10 + k); a.optimizer.step()
    buf = io.BytesIO()
    training.GaussianScene([a]).save(77, buf); buf.seek(0)
    cp, it = torch.load(buf, weights_only=False)
    assert it == 77
    b = training.GaussianAsset(extent=10.0); b.restore(cp[0], o[second])            # under the other optimizer
    buf.seek(0)
    c = training.GaussianAsset(extent=10.0); c.restore(torch.load(buf, weights_only=False)[0][0], o[first])      # and under its own
    assert type(b.optimizer) is kind[second] and type(c.optimizer) is kind[first]
    for n, p in b._params().items():
        sb, sa = b.optimizer.state[p], a.optimizer.state[a._params()[n]]
        assert torch.equal(sb["exp_avg"], sa["exp_avg"]) and torch.equal(sb["exp_avg_sq"], sa["exp_avg_sq"]) and float(sb["step"]) == 3.0
        assert torch.is_tensor(sb["step"]) and sb["step"].dtype == torch.float32
    assert [g["name"] for g in b.optimizer.param_groups] == list(training.GaussianAsset.GROUPS)
    # the next step from equal gradients: each against the float64 twin of the restored state, ONE step from a common float32 state.  Bounds from
    # the formats (tests/host_check/adam_check.cpp derives the operator's): the parameter within 2^-24 (|p| + 9 |update|) -- torch's float32 line
    # has no more roundings than the operator's; the operator's moments are the float64 values rounded once (half an ulp), torch's float32 lines
    # take 3 roundings and a float32 (1 - beta) that is up to 0.8 ulp off: below 3 ulps (of A_m where exp_avg's terms cancel)
    names = list(b._params())
    tw = ac.Twin([b._params()[n] for n in names], moments=[(b.optimizer.state[b._params()[n]]["exp_avg"], b.optimizer.state[b._params()[n]]["exp_avg_sq"]) for n in names], step0=3)
    lrs = [next(g["lr"] for g in b.optimizer.param_groups if g["name"] == n) for n in names]
    fake_grads(b, 20); fake_grads(c, 20)
    p_before = [p.clone() for p in tw.p]
    tw.step([b._params()[n].grad for n in names], lrs=lrs)
    b.optimizer.step(); c.optimizer.step()
    for asset in (b, c):
        lim = 0.5 + 1e-6 if type(asset.optimizer) is optim.GaussianAdam else 3.0
        for i, n in enumerate(names):
            p, st = asset._params()[n], asset.optimizer.state[asset._params()[n]]
            tol = 2.0 ** -24 * (tw.p[i].abs() + 9 * (tw.p[i] - p_before[i]).abs()) * (1 + 1e-6)
            assert torch.all((p.detach().double() - tw.p[i]).abs() <= tol), (type(asset.optimizer).__name__, n)
            assert ac.distance(st["exp_avg"], tw.m[i], tw.A_m[i]) <= lim and ac.distance(st["exp_avg_sq"], tw.v[i]) <= lim, (type(asset.optimizer).__name__, n)
    assert all(float(b.optimizer.state[p]["step"]) == 4.0 for p in b._params().values())
    for n in names:                                                                  # and the two agree: a few float32 ulps of the parameter
        assert torch.allclose(b._params()[n].detach(), c._params()[n].detach(), rtol=4 * 2.0 ** -23, atol=1e-9), n


def test_sparse_adam_steps_hit_rows_only_and_a_boxed_asset_with_a_regulariser_densely():
    box = types.SimpleNamespace(frame={}, min_xyz=torch.tensor([-1.0, -1, -1]), max_xyz=torch.tensor([1.0, 1, 1]))
    nb, na = 40, 30

    def run(**kw):
        opt = options(sparse_adam=True, **kw)
        sc = training.GaussianScene([make_asset(nb, 1), make_asset(na, 2, bounding_box=box)])
        sc.training_setup(opt)
        before = [[p.detach().clone() for p in g._params().values()] for g in sc.gaussians_assets]
        for g in sc.gaussians_assets:
            fake_grads(g, 5)
        w = torch.zeros(nb + na, 1); w[::2] = 0.5                                    # every other Gaussian was hit
        sc.optimize(opt, 1, torch.randn(nb + na, 3), w)
        moved = [[(p.detach() != b).reshape(p.shape[0], -1).any(1) for p, b in zip(g._params().values(), bs)] for g, bs in zip(sc.gaussians_assets, before)]
        return sc, moved
    hit_b, hit_a = torch.arange(nb) % 2 == 0, (torch.arange(nb, nb + na) % 2 == 0)
    sc, moved = run()                                                                # lambda_reg = 0.01, the default
    assert type(sc.gaussians_assets[0].optimizer) is optim.GaussianAdam
    assert all(torch.equal(m, hit_b) for m in moved[0])                              # the background: hit rows only
    assert all(bool(m.all()) for m in moved[1])                                      # the boxed actor: every row
    st = sc.gaussians_assets[0].optimizer.state[sc.gaussians_assets[0]._xyz]
    assert torch.all(st["exp_avg"][~hit_b] == 0) and torch.all(st["exp_avg"][hit_b] != 0) and float(st["step"]) == 1.0
    assert all(p.grad is None for g in sc.gaussians_assets for p in g._params().values())      # zero_grad(set_to_none=True) as before
    sc, moved = run(lambda_reg=0.0)                                                  # no regulariser: the actor is sparse too
    assert all(torch.equal(m, hit_a) for m in moved[1]) and all(torch.equal(m, hit_b) for m in moved[0])
    # fused without sparse: dense everywhere
    opt = options(fused_adam=True)
    sc = training.GaussianScene([make_asset(nb, 1)]); sc.training_setup(opt)
    fake_grads(sc.gaussians_assets[0], 5)
    x0 = sc.gaussians_assets[0]._xyz.detach().clone()
    sc.optimize(opt, 1, torch.randn(nb, 3), torch.zeros(nb, 1))
    assert bool((sc.gaussians_assets[0]._xyz.detach() != x0).any(1).all())
