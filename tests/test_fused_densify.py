"""The fused densify-and-prune without a GPU: the seventh product library (`liblrt_densify.so`: a source list and hash of its own that moves no
other hash, exports, resource gate, argument errors before the device is touched), the rule's header compiled for the host against the float64
twin, the twin against the existing `GaussianAsset.densify_and_prune` in CPU float32, and the switch of the training loop on the CPU path."""
import ctypes as C
import io
import os
import re
import struct
import subprocess
import types

import numpy as np
import pytest
import torch

from lidar_rt_amd import build as lrt_build, densify as dn, optim, resources, training
from tests import densify_cases as dc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


# ---- build ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def densify_lib():
    return lrt_build.build_densify()


def test_the_library_has_a_source_list_of_its_own_and_moves_no_other_hash():
    assert lrt_build.DENSIFY_SOURCES == ["lrt_densify.hip"] and "lrt_densify_math.h" in lrt_build.DENSIFY_HEADERS
    others = (lrt_build.SOURCES + lrt_build.HEADERS + lrt_build.LOSS_SOURCES + lrt_build.LOSS_HEADERS + lrt_build.GRIDCD_SOURCES + lrt_build.GRIDCD_HEADERS
              + lrt_build.INIT_SOURCES + lrt_build.INIT_HEADERS + lrt_build.METRICS_SOURCES + lrt_build.METRICS_HEADERS + lrt_build.ADAM_SOURCES + lrt_build.ADAM_HEADERS)
    assert not any("lrt_densify" in f for f in others)
    # the other libraries' hashes at the commit this library was added on: committed profiles are keyed by them
    assert lrt_build.source_hash() == "2c98b54882a7ff74"          # moved twice since: the non-finite-input fixes in lrt_chamfer.hip; a comment of include/lrt.h (lrt_xchg_apply, zero_only on an overflowed block)
    assert lrt_build.loss_source_hash() == "cc56b0c83f72d5ca"
    assert lrt_build.gridcd_source_hash() == "fd279d9f7ff67722"
    assert lrt_build.init_source_hash() == "0fd7105f5d08ab22"
    assert lrt_build.metrics_source_hash() == "9e8267ef6335030b"
    assert lrt_build.adam_source_hash() == "1b4949dcebd155a4"
    assert "lrt_densify" not in open(lrt_build.EXT_SRC).read()
    assert lrt_build.densify_source_hash() not in (lrt_build.source_hash(), lrt_build.loss_source_hash(), lrt_build.gridcd_source_hash(), lrt_build.init_source_hash(),
                                                   lrt_build.metrics_source_hash(), lrt_build.adam_source_hash())
    assert os.path.basename(lrt_build.DENSIFY_LIB) == "liblrt_densify.so"
    assert lrt_build.DENSIFY_LIB not in (lrt_build.LIB, lrt_build.LOSS_LIB, lrt_build.GRIDCD_LIB, lrt_build.INIT_LIB, lrt_build.METRICS_LIB, lrt_build.ADAM_LIB)
    src = open(lrt_build.__file__).read()
    assert "build_densify(force, verbose)" in src                                        # _build_product builds it
    assert "csrc/liblrt_densify.so" in open(os.path.join(REPO, "setup.py")).read()
    # the same code-generation flags, and hipcc's correctly rounded float32 division and sqrt left on: step 1 of the rule is one IEEE division
    body = src[src.index("def build_densify"):src.index("EXT_SRC =")]
    assert "CODEGEN_FLAGS" in body and "correctly-rounded" not in src and "fast-math" not in src


def test_the_library_builds_and_exports_what_its_header_declares(densify_lib):
    assert os.path.exists(densify_lib) and not lrt_build.densify_is_stale()
    assert open(lrt_build.DENSIFY_STAMP).read().strip() == lrt_build.densify_source_hash()
    hdr = open(os.path.join(REPO, "include", "lrt_densify.h")).read()
    declared = set(re.findall(r"\b(lrt_densify_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(dn.EXPORTS), declared ^ set(dn.EXPORTS)
    lib = dn.load()
    for n in declared:
        assert hasattr(lib, n), n
    exported = set(re.findall(r"\blrt_densify_[a-z_]+\b", subprocess.run(["nm", "-D", "--defined-only", densify_lib], capture_output=True, text=True, check=True).stdout))
    assert exported == declared, exported ^ declared
    const = lambda name: int(re.search(r"#define\s+%s\s+\(?(\d+)" % name, hdr).group(1))
    assert lib.lrt_densify_abi_version() == const("LRT_DENSIFY_ABI_VERSION") == dn.ABI_VERSION
    assert const("LRT_DENSIFY_MAX_GROUPS") == dn.MAX_GROUPS and const("LRT_DENSIFY_BLOCK_ROWS") == dn.BLOCK_ROWS == 256
    assert const("LRT_DENSIFY_SCAN_BLOCKS") == dn.SCAN_BLOCKS and const("LRT_DENSIFY_N_TOTALS") == dn.N_TOTALS


def test_the_kernels_pass_the_resource_gate(densify_lib):
    res = resources.kernel_resources(densify_lib)
    own = sorted(n for n in res if resources.is_own_kernel(n))
    assert own == ["k_densify_apply", "k_densify_plan", "k_densify_scan", "k_densify_stats"], own      # an event: plan + scan + apply
    assert all(any(re.search(g_, n) for g_ in resources.GATED) for n in own)
    assert resources.violations(res) == []
    for n in own:
        r = res[n]
        assert r["vgpr_spill"] == 0 and r["scratch_bytes"] == 0 and not r["dynamic_stack"], (n, r)
    resources.check(densify_lib)


def test_argument_errors_come_before_the_device_and_launch_nothing(densify_lib):
    lib = dn.load()
    buf = (C.c_char * 8192)()
    p = (C.addressof(buf) + 255) // 256 * 256
    err = lambda: lib.lrt_densify_last_error()
    nodev = 1 << 20                                                                     # a device that does not exist: what passes the checks ends there
    assert lib.lrt_densify_workspace_bytes(-1) < 0 and lib.lrt_densify_workspace_bytes((1 << 30) + 1) < 0
    for P in (0, 1, 256, 257, 1_000_000):
        nb = (P + 255) // 256
        r256 = lambda x: (x + 255) // 256 * 256
        assert lib.lrt_densify_workspace_bytes(P) == 256 + r256(P) + r256(48 * nb) + r256(32 * nb)
    # stats
    assert lib.lrt_densify_stats(nodev, -1, p, p, p, p, None) < 0 and b"-1 rows" in err()
    assert lib.lrt_densify_stats(nodev, 10, p, None, p, p, None) < 0 and b"null mean_grads / weights / accum / denom pointer" in err()
    assert lib.lrt_densify_stats(nodev, 10, p, p, p, p, None) < 0 and b"no HIP device" in err()
    # plan
    rule = dn._rule_struct(dc.rule(True, True))

    def plan(P=10, S=2, ptrs=None, box_noise=p, rule_=rule, ws=p, ws_bytes=4096, totals=p):
        a = [p] * 7 if ptrs is None else ptrs
        return lib.lrt_densify_plan(nodev, P, S, *a, box_noise, None if rule_ is None else C.byref(rule_), ws, ws_bytes, totals, None)
    assert plan(P=-1) < 0 and b"-1 rows" in err()
    assert plan(S=4) < 0 and b"4 floats per scaling row (2 or 3)" in err()
    assert plan(rule_=None) < 0 and b"null rule" in err()
    assert plan(totals=None) < 0 and b"null totals" in err()
    for k in range(7):
        assert plan(ptrs=[None if j == k else p for j in range(7)]) < 0 and b"null xyz / scaling" in err()
    assert plan(box_noise=None) < 0 and b"a box without box_noise" in err()
    assert plan(ws=p + 4) < 0 and b"256-byte aligned" in err()
    assert plan(ws_bytes=100) < 0 and b"a workspace of 100 bytes, 10 rows need" in err()
    bad = dn._rule_struct(dc.rule(True, True)); bad.box_min[1] = 5.0
    assert plan(rule_=bad) < 0 and b"box_min[1]" in err()
    nan = dn._rule_struct(dc.rule()); nan.opa_thr = float("nan")
    assert plan(rule_=nan) < 0 and b"a threshold is NaN" in err()
    assert plan() < 0 and b"no HIP device" in err()
    # apply
    grp = lambda **kw: dn._Group(**{**dict(src=p, src_exp_avg=p, src_exp_avg_sq=p, dst=p, dst_exp_avg=p, dst_exp_avg_sq=p, width=3, role=0), **kw})
    table = lambda: [grp(role=1), grp(width=2, role=2), grp(width=45)]

    def apply(groups, P=10, P_new=12, S=2, n=None, ws=p, ws_bytes=4096, rot=p):
        arr = (dn._Group * max(1, len(groups)))(*groups)
        return lib.lrt_densify_apply(nodev, P, P_new, S, rot, p, len(groups) if n is None else n, C.cast(arr, C.c_void_p), ws, ws_bytes, None)
    assert apply(table(), P_new=21) < 0 and b"21 rows out of 10" in err()
    assert apply([], n=0) < 0 and b"0 groups (1 .. 8 in one call)" in err()
    assert apply(table() + [grp(width=0)]) < 0 and b"group 3: width 0" in err()
    assert apply(table() + [grp(width=1025)]) < 0 and b"width 1025" in err()
    assert apply(table() + [grp(src=None)]) < 0 and b"group 3: null source pointer" in err()
    assert apply(table() + [grp(dst=None)]) < 0 and b"group 3: null destination pointer" in err()
    assert apply(table() + [grp(src_exp_avg=None)]) < 0 and b"one moment without the other" in err()
    assert apply(table() + [grp(dst_exp_avg_sq=None)]) < 0 and b"source moments without destination moments" in err()
    assert apply(table() + [grp(role=1)]) < 0 and b"the role xyz belongs to one group of width 3" in err()
    assert apply([grp(role=1), grp(width=3, role=2)]) < 0 and b"the role scaling belongs to one group of width 2" in err()
    assert apply(table() + [grp(role=7)]) < 0 and b"role 7" in err()
    assert apply([grp(role=1), grp()]) < 0 and b"needs a group with the role xyz and one with the role scaling" in err()
    assert apply(table(), rot=None) < 0 and b"null rotation / split_noise" in err()
    assert apply(table(), ws_bytes=8) < 0 and b"a workspace of 8 bytes" in err()
    assert apply(table()) < 0 and b"no HIP device" in err()
    assert apply(table() + [grp(src_exp_avg=None, src_exp_avg_sq=None, dst_exp_avg=None, dst_exp_avg_sq=None)]) < 0 and b"no HIP device" in err()


# ---- the rule's header on the host ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("densify_check") / "densify_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "host_check", "densify_check.cpp")])
    return exe


@pytest.mark.parametrize("S,box", [(2, False), (3, False), (2, True), (3, True)])
def test_the_rule_header_on_the_host_against_the_twin(host_check, tmp_path, S, box):
    """Every decision of every row equals the twin's (the cases keep the rows off the knife edges); the children's xyz and scaling and the
    accumulated gradient norm are evaluated in double and rounded once: within half a float32 ulp of the float64 value (the double roundings
    inside, ~1e-16 relative to the terms, are allowed for by the factor 1 + 1e-6 on the scale |xyz| + |offset|)."""
    P = 2000
    c = dc.build(P, 5, "mixed", S=S, box=box)
    rng = np.random.default_rng(9)
    mg = (rng.standard_normal((P, 3)) * 10.0 ** rng.uniform(-6, 0, (P, 1))).astype(np.float32)
    w = np.where(rng.uniform(size=P) < 0.5, 0.0, rng.uniform(size=P)).astype(np.float32)
    r = c.rule
    bn = c.box_noise if c.box_noise is not None else np.zeros((P, 2, 2, 3), np.float32)
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<4i", P, S, int(r.size_limit), int(r.has_box)))
        f.write(struct.pack("<10f", r.grad_thr, r.big_thr, r.huge_thr, r.opa_thr, *(r.box_min or (0, 0, 0)), *(r.box_max or (0, 0, 0))))
        for a in (c.groups["xyz"], c.groups["scaling"], c.groups["rotation"], c.groups["opacity"], c.accum, c.denom, c.split_noise, bn, mg, w):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    res = subprocess.run([host_check, inp, out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "DENSIFYCHECK ok" in res.stdout, res.stdout + res.stderr
    raw = open(out, "rb").read()
    code = np.frombuffer(raw, np.uint32, P); o = 4 * P
    cx = np.frombuffer(raw, np.float32, 6 * P, o).reshape(P, 2, 3); o += 24 * P
    cs = np.frombuffer(raw, np.float32, S * P, o).reshape(P, S); o += 4 * S * P
    acc2 = np.frombuffer(raw, np.float32, P, o); o += 4 * P
    den2 = np.frombuffer(raw, np.float32, P, o)
    g, m, a, d, sn, bnt = dc.tensors(c, "cpu")
    tw = dn.densify_reference(g, m, a, d, c.rule, sn, bnt)
    assert np.array_equal(code & 3, tw.kind.numpy())
    assert np.array_equal((code >> 2) & 1, tw.mark[:, 0].numpy().astype(np.uint32)) and np.array_equal((code >> 3) & 1, tw.mark[:, 1].numpy().astype(np.uint32))
    assert len(set((code & 3).tolist())) == 3 and ((code >> 2) & 1).sum() > 0
    n_bits = lambda lo_: int(((code >> lo_) & 1).sum() + ((code >> (lo_ + 1)) & 1).sum())
    assert (n_bits(4), n_bits(6), n_bits(8)) == (tw.n_opa, tw.n_scale, tw.n_outside)
    off = (tw.child_xyz - g["xyz"].double()[:, None, :]).abs()
    d_xyz = dc.distance(cx, tw.child_xyz, g["xyz"].double().abs()[:, None, :] + off)
    d_s = dc.distance(cs, tw.child_scaling)
    ta, td = dn.densify_stats_reference(a, d, torch.as_tensor(mg), torch.as_tensor(w))
    d_a = dc.distance(acc2, ta.reshape(-1))
    print(f"DENSIFYCHECK|host|S {S}|box {box}|children xyz {d_xyz:.4f} ulp|children scaling {d_s:.4f} ulp|accum {d_a:.4f} ulp")
    lim = 0.5 * (1.0 + 1e-6)
    assert d_xyz <= lim and d_s <= lim and d_a <= lim
    assert np.array_equal(den2.astype(np.float64), td.reshape(-1).numpy())


# ---- the twin against the existing path -----------------------------------------------------------------------------------------------------------------

def options(**kw):
    """default_options() with the thresholds of tests/densify_cases.py at extent 1."""
    opt = training.default_options()
    opt.densify_grad_threshold, opt.densify_scale_threshold, opt.prune_size_threshold, opt.thresh_opa_prune = dc.GRAD_THR, dc.BIG_THR, dc.HUGE_THR / 0.1, dc.OPA_THR
    for k, v in kw.items():
        setattr(opt, k, v)
    return opt


def asset_of(c, opt, step=True, box=None, device="cpu"):
    """A GaussianAsset holding the case, with the case's statistics and (step) one optimizer step behind it whose moments are the case's."""
    t = lambda a: torch.as_tensor(a, device=device)
    a = training.GaussianAsset.from_tensors(t(c.groups["xyz"]), t(c.groups["f_dc"]), t(c.groups["f_rest"]), t(c.groups["scaling"]), t(c.groups["rotation"]),
                                            t(c.groups["opacity"]), extent=1.0, dimension=c.S, bounding_box=box)
    a.training_setup(opt)
    if step:
        for n, p in a._params().items():
            p.grad = torch.zeros_like(p)
        a.optimizer.step(); a.optimizer.zero_grad(set_to_none=True)                      # zero gradients: the parameters stay, the state exists
        for n, p in a._params().items():
            st = a.optimizer.state[p]
            st["exp_avg"].copy_(t(c.moments[n][0])); st["exp_avg_sq"].copy_(t(c.moments[n][1]))
    a.xyz_gradient_accum, a.denom = t(c.accum).clone(), t(c.denom).clone()
    return a


def state_of(a):
    out = {}
    for n, p in a._params().items():
        st = a.optimizer.state.get(p, {})
        out[n] = (p.detach(), st.get("exp_avg"), st.get("exp_avg_sq"), None if "step" not in st else float(st["step"]))
    return out


@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("size_limit", [20, None])
def test_the_twin_against_the_existing_densify_and_prune_in_cpu_float32(S, size_limit):
    """Counts, row order and every tensor and moment are equal bit for bit; the children's xyz depends on the existing path's own normal draws
    and is left out, the children's scaling (log(exp(s) / 1.6) in float32 there) is within that expression's float32 error of the twin's."""
    P = 1500
    c = dc.build(P, 7, "mixed", S=S, size_limit=bool(size_limit))
    opt = options()
    a = asset_of(c, opt)
    g, m, acc, den, sn, _ = dc.tensors(c, "cpu")
    tw = dn.densify_reference(g, m, acc, den, dn.rule_of(opt, a.extent, a.densify_scale_threshold, size_limit), sn)
    assert vars(dn.rule_of(opt, a.extent, a.densify_scale_threshold, size_limit)) == vars(c.rule)
    torch.manual_seed(3)
    info = a.densify_and_prune(opt, size_limit)
    assert info == tw.info and min(info[:2]) > 0 and info[3] > 0 and (info[2] > 0) == bool(size_limit)
    assert a._xyz.shape[0] == tw.P_new != P and tw.prune_applied == 1
    child = (tw.slot >= 2)
    assert int(child.sum()) > 0 and int((tw.slot == 1).sum()) > 0
    for n, (p, ea, eas, step) in state_of(a).items():
        assert step == 1.0 and p.shape == tw.groups[n].shape, n
        if n in ("xyz", "scaling"):
            assert torch.equal(p[~child], tw.groups[n][~child].float()), n
        else:
            assert torch.equal(p, tw.groups[n]), n
        assert torch.equal(ea, tw.moments[n][0]) and torch.equal(eas, tw.moments[n][1]), n
        assert float(ea[tw.slot != 0].abs().sum()) == 0.0 and float(ea[tw.slot == 0].abs().sum()) > 0.0
    # log(exp(s) / 1.6) in float32: exp within 1 ulp (2^-23 relative, which the logarithm turns into an absolute 2^-23), float32(1.6) and the
    # division 2^-24 each, the logarithm within 1 ulp of its result -- 2^-22 + 2^-23 |result|; a result near 0 (s near log 1.6) carries the
    # absolute part, which is why the gate of the operator measures against this path and not against the result's own ulp alone
    got, want = a._scaling.detach()[child].double(), tw.groups["scaling"][child]
    err = (got - want).abs()
    print(f"FUSEDDENSIFY|cpu|existing path against the twin|S {S}|size_limit {size_limit}|children scaling: largest error {float(err.max()):.3e}, "
          f"{dc.distance(got, want):.3f} ulp of the result")
    assert torch.all(err <= 2.0 ** -22 + 2.0 ** -23 * want.abs())
    # the rows on the gradient threshold: row 1 (equal) and row 4 (x / 0) selected, row 2 (one float32 below) and row 3 (0 / 0) not
    assert [int(tw.kind[i]) > 0 for i in (1, 2, 3, 4)] == [True, False, False, True]


# ---- the CPU path under the gate, and the switch ------------------------------------------------------------------------------------------------------------

def test_the_cpu_path_equals_the_twin_in_structure_and_copies_and_passes_the_gate():
    for S, box in ((2, False), (3, True)):
        c = dc.build(1000, 8, "mixed", S=S, box=box)
        g, m, a, d, sn, bn = dc.tensors(c, "cpu")
        before = [t.clone() for t in list(g.values()) + [a, d]]
        tw, op = dn.densify_reference(g, m, a, d, c.rule, sn, bn), dn.densify(g, m, a, d, c.rule, sn, bn)
        assert all(torch.equal(x, y) for x, y in zip(before, list(g.values()) + [a, d]))           # the inputs are not changed
        assert (op.P_new, op.info, op.n_outside, op.prune_applied) == (tw.P_new, tw.info, tw.n_outside, tw.prune_applied)
        assert torch.equal(op.src, tw.src) and torch.equal(op.slot, tw.slot) and (tw.n_outside > 0) == box
        child = tw.slot >= 2
        for n in dn.GROUPS:
            assert op.groups[n].dtype == torch.float32
            assert torch.equal(op.groups[n][~child], tw.groups[n][~child].float()), n
            assert torch.equal(op.moments[n][0], tw.moments[n][0]) and torch.equal(op.moments[n][1], tw.moments[n][1])
        src, ch = tw.src[child], tw.slot[child] - 2
        tx, ts = dc.torch_children(g["xyz"], g["scaling"], g["rotation"], sn, src, ch)
        scale = g["xyz"][src].double().abs() + tw.offset[child]
        yard = (dc.distance(tx, tw.groups["xyz"][child], scale), dc.distance(ts, tw.groups["scaling"][child]))
        mine = (dc.distance(op.groups["xyz"][child], tw.groups["xyz"][child], scale), dc.distance(op.groups["scaling"][child], tw.groups["scaling"][child]))
        print(f"FUSEDDENSIFY|cpu|S {S}|box {box}|children xyz / scaling: torch float32 {yard[0]:.3f} {yard[1]:.3f} ulp|CPU path {mine[0]:.3f} {mine[1]:.3f} ulp")
        assert mine[0] <= dc.bound(yard[0]) and mine[1] <= dc.bound(yard[1])


def test_the_stats_on_the_cpu_path():
    P = 700
    rng = np.random.default_rng(2)
    acc = torch.as_tensor(rng.uniform(0, 1e-2, (P, 1)).astype(np.float32)); den = torch.as_tensor(rng.integers(0, 5, (P, 1)).astype(np.float32))
    mg = torch.as_tensor((rng.standard_normal((P, 3)) * 1e-3).astype(np.float32)); w = torch.as_tensor(np.where(rng.uniform(size=(P, 1)) < 0.4, 0, 0.7).astype(np.float32))
    ta, td = dn.densify_stats_reference(acc, den, mg, w)
    ref_a = acc + torch.norm(mg, dim=-1, keepdim=True); ref_d = den + (w > 0).float()
    a2, d2 = acc.clone(), den.clone()
    dn.densify_stats(a2, d2, mg, w)
    assert torch.equal(d2, ref_d) and torch.equal(d2.double(), td)
    assert dc.distance(a2, ta) <= dc.bound(dc.distance(ref_a, ta)) and dc.distance(a2, ta) <= 0.5 + 1e-6
    a3, d3 = acc.clone(), den.clone()
    dn.densify_stats(a3, d3, mg, (w > 0).reshape(-1))                                    # a bool filter means the same
    assert torch.equal(a3, a2) and torch.equal(d3, d2)
    with pytest.raises(dn.DensifyError, match="do not describe one asset"):
        dn.densify_stats(a2, d2, mg[:5], w)


def test_default_options_keep_the_switch_off_and_the_loop_unchanged():
    assert training.default_options().fused_densify is False
    c = dc.build(300, 9, "mixed")
    runs = []
    for kw in ({}, {"fused_densify": False}):
        opt = options(**kw)
        a = asset_of(c, opt)
        assert a.fused_densify is False
        torch.manual_seed(11)
        a.add_densification_stats(torch.ones(300, 3) * 1e-5, torch.arange(300) % 2 == 0)
        info = a.densify_and_prune(opt, 20)
        runs.append((info, [p.detach().clone() for p in a._params().values()]))
    assert runs[0][0] == runs[1][0] and all(torch.equal(x, y) for x, y in zip(runs[0][1], runs[1][1]))


@pytest.mark.parametrize("cls", [torch.optim.Adam, optim.GaussianAdam], ids=["torch_adam", "gaussian_adam"])
def test_the_switch_on_the_cpu_path_moves_the_optimizer_state(cls):
    P = 600
    c = dc.build(P, 10, "mixed")
    opt = options(fused_densify=True, fused_adam=cls is optim.GaussianAdam)
    a = asset_of(c, opt)
    assert type(a.optimizer) is cls and a.fused_densify
    g, m, acc, den, _, _ = dc.tensors(c, "cpu")
    torch.manual_seed(5)
    sn = torch.randn((P, 2, 3))                                                          # what the asset draws under this seed
    tw = dn.densify_reference(g, m, acc, den, c.rule, sn)
    torch.manual_seed(5)
    info = a.densify_and_prune(opt, 20)
    assert isinstance(info, tuple) and all(type(v) is int for v in info) and info == tw.info and a._xyz.shape[0] == tw.P_new != P
    child = tw.slot >= 2
    st = state_of(a)
    for n, (p, ea, eas, step) in st.items():
        assert step == 1.0 and torch.equal(ea, tw.moments[n][0]) and torch.equal(eas, tw.moments[n][1]), n     # `step` kept, the moments moved
        assert torch.equal(p[~child], tw.groups[n][~child].float()) and p.dtype == torch.float32
    assert dc.distance(a._xyz.detach()[child], tw.groups["xyz"][child], g["xyz"][tw.src[child]].double().abs() + tw.offset[child]) <= 0.5 + 1e-6
    assert len(a.optimizer.state) == 6 and all(p.grad is None and p.requires_grad and isinstance(p, torch.nn.Parameter) for p in a._params().values())
    assert all(pg["params"][0] is a._params()[pg["name"]] for pg in a.optimizer.param_groups)
    for t_, shape in ((a.xyz_gradient_accum, (tw.P_new, 1)), (a.denom, (tw.P_new, 1)), (a.max_radii2D, (tw.P_new,))):
        assert tuple(t_.shape) == shape and t_.is_contiguous() and float(t_.abs().sum()) == 0.0
    # the step of the same iteration skips the new parameters; the next one steps them
    x0 = a._xyz.detach().clone()
    a.optimizer.step()
    assert torch.equal(a._xyz.detach(), x0) and state_of(a)["xyz"][3] == 1.0
    for p in a._params().values():
        p.grad = torch.full_like(p, 1e-3)
    a.optimizer.step(); a.optimizer.zero_grad(set_to_none=True)
    assert not torch.equal(a._xyz.detach(), x0) and all(v[3] == 2.0 for v in state_of(a).values())
    # the statistics go through the operator too: the hit weights themselves, or a filter
    a.add_densification_stats(torch.full((tw.P_new, 3), 2e-3), (torch.arange(tw.P_new) % 3 == 0).float().reshape(-1, 1))
    assert float(a.denom.sum()) == float((torch.arange(tw.P_new) % 3 == 0).sum()) and abs(float(a.xyz_gradient_accum[0]) - 2e-3 * 3 ** 0.5) < 1e-9
    # capture() / restore()
    buf = io.BytesIO(); torch.save(a.capture(), buf); buf.seek(0)
    b = training.GaussianAsset(extent=1.0, dimension=c.S)
    b.restore(torch.load(buf, weights_only=False), opt)
    assert type(b.optimizer) is cls
    sa, sb = state_of(a), state_of(b)
    for n in sa:
        assert all(torch.equal(x, y) if torch.is_tensor(x) else x == y for x, y in zip(sa[n], sb[n])), n
    assert torch.equal(a.denom, b.denom) and torch.equal(a.xyz_gradient_accum, b.xyz_gradient_accum)
    # two events under one seed give equal bits
    outs = []
    for _ in range(2):
        a2 = asset_of(c, opt)
        torch.manual_seed(77)
        a2.densify_and_prune(opt, 20)
        outs.append(state_of(a2))
    for n in outs[0]:
        assert all(torch.equal(x, y) for x, y in zip(outs[0][n][:3], outs[1][n][:3])), n


def test_an_actor_draws_its_box_noise_after_the_split_noise():
    P = 400
    c = dc.build(P, 12, "mixed", box=True)
    box = types.SimpleNamespace(min_xyz=torch.tensor(dc.BOX_MIN), max_xyz=torch.tensor(dc.BOX_MAX), frame={})
    opt = options(fused_densify=True)
    a = asset_of(c, opt, box=box)
    g, m, acc, den, _, _ = dc.tensors(c, "cpu")
    torch.manual_seed(6)
    sn, bn = torch.randn((P, 2, 3)), torch.randn((P, 2, 2, 3))
    tw = dn.densify_reference(g, m, acc, den, c.rule, sn, bn)
    torch.manual_seed(6)
    info = a.densify_and_prune(opt, 20)
    assert info == tw.info and a._xyz.shape[0] == tw.P_new and tw.n_outside > 0
    # without a size limit the box is not looked at and no box noise is drawn
    a = asset_of(c, opt, box=box)
    torch.manual_seed(6)
    a.densify_and_prune(opt, None)
    torch.manual_seed(6)
    torch.randn((P, 2, 3))
    after = torch.randn(4)
    torch.manual_seed(6)
    a2 = asset_of(c, opt, box=box); a2.densify_and_prune(opt, None)
    assert torch.equal(torch.randn(4), after)


# ---- the edges ----------------------------------------------------------------------------------------------------------------------------------------------

def test_the_guard_holds_back_a_prune_of_every_output():
    c = dc.build(300, 13, "pruned")
    g, m, a, d, sn, bn = dc.tensors(c, "cpu")
    for f in (dn.densify_reference, dn.densify):
        r = f(g, m, a, d, c.rule, sn, bn)
        assert r.prune_applied == 0 and r.n_opa == r.P_new == 300 + r.n_clone + r.n_split and r.n_clone > 0 and r.n_split > 0
    # one output short of everything: applied
    c.groups["opacity"][7] = 2.0
    dc.assert_margins(c)
    g, m, a, d, sn, bn = dc.tensors(c, "cpu")
    r = dn.densify(g, m, a, d, c.rule, sn, bn)
    assert r.prune_applied == 1 and 1 <= r.P_new <= 2 and set(r.src.tolist()) == {7}


def test_an_empty_asset_no_state_yet_and_f_rest_of_width_zero():
    # P == 0
    c = dc.build(0, 14, "mixed")
    g, m, a, d, sn, bn = dc.tensors(c, "cpu")
    for f in (dn.densify_reference, dn.densify):
        r = f(g, m, a, d, c.rule, sn, bn)
        assert (r.P_new, r.info, r.n_outside) == (0, (0, 0, 0, 0), 0) and all(r.groups[n].shape == g[n].shape for n in dn.GROUPS)
    # no optimizer state yet, SH degree 0
    c = dc.build(200, 15, "mixed", sh_degree=0, moments=False)
    assert c.groups["f_rest"].shape == (200, 0, 3)
    g, m, a, d, sn, bn = dc.tensors(c, "cpu")
    tw, op = dn.densify_reference(g, None, a, d, c.rule, sn, bn), dn.densify(g, None, a, d, c.rule, sn, bn)
    assert op.moments is None and tw.moments is None and op.P_new == tw.P_new != 200 and op.groups["f_rest"].shape == (tw.P_new, 0, 3)
    assert torch.equal(op.groups["f_dc"], g["f_dc"][tw.src])
    opt = options(fused_densify=True)
    a_ = asset_of(c, opt, step=False)
    assert len(a_.optimizer.state) == 0
    torch.manual_seed(1)
    info = a_.densify_and_prune(opt, 20)
    assert len(a_.optimizer.state) == 0 and a_._xyz.shape[0] == a_._features_rest.shape[0] and sum(info) > 0
    for p in a_._params().values():
        p.grad = torch.zeros_like(p)
    a_.optimizer.step()                                                                  # the first step creates the state at the new length
    assert a_.optimizer.state[a_._xyz]["exp_avg"].shape == a_._xyz.shape
    with pytest.raises(dn.DensifyError, match="split_noise must be"):
        dn.densify(g, None, a, d, c.rule, sn[:5], bn)
    with pytest.raises(dn.DensifyError, match="needs two moments"):
        dn.densify(g, {"xyz": (g["xyz"], g["xyz"])}, a, d, c.rule, sn, bn)
