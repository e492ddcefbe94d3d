"""Ray-drop refinement without a GPU: the module against the reference's recorded outputs (tests/golden/refine_unet.npz), the folded batch
norms, refine_raydrop on CPU tensors, the training stage on a stub renderer, the refiner argument of the evaluation loop, and the GPU tests' own footing: which kernel
paths their cases reach (a restatement of the launcher), what their two gates reject (the float32 module with deliberate errors), and the twin of
the workspace plan."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from lidar_rt_amd import build as lrt_build
from lidar_rt_amd import raydrop_refine as rr
from lidar_rt_amd import resources
from tests import refine_cases as rc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the module against the reference --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [9, 3])
def test_state_dict_has_the_reference_names_order_and_shapes(C):
    want = rc.golden_state(C)
    assert len(want) == 112
    net = rr.RaydropUNet(C, 4)
    own = net.state_dict()
    assert list(own.keys()) == list(want.keys())
    assert [tuple(v.shape) for v in own.values()] == [tuple(v.shape) for v in want.values()]
    net.load_state_dict(want, strict=True)
    assert len(rr.RaydropUNet(C, 32).state_dict()) == 112                    # 112 entries at any width


@pytest.mark.parametrize("C,H,W", rc.GOLDEN_SHAPES)
def test_float64_twin_reproduces_the_recorded_outputs(C, H, W):
    g = rc.golden()
    net = rr.RaydropUNet(C, 4)
    net.load_state_dict(rc.golden_state(C), strict=True)
    net = net.double().eval()
    with torch.no_grad():
        p, z = net(torch.as_tensor(g[f"x{C}_{H}x{W}"]).double(), return_logits=True)
    ez = float((z - torch.as_tensor(g[f"logit{C}_{H}x{W}"]).double()).abs().max())
    ep = float((p - torch.as_tensor(g[f"prob{C}_{H}x{W}"]).double()).abs().max())
    print(f"{C} inputs {H}x{W}: logits {ez:.3e}, probabilities {ep:.3e}")
    assert p.shape == (1, 1, H, W)
    assert ez <= 1e-5 and ep <= 1e-5


def test_golden_shapes_reach_the_edge_cases():
    # 18 x 38: 9x19, 4x9, 2x4, 1x2 -- a bottom of one row (an upsampling source of size 1, T = 2) and odd sizes with one-sided padding on both axes
    assert [(18 >> i, 38 >> i) for i in range(5)][-1] == (1, 2)
    assert (33 >> 1) * 2 != 33 and (75 >> 1) * 2 != 75 and (18 >> 1) % 2 == 1 and (38 >> 1) % 2 == 1


# ---- pack ---------------------------------------------------------------------------------------------------------------------------------------------

def test_folded_affine_equals_batch_norm_in_float64():
    net = rc.network(9, 8)
    g = torch.Generator().manual_seed(5)
    n = 0
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            a, b = rr.fold_bn(m)
            assert a.dtype == b.dtype == torch.float32
            x = torch.randn((1, m.num_features, 3, 5), generator=g, dtype=torch.float64) * 3.0
            m64 = torch.nn.BatchNorm2d(m.num_features).double().eval()
            m64.load_state_dict(m.state_dict())
            want = m64(x)
            got = a.double()[None, :, None, None] * x + b.double()[None, :, None, None]
            # a and b are float32 roundings of the float64 values: 2^-24 relative each
            bound = 2.0 ** -23 * (a.double().abs()[None, :, None, None] * x.abs() + b.double().abs()[None, :, None, None]) + 1e-12
            assert bool(((got - want).abs() <= bound).all())
            n += 1
    assert n == 18


def test_pack_layout_and_refusals():
    net = rc.network(9, 8)
    pk = rr.pack(net)
    assert pk.params.dtype == torch.float32 and pk.params.numel() == rr.param_count(9, 8) and pk.in_channels == 9 and pk.channels == 8
    c = 8
    w_in = pk.params[:9 * c].reshape(9, c)
    assert torch.equal(w_in, net.inc.conv.weight.detach().reshape(c, 9).t())
    off = 9 * c + c
    a, b = rr.fold_bn(net.down1.conv.double_conv[0])
    assert torch.equal(pk.params[off:off + c], a) and torch.equal(pk.params[off + c:off + 2 * c], b)
    w = pk.params[off + 2 * c:off + 2 * c + 9 * c * 2 * c].reshape(3, 3, c, 2 * c)
    assert torch.equal(w, net.down1.conv.double_conv[3].weight.detach().permute(2, 3, 1, 0))
    assert float(pk.params[-1]) == float(net.outc.conv[2].bias.detach())
    assert pk.backend is None and rr.pack(net, backend="hip").backend == "hip" and rr.DEFAULT_CUDA_BACKEND in ("hip", "torch")
    with pytest.raises(ValueError, match="multiple of 8"):
        rr.pack(rr.RaydropUNet(9, 12))
    with pytest.raises(ValueError, match="multiple of 8"):
        rr.pack(rr.RaydropUNet(9, 4))


# ---- refine_raydrop on CPU tensors ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [9, 3])
def test_refine_raydrop_on_cpu_tensors_equals_the_module(C):
    H, W = 18, 38
    net = rc.network(C, 8)
    render, rays = rc.frame(H, W)
    rays = rays if C == 9 else None
    x = rr.refine_inputs(render, rays)
    assert x.shape == (1, C, H, W)
    assert torch.equal(x[0, 0], render["raydrop"][..., 0]) and torch.equal(x[0, 1], render["intensity"][..., 0]) and torch.equal(x[0, 2], render["depth"][..., 0])
    if C == 9:
        assert torch.equal(x[0, 3:6], rays[0].permute(2, 0, 1)) and torch.equal(x[0, 6:9], rays[1].permute(2, 0, 1))
    with torch.no_grad():
        want_p, want_z = net(x, return_logits=True)
    for packed in (rr.pack(net), net):
        p, z = rr.refine_raydrop(render, rays, packed, return_logits=True)
        assert p.shape == z.shape == (H, W, 1) and p.dtype == torch.float32
        assert torch.equal(p, want_p.reshape(H, W, 1)) and torch.equal(z, want_z.reshape(H, W, 1))
    out = torch.zeros((H, W, 1))
    assert rr.refine_raydrop(render, rays, net, out=out) is out and torch.equal(out, want_p.reshape(H, W, 1))
    # a module left in train() is still evaluated with the stored statistics and without dropout, and comes back in train()
    net2 = rr.RaydropUNet(C, 8)
    net2.load_state_dict(net.state_dict())
    net2.train()
    assert torch.equal(rr.refine_raydrop(render, rays, net2), want_p.reshape(H, W, 1)) and net2.training
    with pytest.raises(rr.RefineError, match="hip"):
        rr.refine_raydrop(render, rays, rr.pack(net), backend="hip")


def test_the_cases_really_randomise_the_batch_norm_statistics():
    net = rc.network(9, 8)
    plain = rr.RaydropUNet(9, 8)
    sd = {k: v for k, v in net.state_dict().items()}
    for k, v in plain.state_dict().items():
        if "running_" in k:
            sd[k] = v                                                        # default statistics: mean 0, variance 1
    plain.load_state_dict(sd)
    plain.eval()
    render, rays = rc.frame(18, 38)
    a = rr.refine_raydrop(render, rays, net, return_logits=True)[1]
    b = rr.refine_raydrop(render, rays, plain, return_logits=True)[1]
    assert float((a - b).abs().max()) > 1e-2


# ---- the training stage ------------------------------------------------------------------------------------------------------------------------------------

class _Sensor:
    def __init__(self, n, H=16, W=32):
        g = torch.Generator().manual_seed(9)
        self.H, self.W = H, W
        self.masks = {f: torch.rand((H, W), generator=g) > 0.3 for f in range(n)}
        self.rays = {f: rc.frame(H, W, seed=f)[1] for f in range(n)}
        self.calls = []

    def get_mask(self, f):
        return self.masks[f]

    def get_range_rays(self, f):
        return self.rays[f]

    def render(self, f):
        self.calls.append(f)
        return rc.frame(self.H, self.W, seed=f)[0]


def test_train_refiner_same_seed_same_weights_and_every_frame_before_a_repeat():
    runs = []
    for seed in (3, 3, 4):
        s = _Sensor(5)
        log = []
        net = rr.train_refiner(s.render, s, range(5), epochs=3, batch=4, seed=seed, channels=8, log=log)
        assert net.training and net.in_channels == 9 and net.channels == 8
        assert len(s.calls) == 12 and [len(r["frames"]) for r in log] == [4, 4, 4] and all(np.isfinite(r["loss"]) for r in log)
        assert sorted(s.calls[:5]) == [0, 1, 2, 3, 4] and sorted(s.calls[5:10]) == [0, 1, 2, 3, 4]      # the stack is emptied before it is refilled
        runs.append((net.state_dict(), list(s.calls)))
    assert runs[0][1] == runs[1][1] and all(torch.equal(a, b) for a, b in zip(runs[0][0].values(), runs[1][0].values()))
    assert any(not torch.equal(a, b) for a, b in zip(runs[0][0].values(), runs[2][0].values()))
    fresh = rr.RaydropUNet(9, 8).state_dict()
    assert list(runs[0][0].keys()) == list(fresh.keys())
    assert int(runs[0][0]["down1.conv.double_conv.0.num_batches_tracked"]) == 12                          # train() mode: one update per frame


def test_train_refiner_accumulates_a_batch_before_one_adam_step(monkeypatch):
    steps = []
    real = torch.optim.Adam.step

    def counting(self, *a, **k):
        steps.append(1)
        return real(self, *a, **k)
    monkeypatch.setattr(torch.optim.Adam, "step", counting)
    s = _Sensor(3)
    net0 = rr.RaydropUNet(3, 8)
    before = {k: v.clone() for k, v in net0.state_dict().items()}
    grads = []
    h = net0.inc.conv.weight.register_hook(lambda g: grads.append(g.clone()))
    net = rr.train_refiner(s.render, s, range(3), in_spatial=False, epochs=2, batch=3, seed=0, net=net0)
    h.remove()
    assert net is net0 and len(steps) == 2 and len(s.calls) == 6 and len(grads) == 6
    # Adam's first step moves every weight with a gradient by lr, whatever the gradient's size: one step of 1e-3, not three
    moved = (net.state_dict()["inc.conv.weight"] - before["inc.conv.weight"]).abs().max()
    assert 0.0 < float(moved) <= 2.0 * 1e-3 * 1.0001


def test_the_column_roll_moves_labels_with_inputs():
    s = _Sensor(1)
    render = s.render(0)
    x0, l0 = rr.refine_sample(render, s.rays[0], s.masks[0], 0)
    x7, l7 = rr.refine_sample(render, s.rays[0], s.masks[0], 7)
    assert x0.shape == (1, 9, 16, 32) and l0.shape == (16 * 32, 1)
    assert torch.equal(l0.reshape(16, 32), (~s.masks[0]).float())
    assert torch.equal(x7, torch.roll(x0, -7, dims=-1)) and torch.equal(l7.reshape(16, 32), torch.roll(l0.reshape(16, 32), -7, dims=-1))
    assert torch.equal(x7[0, 0, :, 0], render["raydrop"][:, 7, 0]) and torch.equal(l7.reshape(16, 32)[:, 0], (~s.masks[0][:, 7]).float())
    # with a roll the training draws it for input and labels alike: the stage still runs and visits the frames
    net = rr.train_refiner(s.render, s, [0], rot=True, epochs=1, batch=2, channels=8)
    assert len(s.calls) == 3 and net.training


# ---- the loop's argument -------------------------------------------------------------------------------------------------------------------------------------

def test_render_frames_hands_each_render_to_the_refiner(monkeypatch):
    from lidar_rt_amd import evaluation, renderer

    class _Tracer:
        training, deferred_checks = True, False

        def eval(self): self.training = False
        def train(self, mode=True): self.training = mode
        def check(self): pass
    monkeypatch.setattr(renderer, "tracer_2dgs", _Tracer())
    H, W = 16, 32
    s = _Sensor(2, H, W)
    monkeypatch.setattr(renderer, "raytracing", lambda f, *a, **k: dict(rc.frame(H, W, seed=f)[0]))
    net = rc.network(9, 8)
    plain = evaluation.render_frames([], s, [0, 1], torch.zeros(3))
    refined = evaluation.render_frames([], s, [0, 1], torch.zeros(3), refiner=net)
    for f in (0, 1):
        assert torch.equal(plain[f]["raydrop"], rc.frame(H, W, seed=f)[0]["raydrop"])
        assert torch.equal(refined[f]["raydrop"], rr.refine_raydrop(rc.frame(H, W, seed=f)[0], s.rays[f], net))
        assert torch.equal(refined[f]["depth"], plain[f]["depth"]) and not torch.equal(refined[f]["raydrop"], plain[f]["raydrop"])
    net3 = rc.network(3, 8)
    r3 = evaluation.render_frames([], s, [1], torch.zeros(3), refiner=net3)
    assert torch.equal(r3[1]["raydrop"], rr.refine_raydrop(rc.frame(H, W, seed=1)[0], None, net3))


# ---- what the cases of the GPU tests reach ---------------------------------------------------------------------------------------------------------------------

def conv_launches(c, H, W):
    """Every k_rf_conv launch of one frame in stream order, (layer, taps, pixels, Cin, Cout): the loop over the pairs in lrt_refine_forward
    (lrt_refine.hip, `for (int i = 0; i < RF_PAIRS; i++)`) with rf_pair_channels of lrt_refine_math.h -- in, out and level per pair in units of c,
    the middle width the output's going down and the input's going up -- and the two 1 x 1 projections of the attention block before pair 4."""
    n = [(H >> l) * (W >> l) for l in range(5)]
    names = ("down1", "down2", "down3", "down4", "up1", "up2", "up3", "up4")
    out = []
    for i, (ci, co, lvl) in enumerate(zip((1, 2, 4, 8, 16, 8, 4, 2), (2, 4, 8, 8, 4, 2, 1, 1), (1, 2, 3, 4, 3, 2, 1, 0))):
        if i == 4:
            out += [("attn.qkv", 1, n[4], 8 * c, 24 * c), ("attn.proj", 1, n[4], 8 * c, 8 * c)]
        cm = co if i < 4 else ci
        out += [(names[i] + ".1", 9, n[lvl], ci * c, cm * c), (names[i] + ".2", 9, n[lvl], cm * c, co * c)]
    return out


def conv_variant(pixels, Cin, Cout):
    """(NT, KS, m_tiles) as launch_conv of lrt_refine.hip chooses them: one 32 x 32 tile per wave gives `waves`; at most 2048 of them and Cin a
    multiple of 8 x 4: K split over the four waves; an even number of column tiles and at least 4096 waves of two tiles: NT = 2; else the plain kernel."""
    m_tiles, n_tiles = (pixels + 31) // 32, (Cout + 31) // 32
    waves = m_tiles * n_tiles
    if waves <= 2048 and Cin % 32 == 0:
        return 1, 4, m_tiles
    if n_tiles % 2 == 0 and waves // 2 >= 4096:
        return 2, 1, m_tiles
    return 1, 1, m_tiles


def paths_of(case):
    """{(path, (NT, KS))} that one case runs; the paths are those listed in tests/refine_cases.py.  Attention and the frame's size have no variant."""
    C, c, H, W = case
    reached = set()
    for layer, taps, pixels, Cin, Cout in conv_launches(c, H, W):
        NT, KS, m_tiles = conv_variant(pixels, Cin, Cout)
        c_per = Cin // KS                                                    # k_rf_conv: `c_per = g.Cin / KS`, the channel range of one wave
        if c_per > 32 and c_per % 32 != 0:                                   # `for (; c0 + 32 <= c_end; ...)` runs and leaves a rest to `for (; c0 < c_end; ...)`
            reached.add(("1", (NT, KS)))
        if Cout > 32 and Cout % 32 != 0:                                     # `col_ok[t] = n0 + 32 t + r < g.Cout` is false on some lanes of a tile with n0 + 32 t >= 32
            reached.add(("2", (NT, KS)))
        if NT == 2 and pixels % 32 != 0 and m_tiles % 4 != 0:                # `if (q < n_pix)` in the store, `if (tile * 32 >= n_pix) return` for whole waves
            reached.add(("3", (NT, KS)))
        if (H >> 4, W >> 4) == (1, 1) and pixels < 32 and (NT, KS) == (1, 1):
            reached.add(("5 a level under 32 pixels", (NT, KS)))
    T = (H >> 4) * (W >> 4)
    if T > 64 and T % 64 != 0:                                               # k_rf_attn: `for (int s = lane; s < T; s += 64)` ends on different rounds for different lanes
        reached.add(("4 ragged", None))
    if T == 1:
        reached.add(("4 one token", None))
    if (H >> 4, W >> 4) == (1, 1):                                           # rf_up_scale(1) = 0: up1 samples a single pixel
        reached.add(("5 a 1 x 1 bottom", None))
    return reached


def test_the_new_cases_reach_what_the_first_ones_never_run(refine_lib):
    old = set().union(*(paths_of(case) for case in rc.CASES))
    new = set().union(*(paths_of(case) for case in rc.NEW_CASES))
    # the first cases run all three kernel variants and none of the paths; NT = 2 only at 64 x 2048, where pixels and tiles are exact
    variants = {conv_variant(p, ci, co)[:2] for case in rc.CASES for _, _, p, ci, co in conv_launches(case[1], case[2], case[3])}
    assert variants == {(1, 4), (2, 1), (1, 1)}
    assert old == set(), old
    # paths 1 and 2 can occur in every variant (at NT = 2 only from 131072 pixels on at a width other than 32: the last case), path 3 at NT = 2,
    # a level under 32 pixels only in the plain kernel: the K-split kernel has one tile per workgroup whatever the level's size
    want = {("1", (1, 4)), ("1", (1, 1)), ("1", (2, 1)), ("2", (1, 4)), ("2", (1, 1)), ("2", (2, 1)), ("3", (2, 1)), ("4 ragged", None), ("4 one token", None),
            ("5 a level under 32 pixels", (1, 1)), ("5 a 1 x 1 bottom", None)}
    assert new == want, new ^ want
    assert {("3", (2, 1))} == paths_of((9, 32, 65, 2017)) - {("4 ragged", None)}
    assert {case[1] for case in rc.CASES + rc.NEW_CASES} == set(rc.WIDTHS) and {case[0] for case in rc.NEW_CASES} == {3, 9}
    lib = rr.load()
    assert [c for c in range(0, 81, 8) if lib.lrt_refine_work_bytes(64, 256, 9, c) > 0] == list(rc.WIDTHS)
    # the attention sizes that the issue names, and the long chain of the widest network
    tokens = {case: (case[2] >> 4) * (case[3] >> 4) for case in rc.NEW_CASES}
    assert tokens[(9, 24, 80, 210)] == 65 and tokens[(9, 8, 17, 1100)] == 68 and tokens[(9, 32, 65, 2017)] == 504 and tokens[(9, 8, 16, 16)] == 1
    assert max(taps * Cin for _, taps, _, Cin, _ in conv_launches(64, 33, 75)) == 9216
    assert len(set(rc.CASES + rc.NEW_CASES)) == len(rc.CASES) + len(rc.NEW_CASES) == 26


@pytest.mark.parametrize("C,c,H,W", rc.NEW_CASES, ids=lambda v: str(v))
def test_the_new_cases_keep_the_conditions_of_the_mask_test(C, c, H, W):
    z64, z32, e_f32 = rc.references(C, c, H, W)
    assert bool(torch.isfinite(z64).all()) and bool(torch.isfinite(z32).all()) and 0.0 < e_f32 < 1e-5
    near = (z64 - rc.LOGIT_04).abs() <= rc.K * e_f32
    differ32 = (torch.sigmoid(z32) < 0.4) != (z64 < rc.LOGIT_04)
    drops = float((z64 < rc.LOGIT_04).double().mean())
    print(f"refine {C} inputs, channels {c}, {H}x{W}: e_f32 {e_f32:.3e}, {int(near.sum())} near, float32 module {int(differ32.sum())} differ, "
          f"allowance {rc.MASK_CAP * H * W:.1f} pixels, {drops:.2f} of the mask dropped")
    assert int(near.sum()) <= rc.MASK_CAP * H * W and int(differ32.sum()) <= rc.MASK_CAP * H * W
    assert 0.0 < drops < 1.0                                                 # hits and drops alike: the mask comparison is not vacuous


# ---- negative controls: what the two gates of the GPU tests reject ----------------------------------------------------------------------------------------------

def _stand_in(case, damage):
    """(logit error, e_f32 of the logits, layer ratios) of the float32 CPU module with one deliberate error, gated exactly as the operator is."""
    import copy
    C, c, H, W = case
    net = copy.deepcopy(rc.network(C, c))
    with torch.no_grad():
        damage(net)
    z, got = rc.collect(net, rc.case_input(C, H, W))
    z64, _, e_f32 = rc.references(C, c, H, W)
    b64, _, layer_e_f32 = rc.layer_references(C, c, H, W)
    return float((z.double() - z64).abs().max()), e_f32, rc.layer_ratios(got, b64, layer_e_f32)


def _drop_the_last_key(net):
    def attend(x):                                                           # RaydropUNet._attend with every softmax over the keys 0 .. T - 2
        a = net.attn
        B, Cc, H, W = x.shape
        d = Cc // rr.HEADS
        qkv = a.proj_qkv(a.norm(x)).reshape(B, 3, rr.HEADS, d, H * W)
        q, k, v = qkv[:, 0], qkv[:, 1][..., :-1], qkv[:, 2][..., :-1]
        w = (q.transpose(-1, -2) @ k) * (int(d) ** -0.5)
        h = (torch.softmax(w, dim=-1) @ v.transpose(-1, -2)).contiguous()
        return x + a.proj(h.reshape(B, H, W, Cc).permute(0, 3, 1, 2))
    net._attend = attend


def test_an_undamaged_stand_in_passes_both_gates():
    e_op, e_f32, ratios = _stand_in((9, 24, 33, 75), lambda net: None)
    assert e_op <= e_f32 and rc.rejected_layers(ratios, 1.0) == []


def test_a_softmax_short_of_one_key_passes_the_logit_gate_and_fails_the_layer_gate():
    # T = 65: the key that a loop over whole rounds of 64 lanes would lose.  The logits move by less than the float32 module's own error, which
    # is why the layers are gated: this assertion records it, the next ones are the gate
    e_op, e_f32, ratios = _stand_in((9, 24, 80, 210), _drop_the_last_key)
    print(f"last key dropped: logits {e_op:.3e} against a gate of {rc.K * e_f32:.3e}; HB {ratios['HB'][2]:.1f}, X4A {ratios['X4A'][2]:.1f} times their allowances")
    assert e_op <= rc.K * e_f32
    bad = rc.rejected_layers(ratios, rc.K_CAP)
    assert "HB" in bad and "X4A" in bad and not set(bad) & {"X0", "M1", "X1", "M2", "X2", "M3", "X3", "M4", "X4", "QKV"}


def test_lost_remainder_channels_fail_both_gates():
    # channels = 24: the first convolution of down2 sums 48 input channels per tap, 32 in a four-group step and 16 in two single steps
    def damage(net):
        net.down2.conv.double_conv[3].weight[:, 32:48] = 0.0
    e_op, e_f32, ratios = _stand_in((9, 24, 33, 75), damage)
    print(f"remainder channels lost: logits {e_op / (rc.K * e_f32):.0f} gates, M2 {ratios['M2'][2]:.0f} allowances")
    assert e_op > rc.K * e_f32 and e_op > rc.K_CAP * e_f32
    bad = rc.rejected_layers(ratios, rc.K_CAP)
    assert bad[0] == "M2" and "X0" not in bad and "M1" not in bad and "X1" not in bad


def test_lost_output_channels_of_a_partial_column_tile_fail_both_gates():
    # channels = 24: the first convolution of down1 writes 48 output channels, the second column tile holds 16
    def damage(net):
        net.down1.conv.double_conv[3].weight[32:] = 0.0
    e_op, e_f32, ratios = _stand_in((9, 24, 33, 75), damage)
    print(f"output channels lost: logits {e_op / (rc.K * e_f32):.0f} gates, M1 {ratios['M1'][2]:.0f} allowances")
    assert e_op > rc.K * e_f32 and e_op > rc.K_CAP * e_f32
    bad = rc.rejected_layers(ratios, rc.K_CAP)
    assert bad[0] == "M1" and "X0" not in bad


# ---- the library ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def refine_lib():
    return lrt_build.build_refine()


def test_the_library_has_a_source_list_of_its_own_and_moves_no_other_hash():
    assert lrt_build.REFINE_SOURCES == ["lrt_refine.hip"] and "lrt_refine_math.h" in lrt_build.REFINE_HEADERS and "lrt_device_guard.h" in lrt_build.REFINE_HEADERS
    others = (lrt_build.SOURCES + lrt_build.HEADERS + lrt_build.LOSS_SOURCES + lrt_build.LOSS_HEADERS + lrt_build.GRIDCD_SOURCES + lrt_build.GRIDCD_HEADERS
              + lrt_build.INIT_SOURCES + lrt_build.INIT_HEADERS + lrt_build.METRICS_SOURCES + lrt_build.METRICS_HEADERS + lrt_build.ADAM_SOURCES + lrt_build.ADAM_HEADERS
              + lrt_build.DENSIFY_SOURCES + lrt_build.DENSIFY_HEADERS + lrt_build.PROJECT_SOURCES + lrt_build.PROJECT_HEADERS + lrt_build.SWEEP_SOURCES + lrt_build.SWEEP_HEADERS)
    assert not any("lrt_refine" in f for f in others)
    hashes = [getattr(lrt_build, fn)() for fn in ("source_hash", "loss_source_hash", "gridcd_source_hash", "init_source_hash", "metrics_source_hash",
                                                  "adam_source_hash", "densify_source_hash", "project_source_hash", "sweep_source_hash")]
    assert lrt_build.refine_source_hash() not in hashes and "lrt_refine" not in open(lrt_build.EXT_SRC).read()
    assert os.path.basename(lrt_build.REFINE_LIB) == "liblrt_refine.so" and os.path.basename(lrt_build.REFINE_STAMP) == "liblrt_refine.srchash"
    src = open(lrt_build.__file__).read()
    assert "build_refine(force, verbose)" in src[src.index("def _build_product"):src.index("def _build_lib")]
    assert "csrc/liblrt_refine.so" in open(os.path.join(REPO, "setup.py")).read()
    body = src[src.index("def build_refine"):src.index("EXT_SRC =")]
    assert "CODEGEN_FLAGS" in body and "resources.check(REFINE_LIB)" in body


def test_the_library_builds_and_exports_what_its_header_declares(refine_lib):
    assert os.path.exists(refine_lib) and not lrt_build.refine_is_stale()
    assert open(lrt_build.REFINE_STAMP).read().strip() == lrt_build.refine_source_hash()
    hdr = open(os.path.join(REPO, "include", "lrt_refine.h")).read()
    declared = set(re.findall(r"\b(lrt_refine_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(rr.EXPORTS), declared ^ set(rr.EXPORTS)
    exported = set(re.findall(r"\blrt_refine_[a-z_]+\b", subprocess.run(["nm", "-D", "--defined-only", refine_lib], capture_output=True, text=True, check=True).stdout))
    assert exported == declared, exported ^ declared
    const = lambda name: int(re.search(r"#define\s+%s\s+\(?(\d+)" % name, hdr).group(1))
    assert const("LRT_REFINE_ABI_VERSION") == rr.ABI_VERSION and const("LRT_REFINE_HEADS") == rr.HEADS
    assert const("LRT_REFINE_MAX_TOKENS") == rr.MAX_TOKENS and const("LRT_REFINE_MAX_PIXELS") == rr.MAX_PIXELS
    # the size checks are host code: they answer without a device
    lib = rr.load()
    assert lib.lrt_refine_abi_version() == rr.ABI_VERSION
    for C, c in ((9, 32), (3, 8), (9, 64)):
        assert lib.lrt_refine_param_count(C, c) == rr.param_count(C, c) == sum(p.numel() for p in rr.RaydropUNet(C, c).parameters())     # a and b take the place of a batch norm's weight and bias
    assert rr.work_bytes(64, 2048, 9, 32) % 256 == 0
    # every intermediate of a 64 x 2048 frame at channels = 32, in floats: levels of 131072, 32768, 8192, 2048, 512 pixels
    n = [131072, 32768, 8192, 2048, 512]
    floats = 32 * (n[0] * (1 + 2 + 1) + n[1] * (2 + 2 + 4 + 1) + n[2] * (4 + 4 + 8 + 2) + n[3] * (8 + 8 + 16 + 4) + n[4] * (8 + 8 + 24 + 8 + 8))
    assert rr.work_bytes(64, 2048, 9, 32) == 4 * floats
    for H, W, msg in ((1024, 1024, "tokens"), (8, 64, "16 x 16"), (8192, 8192, "pixels")):
        with pytest.raises(rr.RefineError, match=msg):
            rr.work_bytes(H, W, 9, 32)
    with pytest.raises(rr.RefineError, match="multiple of 8"):
        rr.work_bytes(64, 256, 9, 12)


def test_the_plan_twin_has_the_size_of_the_operators_workspace(refine_lib):
    lib = rr.load()
    for C, c, H, W in rc.CASES + rc.NEW_CASES:
        offsets, total = rc.plan(c, H, W)
        assert list(offsets) == list(rc.BUFFERS) and len(offsets) == 20
        assert 4 * total == lib.lrt_refine_work_bytes(H, W, C, c) == rr.work_bytes(H, W, C, c), (C, c, H, W)
        end = 0
        for b, (off, level, ch) in offsets.items():                          # nothing is aliased: each buffer starts at or behind the end of the one before
            assert off % 64 == 0 and off >= end and 0 <= level <= 4 and ch % c == 0
            end = off + (H >> level) * (W >> level) * ch
        assert end <= total


def test_the_kernels_pass_the_resource_gate(refine_lib):
    res = resources.kernel_resources(refine_lib)
    own = sorted(n for n in res if resources.is_own_kernel(n))
    assert all(n.startswith("k_rf_") for n in own), own
    assert sorted({n.split("<")[0] for n in own}) == ["k_rf_attn", "k_rf_conv", "k_rf_in", "k_rf_out"]
    # three sources of 3 x 3 and the 1 x 1, each with one column tile per wave, with two, and with K split over the workgroup's waves
    assert sum(n.startswith("k_rf_conv<") for n in own) == 12
    assert resources.violations(res) == []
    text = open(os.path.join(REPO, "lidar_rt_amd", "csrc", "lrt_refine.hip")).read()
    code = re.sub(r"//.*", "", text)
    assert "atomic" not in code and "hipMalloc" not in code and "Synchronize" not in code
    assert "__builtin_amdgcn_mfma_f32_32x32x2f32" in code and "bf16" not in code and "fp8" not in code
