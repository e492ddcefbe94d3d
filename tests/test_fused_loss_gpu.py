"""The fused range-image loss (`losses.range_image_loss`, csrc/liblrt_loss.so) on the GPU.

Accuracy rule (every numeric comparison below): the reference is `losses.range_image_loss_torch` in FLOAT64 on the same inputs; the yardstick is
the distance of the FLOAT32 torch path (the same function on the float32 inputs, on the GPU) from it; the fused operator's distance -- absolute
for the scalars, relative L2 over the tensor for `d_rendered` -- may be at most 2 x the yardstick's, with a floor of one float32 ulp of the
result (a float32 output cannot be asked to lie nearer to the float64 value than its own spacing; where the yardstick is 0 the floor is the bound).
Every figure is printed before it is asserted (`FUSEDLOSS|...` lines; profiles/fused_loss.md holds a recorded set)."""
import ctypes as C
import json
import os
import subprocess
import sys
import time
import types

import numpy as np
import pytest
import torch

from lidar_rt_amd import losses, scenes, training

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
DEV = torch.device("cuda:0")
WEIGHTS = ("lambda_depth_l1", "lambda_intensity_l1", "lambda_intensity_l2", "lambda_intensity_dssim", "lambda_raydrop_bce")
SIZES = ("golden", (64, 2048), (66, 1030), (64, 2650), (5, 7), (11, 200))


def _inputs(size, mask_kind, seed=0):
    """A seeded case: intensity in [0, 1], depth in [0, 40] m, logits scaled so that some probabilities land beyond the clamp on both sides."""
    g = torch.Generator().manual_seed(seed)
    if size == "golden":                                            # the reference's recorded 16 x 64 image pair as rendered / ground-truth intensity
        G = np.load(os.path.join(HERE, "golden", "loop_golden.npz"))
        a, b = torch.as_tensor(G["loss_img_a"])[0], torch.as_tensor(G["loss_img_b"])[0]
        H, W = a.shape
    else:
        H, W = size
        a, b = torch.rand(H, W, generator=g), torch.rand(H, W, generator=g)
    r = torch.randn(H, W, 9, generator=g)
    r[:, :, 0] = a
    r[:, :, 1] *= 3.0
    r[:, :, 2] *= 9.0
    r[:, :, 3] = 40 * torch.rand(H, W, generator=g)
    gt_depth = 40 * torch.rand(H, W, generator=g)
    u = torch.rand(H, W, generator=g)
    mask = {"drop30": u >= 0.3, "valid": torch.ones(H, W, dtype=torch.bool), "dropped": torch.zeros(H, W, dtype=torch.bool)}[mask_kind]
    return [x.to(DEV) for x in (r, gt_depth, b, mask)]


def _options(use_rayhit=False, zero=None):
    o = training.default_options()
    o.lambda_intensity_l2 = 0.2                                     # the reference's default is 0: give the term work
    o.use_rayhit = use_rayhit
    if zero is not None:
        setattr(o, zero, 0.0)
    return o


def _ulp32(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def _bound(yard, ref):
    return max(2.0 * yard, _ulp32(ref))


def _three_ways(r, gt_depth, gt_int, mask, opt):
    """[total, depth, intensity, drop, n] and d_rendered of: float64 torch (reference), float32 torch (yardstick), the fused operator."""
    res = []
    for fn, dt in ((losses.range_image_loss_torch, torch.float64), (losses.range_image_loss_torch, torch.float32), (losses.range_image_loss, torch.float32)):
        x = r.to(dt).detach().clone().requires_grad_(True)
        out = fn(x, gt_depth.to(dt), gt_int.to(dt), mask, opt)
        out[0].backward()
        res.append(([float(v.detach().double()) for v in out], x.grad.detach().double()))
    return res


def _check_case(tag, r, gt_depth, gt_int, mask, opt):
    (s64, g64), (s32, g32), (sf, gf) = _three_ways(r, gt_depth, gt_int, mask, opt)
    for k, name in enumerate(("total", "depth", "intensity", "raydrop")):
        yard, mine = abs(s32[k] - s64[k]), abs(sf[k] - s64[k])
        print(f"FUSEDLOSS|{tag}|{name}|ref {s64[k]:.9g}|yardstick {yard:.3e}|fused {mine:.3e}|bound {_bound(yard, s64[k]):.3e}")
    nrm = float(g64.norm())
    yard_g = float((g32 - g64).norm()) / nrm if nrm > 0 else 0.0
    mine_g = float((gf - g64).norm()) / nrm if nrm > 0 else float(gf.norm())
    print(f"FUSEDLOSS|{tag}|d_rendered|ref norm {nrm:.6g}|yardstick {yard_g:.3e}|fused {mine_g:.3e}|bound {max(2 * yard_g, 2.0 ** -23):.3e}")
    assert sf[4] == s64[4] == max(float(mask.sum()), 1.0)           # n is exact
    for k, name in enumerate(("total", "depth", "intensity", "raydrop")):
        assert abs(sf[k] - s64[k]) <= _bound(abs(s32[k] - s64[k]), s64[k]), (tag, name, sf[k], s32[k], s64[k])
    assert mine_g <= max(2 * yard_g, 2.0 ** -23), (tag, mine_g, yard_g)
    return sf, gf


@pytest.mark.parametrize("use_rayhit", [False, True])
@pytest.mark.parametrize("mask_kind", ["drop30", "valid", "dropped"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: s if isinstance(s, str) else f"{s[0]}x{s[1]}")
def test_terms_and_gradient_against_float64(size, mask_kind, use_rayhit):
    r, gt_depth, gt_int, mask = _inputs(size, mask_kind)
    opt = _options(use_rayhit)
    p = torch.sigmoid(r[:, :, 2]) if not use_rayhit else torch.softmax(r[:, :, 1:3], -1)[..., 1]
    if r.shape[0] * r.shape[1] >= 1024:
        assert int((p < 1e-7).sum()) > 0 and int((p > 1 - 1e-7).sum()) > 0        # the case has probabilities beyond the clamp on both sides
    sf, gf = _check_case(f"{size}/{mask_kind}/rayhit{int(use_rayhit)}", r, gt_depth, gt_int, mask, opt)
    assert float(gf[:, :, 4:].abs().max()) == 0.0
    if not use_rayhit:
        assert float(gf[:, :, 1].abs().max()) == 0.0
    else:
        assert torch.equal(gf[:, :, 1], -gf[:, :, 2])
    if mask_kind == "dropped":
        assert sf[4] == 1.0 and sf[1] == 0.0 and float(gf[:, :, 0].abs().max()) == 0.0 and float(gf[:, :, 3].abs().max()) == 0.0


@pytest.mark.parametrize("zero", WEIGHTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: s if isinstance(s, str) else f"{s[0]}x{s[1]}")
def test_each_weight_set_to_zero_in_turn(size, zero):
    r, gt_depth, gt_int, mask = _inputs(size, "drop30", seed=1)
    sf, gf = _check_case(f"{size}/drop30/{zero}=0", r, gt_depth, gt_int, mask, _options(False, zero))
    if zero == "lambda_depth_l1":
        assert sf[1] == 0.0 and float(gf[:, :, 3].abs().max()) == 0.0           # an exact zero, term and gradient
    if zero == "lambda_raydrop_bce":
        assert sf[3] == 0.0 and float(gf[:, :, 2].abs().max()) == 0.0


def test_all_weights_zero_is_an_exact_zero():
    r, gt_depth, gt_int, mask = _inputs((66, 1030), "drop30")
    opt = _options()
    for k in WEIGHTS:
        setattr(opt, k, 0.0)
    x = r.clone().requires_grad_(True)
    out = losses.range_image_loss(x, gt_depth, gt_int, mask, opt)
    out[0].backward()
    assert [float(v) for v in out[:4]] == [0.0, 0.0, 0.0, 0.0] and float(x.grad.abs().max()) == 0.0


def _raw_backward(r, gt_depth, gt_int, mask, opt, d_rendered, upstream=1.0):
    """Forward + backward through the C ABI into a buffer of the caller's."""
    lib = losses.load()
    H, W = r.shape[:2]
    nb = int(lib.lrt_loss_work_bytes(H, W))
    work = torch.empty((nb + 7) // 8, dtype=torch.float64, device=DEV)
    out = torch.empty(5, device=DEV)
    w = (C.c_double * 5)(*losses._weights(opt))
    m8 = mask.contiguous().view(torch.uint8)
    up = torch.full((1,), upstream, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    a = (0, H, W, r.data_ptr(), gt_depth.data_ptr(), gt_int.data_ptr(), m8.data_ptr(), w, int(opt.use_rayhit))
    assert lib.lrt_loss_forward(*a, out.data_ptr(), work.data_ptr(), nb, st) == 0, lib.lrt_loss_last_error()
    assert lib.lrt_loss_backward(*a, up.data_ptr(), d_rendered.data_ptr(), work.data_ptr(), nb, st) == 0, lib.lrt_loss_last_error()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("use_rayhit", [False, True])
@pytest.mark.parametrize("size", [(66, 1030), (5, 7), (64, 2650)])
def test_unused_channels_are_exact_zeros_in_a_buffer_full_of_nan(size, use_rayhit):
    r, gt_depth, gt_int, mask = _inputs(size, "drop30", seed=3)
    opt = _options(use_rayhit)
    H, W = r.shape[:2]
    guard = 64                                                      # floats on either side of the image: the kernel writes its H x W x 9 and nothing else
    buf = torch.full((H * W * 9 + 2 * guard,), float("nan"), device=DEV)
    d = buf[guard:guard + H * W * 9].view(H, W, 9)
    _raw_backward(r, gt_depth, gt_int, mask, opt, d, upstream=0.5)
    assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[-guard:]).all())
    assert not bool(torch.isnan(d).any())
    assert float(d[:, :, 4:].abs().max()) == 0.0 and (use_rayhit or float(d[:, :, 1].abs().max()) == 0.0)
    assert float(d[:, :, 0].abs().max()) > 0 and float(d[:, :, 2].abs().max()) > 0 and float(d[:, :, 3].abs().max()) > 0
    # the upstream scalar is read on the device: half of the gradient at upstream 1, to rounding
    x = r.clone().requires_grad_(True)
    losses.range_image_loss(x, gt_depth, gt_int, mask, opt)[0].backward()
    assert float((d.double() * 2 - x.grad.double()).norm()) <= 1e-6 * float(x.grad.double().norm())


def test_two_calls_return_identical_bits():
    r, gt_depth, gt_int, mask = _inputs((64, 2650), "drop30", seed=5)
    opt = _options(True)
    runs = []
    for _ in range(2):
        x = r.clone().requires_grad_(True)
        out = losses.range_image_loss(x, gt_depth, gt_int, mask, opt)
        out[0].backward()
        runs.append((torch.stack([v.detach() for v in out]).clone(), x.grad.clone()))
        losses._WORK.clear()                                         # the second call gets a fresh (uninitialised) workspace
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_interleaved_forwards_of_one_size_keep_their_own_backward():
    """The workspace is cached per image size: a second forward before the first one's backward must not leak into it."""
    opt = _options()
    ra, da, ia, ma = _inputs((66, 1030), "drop30", seed=6)
    rb, db, ib, mb = _inputs((66, 1030), "valid", seed=7)
    xa = ra.clone().requires_grad_(True)
    la = losses.range_image_loss(xa, da, ia, ma, opt)[0]
    xb = rb.clone().requires_grad_(True)
    lb = losses.range_image_loss(xb, db, ib, mb, opt)[0]
    la.backward(); lb.backward()
    xa2 = ra.clone().requires_grad_(True)
    losses.range_image_loss(xa2, da, ia, ma, opt)[0].backward()
    assert torch.equal(xa.grad, xa2.grad)


def test_a_call_on_a_side_stream_behind_a_busy_gpu_does_not_wait():
    r, gt_depth, gt_int, mask = _inputs((64, 2048), "drop30", seed=8)
    opt = _options()
    side = torch.cuda.Stream()

    def step():
        x = r.clone().requires_grad_(True)
        out = losses.range_image_loss(x, gt_depth, gt_int, mask, opt)
        out[0].backward()
        return out, x

    with torch.cuda.stream(side):
        for _ in range(3):                                           # loads the library, sizes the workspace, warms the allocator on this stream
            ref_out, ref_x = step()
        torch.cuda.synchronize()
        torch.cuda._sleep(1_000_000); torch.cuda.synchronize()
        t0 = time.perf_counter(); torch.cuda._sleep(20_000_000); torch.cuda.synchronize()
        rate = 20_000_000 / max(time.perf_counter() - t0, 1e-6)
        torch.cuda._sleep(int(0.4 * rate))                           # ONE long-running kernel in front of the step
        marker = torch.cuda.Event(); marker.record()
        t0 = time.perf_counter()
        out, x = step()
        host_s = time.perf_counter() - t0
        still_busy = not marker.query()
    assert still_busy, f"the GPU finished the dummy work before the step was enqueued ({host_s * 1e3:.1f} ms of host time)"
    assert host_s < 0.1, f"enqueueing forward + backward took {host_s * 1e3:.1f} ms of host time while the GPU was busy: something waited"
    torch.cuda.synchronize()
    assert torch.equal(x.grad, ref_x.grad) and all(torch.equal(a, b) for a, b in zip(out, ref_out))


# ---- inside the training loop -----------------------------------------------------------------------------------------------------------------

def _small_training_case():
    """The case of tests/test_training.py::test_short_optimisation_run_on_the_gpu."""
    sc = scenes.make_scene(8000, seed=21, radius_scale=0.25)
    o, d = scenes.kitti_rays(16, 256)
    t = lambda a: torch.as_tensor(a, device=DEV)

    def asset(noise):
        rr = np.random.default_rng(1)
        op = sc["opacities"]
        a = training.GaussianAsset.from_tensors(
            t(sc["means"] + noise * rr.normal(size=sc["means"].shape).astype(np.float32)), t(sc["shs"][:, :1]), t(sc["shs"][:, 1:]),
            t(np.log(sc["scales"])), t(sc["rotations"]), t(np.log(op / (1 - op)) - 3.0 * float(noise > 0)), extent=15.0)
        a.active_sh_degree = 3
        return a
    opt = training.default_options()
    opt.position_lr_init, opt.position_lr_final = 0.002, 0.0002
    bg = torch.tensor([0.0, 0.0, 1.0], device=DEV)
    frames = training.RangeFrames()
    truth = training.GaussianScene([asset(0.0)])
    from lidar_rt_amd.renderer import raytracing
    args = types.SimpleNamespace(dynamic=False, opt=opt, pipe=types.SimpleNamespace())
    with torch.no_grad():
        pk = raytracing(0, truth.gaussians_assets, (t(o), t(d), torch.zeros(3, device=DEV)), bg, args)
    mask = pk["raydrop"].squeeze(-1) < 0.6
    frames.add_frame(0, t(o), t(d), pk["depth"].squeeze(-1).detach(), pk["intensity"].squeeze(-1).detach(), mask)
    return asset, opt, bg, frames, args


def test_short_optimisation_run_with_the_fused_loss():
    asset, opt, bg, frames, _ = _small_training_case()
    opt.fused_loss = True
    scene = training.GaussianScene([asset(0.05)])
    scene.training_setup(opt)
    hist = [training.training_step(scene, frames, 0, it, opt, bg) for it in range(1, 61)]
    first, last = float(torch.stack([h["loss"] for h in hist[:5]]).mean()), float(torch.stack([h["loss"] for h in hist[-5:]]).mean())
    assert np.isfinite(last) and last < 0.7 * first, (first, last)
    for k in ("depth", "intensity", "raydrop"):
        assert np.isfinite(float(hist[-1][k])) and float(hist[-1][k]) > 0
    # the first step's numbers equal the unfused step's on the same start (the optimiser has not moved anything yet)
    opt2 = training.default_options(); opt2.position_lr_init, opt2.position_lr_final = opt.position_lr_init, opt.position_lr_final
    scene2 = training.GaussianScene([asset(0.05)])
    scene2.training_setup(opt2)
    h2 = training.training_step(scene2, frames, 0, 1, opt2, bg)
    for k in ("loss", "depth", "intensity", "raydrop"):
        assert abs(float(hist[0][k]) - float(h2[k])) <= 1e-4 * abs(float(h2[k])) + 1e-7, (k, float(hist[0][k]), float(h2[k]))


def test_first_step_means_gradient_agrees_with_the_unfused_step():
    """Tracer(deterministic=True) on all sides, so that only the loss differs: the gradient of the image from the float64 torch loss (reference), the
    float32 torch loss (the unfused step: yardstick) and the fused operator, each pushed through the same ordered tracer backward to means3D.grad."""
    from lidar_rt_amd import renderer
    asset, opt, bg, frames, args = _small_training_case()
    old = renderer.deterministic
    renderer.deterministic = True
    try:
        grads, images = {}, {}
        for kind in ("f64", "f32", "fused"):
            scene = training.GaussianScene([asset(0.05)])
            pkg = renderer.raytracing(0, scene.gaussians_assets, frames, bg, args, return_rendered=True)
            rendered = pkg["rendered"]
            gt = (frames.get_depth(0), frames.get_intensity(0), frames.get_mask(0))
            if kind == "fused":
                losses.range_image_loss(rendered, *gt, opt)[0].backward()
            elif kind == "f32":
                losses.range_image_loss_torch(rendered, *gt, opt)[0].backward()
            else:
                x = rendered.detach().double().requires_grad_(True)
                losses.range_image_loss_torch(x, gt[0].double(), gt[1].double(), gt[2], opt)[0].backward()
                rendered.backward(x.grad.float())
            torch.cuda.synchronize()
            grads[kind], images[kind] = pkg["means3D"].grad.double().clone(), rendered.detach().clone()
        assert torch.equal(images["f64"], images["f32"]) and torch.equal(images["f64"], images["fused"])      # the deterministic forward: one image
    finally:
        renderer.deterministic = old
    nrm = float(grads["f64"].norm())
    yard, mine = float((grads["f32"] - grads["f64"]).norm()) / nrm, float((grads["fused"] - grads["f64"]).norm()) / nrm
    print(f"FUSEDLOSS|training first step|means3D.grad|ref norm {nrm:.6g}|yardstick {yard:.3e}|fused {mine:.3e}|bound {max(2 * yard, 2.0 ** -23):.3e}")
    assert nrm > 0 and mine <= max(2 * yard, 2.0 ** -23), (mine, yard)


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=False)


def test_a_deterministic_fused_run_resumed_from_its_checkpoint_repeats_the_uninterrupted_run_bit_for_bit(tmp_path):
    """`train --deterministic --fused-loss`: the harness of tests/test_train_entry_gpu.py's deterministic case."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import make_sequence
    data = str(tmp_path / "seq")
    make_sequence.make("kitti360_dynamic", data, n_frames=4, scale=0.1)
    common = ["--data", data, "--log-every", "1", "--save-every", "12", "--max-points", "60000", "--deterministic", "--fused-loss",
              "--opt", "densify_from_iter=4", "--opt", "densification_interval=8"]
    run = lambda out, extra: subprocess.run([sys.executable, "-m", "lidar_rt_amd.train", "--out", out] + common + extra, cwd=REPO, capture_output=True,
                                            text=True, timeout=1500)
    a = run(str(tmp_path / "a"), ["--iters", "24"])
    assert a.returncode == 0, a.stdout[-2000:] + a.stderr[-3000:]
    b = run(str(tmp_path / "b"), ["--iters", "24", "--resume", str(tmp_path / "a" / "chkpnt12.pth")])
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-3000:]
    rows_a = [json.loads(l) for l in a.stdout.splitlines() if l.startswith("{")]
    rows_b = [json.loads(l) for l in b.stdout.splitlines() if l.startswith("{")]
    tail_a = [r for r in rows_a if r["iteration"] > 12]
    assert [r["iteration"] for r in rows_b] == [r["iteration"] for r in tail_a] and len(rows_b) == 12
    assert rows_a[-1]["loss"] < rows_a[0]["loss"]
    for ra, rb in zip(tail_a, rows_b):
        assert ra["frame"] == rb["frame"] and ra["points"] == rb["points"] and ra["loss"] == rb["loss"], (ra, rb)
        assert ra["depth"] == rb["depth"] and ra["intensity"] == rb["intensity"] and ra["raydrop"] == rb["raydrop"], (ra, rb)
    pa, pb = _load(tmp_path / "a" / "chkpnt24.pth")[0], _load(tmp_path / "b" / "chkpnt24.pth")[0]
    assert len(pa) == len(pb) == 9
    for ga, gb in zip(pa, pb):
        for i in (1, 2, 3, 4, 5, 6, 8, 9):
            assert torch.equal(ga[i].detach().cpu(), gb[i].detach().cpu()), i
        for k, st in ga[10]["state"].items():
            for n in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(gb[10]["state"][k][n].cpu(), st[n].cpu()), (k, n)


def test_two_ranks_with_the_fused_loss_stay_bit_identical(tmp_path):
    """Every rank holds the whole gathered frame and runs the same ordered kernels: `check_replicas` after every step (it raises otherwise)
    and the saved parameters of the two ranks are the same bits."""
    worker = os.path.join(HERE, "fused_loss_dist_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29647",
                        worker, str(tmp_path / "w2")], env=env, cwd=REPO, timeout=600, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    r0, r1 = np.load(str(tmp_path / "w2.rank0.npz")), np.load(str(tmp_path / "w2.rank1.npz"))
    assert r0["log"][:, 2:].sum() > 0, "the case must densify"
    assert np.all(np.isfinite(r0["log"][:, 0]))
    for k in ("log", "xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "m_xyz", "v_xyz"):
        np.testing.assert_array_equal(r0[k], r1[k])
