"""The grid Chamfer operator on the GPU: exactness against this package's chamfer_3DDist on the torch-formed points (distances and neighbour
indices bit for bit), the empty cloud, the gradients against float64 autograd of the PyTorch yardstick under the project's rule
(profiles/fused_loss.md: within max(2 x the existing float32 path's own distance from float64, 2^-23) in relative L2), outputs written
whole, repeatability, stream order, training through `training_step` and the deterministic resume of `python -m lidar_rt_amd.train`."""
import json
import os
import subprocess
import sys
import time
import types

import numpy as np
import pytest
import torch

from lidar_rt_amd import grid_chamfer as gc, scenes, training

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
DEV = torch.device("cuda:0")
EPS = 2.0 ** -23
SIZES = [(5, 7), (11, 200), (16, 64), (66, 1030)]
MASKS = ["all", "drop30", "one", "two"]
CLOUDS = ["coherent", "incoherent", "lattice"]


def _case(H, W, mask, cloud, seed=0):
    """(o, d, range_a, range_b, mask_a, mask_b) on the device, float32 / bool."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    o, d = scenes.kitti_rays(H, W, origin=(1.5, -2.0, 0.7))
    if (H, W) == (16, 64):                                                   # the recorded 16 x 64 images as ground-truth ranges
        G = np.load(os.path.join(HERE, "golden", "loop_golden.npz"))
        gt = (4.0 + 40.0 * np.abs(G["loss_img_b"][0])).astype(np.float32)
    else:
        gt = (6.0 + 30.0 * rng.uniform(size=(H, 1)) + 3.0 * np.sin(np.arange(W) / 9.0)[None, :] + rng.uniform(0, 0.5, (H, W))).astype(np.float32)
    if cloud == "coherent":
        ra, rb = (gt + rng.normal(0, 0.03, (H, W))).astype(np.float32), gt
    elif cloud == "incoherent":                                              # independent random ranges: the search degenerates towards brute force
        ra, rb = rng.uniform(1, 80, (H, W)).astype(np.float32), rng.uniform(1, 80, (H, W)).astype(np.float32)
    else:                                                                    # lattice: rays quantised to a coarse grid at constant range: distinct pixels, identical points
        d = np.round(d * 2) / 2
        d[np.abs(d).sum(-1) == 0] = (1.0, 0.0, 0.0)
        d = d.astype(np.float32); o = np.zeros_like(o)
        ra, rb = np.full((H, W), 4.0, np.float32), np.full((H, W), 4.0, np.float32)
    ma = np.ones((H, W), bool)
    mb = ma
    if mask == "drop30":
        ma = rng.uniform(size=(H, W)) >= 0.3; mb = ma
    elif mask == "one":
        ma = np.zeros((H, W), bool); ma[H // 2, W // 3] = True; mb = ma
    elif mask == "two":
        ma = rng.uniform(size=(H, W)) >= 0.3; mb = rng.uniform(size=(H, W)) >= 0.4
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=DEV)
    return t(o), t(d), t(ra), t(rb), t(ma), t(mb)


def _existing(o, d, ra, rb, ma, mb, mode=None):
    """This package's chamfer_3DDist on the torch-formed, index_selected points: (d1, d2, i1, i2, index list of A, of B)."""
    from lidar_rt_amd.chamfer3D import chamfer_3DDist, _C
    ia, ib = torch.nonzero(ma.reshape(-1)).squeeze(1), torch.nonzero(mb.reshape(-1)).squeeze(1)
    pa = (o + d * ra.reshape(*d.shape[:2], 1)).reshape(-1, 3).index_select(0, ia)
    pb = (o + d * rb.reshape(*d.shape[:2], 1)).reshape(-1, 3).index_select(0, ib)
    if mode is not None:
        _C.set_option("mode", mode, DEV)
    try:
        d1, d2, i1, i2 = chamfer_3DDist()(pa[None].contiguous(), pb[None].contiguous())
    finally:
        if mode is not None:
            _C.set_option("mode", 2, DEV)                                    # the state is per device: back to the default (auto)
    return d1[0], d2[0], i1[0], i2[0], ia, ib


@pytest.mark.parametrize("H,W", SIZES)
def test_distances_and_indices_equal_the_existing_operator_bit_for_bit(H, W):
    mode = None if (H, W) == SIZES[-1] else 0                                # brute force for the small shapes, the default (tree) for the largest
    ties = 0
    for mask in MASKS:
        for cloud in CLOUDS:
            o, d, ra, rb, ma, mb = _case(H, W, mask, cloud)
            d1, d2, i1, i2, ia, ib = _existing(o, d, ra, rb, ma, mb, mode)
            da, db, xa, xb = gc.grid_chamfer_nearest(o, d, ra, rb, ma, mb)
            tag = (H, W, mask, cloud)
            assert torch.equal(da.reshape(-1)[ia], d1) and torch.equal(db.reshape(-1)[ib], d2), tag
            assert torch.equal(xa.reshape(-1)[ia].long(), ib[i1.long()]), tag      # mask_index[idx of the existing op] == idx of this op
            assert torch.equal(xb.reshape(-1)[ib].long(), ia[i2.long()]), tag
            # invalid pixels: 0 and -1
            assert float(da[~ma].abs().sum()) == 0.0 and bool((xa[~ma] == -1).all()) and float(db[~mb].abs().sum()) == 0.0 and bool((xb[~mb] == -1).all()), tag
            # the scalars: float64 means of these very distances, one rounding.  Another float64 summation order moves the sum by ~n 2^-53, which
            # can move the rounded float32 by at most one unit in the last place (2^-23 relative)
            loss, m_a, m_b = gc.grid_chamfer(o, d, ra, rb, ma, mb, weight=0.3)
            w_a, w_b = float(d1.double().mean()), float(d2.double().mean())
            assert abs(float(m_a) - w_a) <= EPS * w_a and abs(float(m_b) - w_b) <= EPS * w_b, tag
            assert abs(float(loss) - 0.3 * 0.5 * (w_a + w_b)) <= EPS * 0.3 * 0.5 * (w_a + w_b), tag
            if cloud == "lattice" and mask != "one":
                pb = (o + d * rb[..., None]).reshape(-1, 3)[ib]
                ties += int(pb.shape[0] - torch.unique(pb, dim=0).shape[0])
    assert ties > 0                                                          # the lattice did produce distinct pixels with identical points


def test_an_empty_cloud_gives_exact_zeros_and_no_error():
    o, d, ra, rb, ma, _ = _case(11, 200, "drop30", "coherent")
    none = torch.zeros_like(ma)
    for m_a, m_b in ((none, none), (ma, none), (none, ma)):
        o_, d_, r_ = o.clone().requires_grad_(True), d.clone().requires_grad_(True), ra.clone().requires_grad_(True)
        loss, mean_a, mean_b = gc.grid_chamfer(o_, d_, r_, rb, m_a, m_b, weight=2.0)
        loss.backward()
        assert float(loss) == 0.0 and float(mean_a) == 0.0 and float(mean_b) == 0.0
        for g in (o_.grad, d_.grad, r_.grad):
            assert g is not None and float(g.abs().sum()) == 0.0 and not bool(torch.isnan(g).any())
        da, db, xa, xb = gc.grid_chamfer_nearest(o, d, ra, rb, m_a, m_b)
        assert float(da.abs().sum()) == 0.0 and float(db.abs().sum()) == 0.0 and bool((xa == -1).all()) and bool((xb == -1).all())


def _rel(x, ref):
    return float((x.double() - ref).norm() / ref.norm().clamp_min(1e-300))


GRAD_CASES = {"coherent_11x200": ((11, 200), "drop30", "coherent"), "incoherent_5x7": ((5, 7), "all", "incoherent"),
              "two_masks_11x200": ((11, 200), "two", "coherent"), "coherent_66x1030": ((66, 1030), "drop30", "coherent"),
              "collapsed_prediction_16x64": ((16, 64), "all", "collapsed_a"), "collapsed_ground_truth_16x64": ((16, 64), "drop30", "collapsed_b")}


def _grad_case(name):
    (H, W), mask, cloud = GRAD_CASES[name]
    o, d, ra, rb, ma, mb = _case(H, W, mask, "coherent" if cloud.startswith("collapsed") else cloud)
    if cloud == "collapsed_a":
        ra = torch.zeros_like(ra)                                            # every predicted point AT the sensor: one of them attracts every ground-truth point
    if cloud == "collapsed_b":
        rb = torch.zeros_like(rb)
    return o, d, ra, rb, ma, mb


def _three_gradients(o, d, ra, rb, ma, mb, weight):
    """(float64 autograd of the yardstick, the existing float32 path, the grid operator): each (d_range_a, d_rays_o, d_rays_d)."""
    from lidar_rt_amd.chamfer3D import chamfer_3DDist
    leaf = lambda x, dt: x.detach().to(dt).clone().requires_grad_(True)
    o64, d64, r64 = leaf(o, torch.float64), leaf(d, torch.float64), leaf(ra, torch.float64)
    gc.grid_chamfer_torch(o64, d64, r64, rb.double(), ma, mb, weight=weight)[0].backward()
    o32, d32, r32 = leaf(o, torch.float32), leaf(d, torch.float32), leaf(ra, torch.float32)
    ia, ib = torch.nonzero(ma.reshape(-1)).squeeze(1), torch.nonzero(mb.reshape(-1)).squeeze(1)
    pa = (o32 + d32 * r32.reshape(*d.shape[:2], 1)).reshape(-1, 3).index_select(0, ia)
    pb = (o32 + d32 * rb.reshape(*d.shape[:2], 1)).reshape(-1, 3).index_select(0, ib)
    d1, d2, _, _ = chamfer_3DDist()(pa[None].contiguous(), pb[None].contiguous())
    (weight * 0.5 * (d1.mean() + d2.mean())).backward()
    og, dg, rg = leaf(o, torch.float32), leaf(d, torch.float32), leaf(ra, torch.float32)
    gc.grid_chamfer(og, dg, rg, rb, ma, mb, weight=weight)[0].backward()
    return (r64.grad, o64.grad, d64.grad), (r32.grad, o32.grad, d32.grad), (rg.grad, og.grad, dg.grad)


@pytest.mark.parametrize("name", list(GRAD_CASES))
def test_gradients_against_float64_autograd_under_the_yardstick_rule(name):
    """Relative L2 against float64 autograd of grid_chamfer_torch; yardstick = torch points -> chamfer_3DDist -> autograd.  One
    GRIDCD|case:tensor|yardstick|grid line per tensor is printed before the assertion (run with -s); profiles/grid_chamfer.md is where they are
    recorded."""
    o, d, ra, rb, ma, mb = _grad_case(name)
    if name.startswith("collapsed"):
        xa, xb = gc.grid_chamfer_nearest(o, d, ra, rb, ma, mb)[2:]
        src = xb[mb] if name.startswith("collapsed_prediction") else xa[ma]
        assert int(torch.bincount(src.long()).max()) > 64                    # at least one inverse neighbour list is longer than a wave's worth
    ref, old, new = _three_gradients(o, d, ra, rb, ma, mb, 0.7)
    rows = []
    for what, r, y, f in zip(("d_range_a", "d_rays_o", "d_rays_d"), ref, old, new):
        rows.append((what, _rel(y, r), _rel(f, r)))
        print(f"GRIDCD|{name}:{what}|{rows[-1][1]:.3e}|{rows[-1][2]:.3e}")
    for what, yard, fused in rows:
        assert fused <= max(2.0 * yard, EPS), (name, what, yard, fused)
    assert float(new[0][~ma].abs().sum()) == 0.0


def test_backward_writes_every_element_and_repeats_bit_for_bit():
    o, d, ra, rb, ma, mb = _grad_case("collapsed_prediction_16x64")
    ra = ra.clone(); ra[:, 20:] = _case(16, 64, "all", "coherent")[2][:, 20:]    # long lists AND short ones
    lib = gc.load()
    H, W = ra.shape
    ma8, mb8 = ma.view(torch.uint8), mb.view(torch.uint8)
    outs = []
    for fill in (float("nan"), 0.0, float("nan"), 0.0, float("nan")):         # 5 forward + backward calls, NaN- and zero-prefilled buffers
        out, da, db, xa, xb = gc._launch_forward(o, d, ra, rb, ma8, mb8, 0.7)
        g = [torch.full((H, W), fill, device=DEV), torch.full((H, W, 3), fill, device=DEV), torch.full((H, W, 3), fill, device=DEV)]
        work = gc._workspace(H, W, DEV)
        dl = torch.ones(1, device=DEV)
        stream = torch.cuda.current_stream(DEV).cuda_stream
        rc = lib.lrt_gridcd_backward(0, H, W, o.data_ptr(), d.data_ptr(), ra.data_ptr(), ma8.data_ptr(), rb.data_ptr(), mb8.data_ptr(), 0.7, xa.data_ptr(),
                                     xb.data_ptr(), dl.data_ptr(), g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), work.data_ptr(), work.numel() * 8, stream)
        assert rc == 0, lib.lrt_gridcd_last_error()
        outs.append([out, da, db, xa, xb] + g)
    torch.cuda.synchronize()
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert not bool(torch.isnan(x.float()).any()) and torch.equal(x, y)
    assert float(outs[0][5].abs().sum()) > 0 and float(outs[0][6].abs().sum()) > 0


def test_the_call_is_stream_ordered_behind_a_busy_kernel_without_a_host_wait():
    from tests.test_stream_order_gpu import _busy
    o, d, ra, rb, ma, mb = _case(66, 1030, "drop30", "coherent")
    leaf = lambda x: x.clone().requires_grad_(True)

    def step():
        o_, d_, r_ = leaf(o), leaf(d), leaf(ra)
        loss = gc.grid_chamfer(o_, d_, r_, rb, ma, mb, weight=0.5)[0]
        loss.backward()
        return loss.detach(), r_.grad, o_.grad, d_.grad
    want = step()                                                             # sizes the workspace
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _busy(0.01); torch.cuda.synchronize()                                 # calibrates the spin kernel
        _busy(0.4)
        marker = torch.cuda.Event(); marker.record()
        t0 = time.perf_counter()
        got = step()
        host_s = time.perf_counter() - t0
        still_busy = not marker.query()
    assert still_busy, f"the GPU finished the dummy work before the call was enqueued ({host_s * 1e3:.1f} ms of host time)"
    assert host_s < 0.1, f"enqueueing forward + backward took {host_s * 1e3:.1f} ms of host time while the GPU was busy: something waited"
    side.synchronize()
    for x, y in zip(want, got):
        assert torch.equal(x, y)


# ---- training ---------------------------------------------------------------------------------------------------------------------------------

def _training_scene(opt):
    """The 16 x 256 scene of tests/test_training.py: targets rendered from a ground-truth scene, a perturbed copy to optimise."""
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
    bg = torch.tensor([0.0, 0.0, 1.0], device=DEV)
    frames = training.RangeFrames()
    truth = training.GaussianScene([asset(0.0)])
    from lidar_rt_amd.renderer import raytracing
    args = types.SimpleNamespace(dynamic=False, opt=opt, pipe=types.SimpleNamespace())
    with torch.no_grad():
        pk = raytracing(0, truth.gaussians_assets, (t(o), t(d), torch.zeros(3, device=DEV)), bg, args)
    mask = pk["raydrop"].squeeze(-1) < 0.6
    frames.add_frame(0, t(o), t(d), pk["depth"].squeeze(-1).detach(), pk["intensity"].squeeze(-1).detach(), mask)
    scene = training.GaussianScene([asset(0.05)])
    scene.training_setup(opt)
    return scene, frames, bg


def test_sixty_iterations_with_the_differentiable_grid_term_train_like_the_existing_operator():
    runs = {}
    for grid in (False, True):
        opt = training.default_options()
        opt.position_lr_init, opt.position_lr_final = 0.002, 0.0002
        opt.grid_chamfer = grid
        scene, frames, bg = _training_scene(opt)
        hist = [training.training_step(scene, frames, 0, it, opt, bg, chamfer_points_detached=False) for it in range(1, 61)]
        first, last = float(torch.stack([h["loss"] for h in hist[:5]]).mean()), float(torch.stack([h["loss"] for h in hist[-5:]]).mean())
        runs[grid] = (first, last, float(hist[0]["chamfer"]), float(hist[-1]["chamfer"]))
        assert np.isfinite(last) and last < 0.7 * first, (grid, first, last)   # the criterion of tests/test_training.py
    # the same first Chamfer value (the same neighbours; float64 means here, float32 means there, and the default tracer's forward carries
    # float-atomic noise of its own), and the same kind of drop
    assert abs(runs[True][2] - runs[False][2]) <= 1e-4 * abs(runs[False][2]), runs
    assert abs(runs[True][1] / runs[True][0] - runs[False][1] / runs[False][0]) < 0.15, runs


def test_first_step_means3d_gradient_with_the_switch_on_and_off_under_the_yardstick_rule(monkeypatch):
    """Only the Chamfer term is weighted, the tracer is deterministic: means3D.grad differs between the runs by the Chamfer gradient alone.  Third run:
    the grid switch on with the operator replaced by the float64 yardstick -- the reference both float32 gradients are measured against."""
    from lidar_rt_amd import renderer
    monkeypatch.setattr(renderer, "deterministic", True)
    monkeypatch.setattr(renderer, "tracer_2dgs", None)

    def first_grad(grid, f64=False):
        opt = training.default_options()
        for k in ("lambda_depth_l1", "lambda_intensity_l1", "lambda_intensity_l2", "lambda_intensity_dssim", "lambda_raydrop_bce", "lambda_reg"):
            setattr(opt, k, 0.0)
        opt.lambda_cd, opt.grid_chamfer = 1.0, grid
        scene, frames, bg = _training_scene(opt)
        seen = {}
        inner = scene.optimize
        scene.optimize = lambda o_, it, mean_grads, acc: (seen.__setitem__("g", mean_grads.detach().clone()), inner(o_, it, mean_grads, acc))[1]
        def torch64(o, d, ra, rb, m, weight=1.0):
            loss, a, b = gc.grid_chamfer_torch(o.double(), d.double(), ra.double(), rb.double(), m, weight=weight)
            return loss.float(), a, b
        with monkeypatch.context() as mp:
            if f64:
                mp.setattr(gc, "grid_chamfer", torch64)
            training.training_step(scene, frames, 0, 1, opt, bg, chamfer_points_detached=False)
        return seen["g"]
    off, on = first_grad(False), first_grad(True)
    ref = first_grad(True, f64=True).double()
    assert float(ref.abs().sum()) > 0
    yard, fused = _rel(off, ref), _rel(on, ref)
    print(f"GRIDCD|training_step:means3D.grad|{yard:.3e}|{fused:.3e}")
    assert fused <= max(2.0 * yard, EPS), (yard, fused)
    monkeypatch.setattr(renderer, "tracer_2dgs", None)                        # the next test builds its own tracer for its own flags


RESUME_CASES = {"grid_chamfer": [], "grid_chamfer_and_sensor_poses": ["--refine-poses"]}


@pytest.mark.parametrize("case", list(RESUME_CASES))
def test_a_deterministic_run_with_the_differentiable_grid_term_resumes_bit_for_bit(tmp_path, case):
    """The recipe of tests/test_train_entry_gpu.py with lambda_cd = 0.01, --grid-chamfer --chamfer-grad: the Chamfer gradient reaches the Gaussians
    (and with --refine-poses the sensor poses, through the rays): the case tests/test_actor_refine_gpu.py had to run with lambda_cd = 0."""
    from tests.test_train_entry_gpu import _load
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import make_sequence
    data = str(tmp_path / "seq")
    make_sequence.make("kitti360_dynamic", data, n_frames=4, scale=0.1)
    common = ["--data", data, "--log-every", "1", "--save-every", "6", "--max-points", "60000", "--deterministic", "--grid-chamfer", "--chamfer-grad",
              "--opt", "lambda_cd=0.01", "--opt", "densify_from_iter=2", "--opt", "densification_interval=4"] + RESUME_CASES[case]   # densifications at 4, 8, 12
    run = lambda out, extra: subprocess.run([sys.executable, "-m", "lidar_rt_amd.train", "--out", out] + common + extra, cwd=REPO, capture_output=True,
                                            text=True, timeout=900)
    a = run(str(tmp_path / "a"), ["--iters", "12"])
    assert a.returncode == 0, a.stdout[-2000:] + a.stderr[-3000:]
    b = run(str(tmp_path / "b"), ["--iters", "12", "--resume", str(tmp_path / "a" / "chkpnt6.pth")])
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-3000:]
    rows_a = [json.loads(l) for l in a.stdout.splitlines() if l.startswith("{")]
    rows_b = [json.loads(l) for l in b.stdout.splitlines() if l.startswith("{")]
    tail_a = [r for r in rows_a if r["iteration"] > 6]
    assert [r["iteration"] for r in rows_b] == [r["iteration"] for r in tail_a] and len(rows_b) == 6
    for ra, rb in zip(tail_a, rows_b):
        assert ra["frame"] == rb["frame"] and ra["points"] == rb["points"] and ra["loss"] == rb["loss"], (ra, rb)
    pa, pb = _load(tmp_path / "a" / "chkpnt12.pth")[0], _load(tmp_path / "b" / "chkpnt12.pth")[0]
    assert len(pa) == len(pb) == 9
    for ga, gb in zip(pa, pb):
        for i in (1, 2, 3, 4, 5, 6, 8, 9):
            assert torch.equal(ga[i].detach().cpu(), gb[i].detach().cpu()), i
        for k, st in ga[10]["state"].items():
            for n in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(gb[10]["state"][k][n].cpu(), st[n].cpu()), (k, n)
    if "--refine-poses" in common:
        sa, sb = _load(tmp_path / "a" / "poses12.pth"), _load(tmp_path / "b" / "poses12.pth")
        assert set(sa["xi"]) == set(sb["xi"]) and any(float(x.abs().sum()) > 0 for x in sa["xi"].values())
        for f in sa["xi"]:
            assert torch.equal(sa["xi"][f], sb["xi"][f]), f
