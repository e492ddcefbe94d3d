"""The fused evaluation metrics on the GPU: every figure of `metrics.frame_metrics` against the float64 twin `frame_metrics_reference` and
against today's float32 `evaluation` path, under these rules (profiles/fused_metrics.md records the measured figures):

* medae: the SAME BITS as the sort-based median of the same float32 errors;
* the ratios of exact counts (ray-drop rmse / acc / f1, fscore, n_pred, n_gt): within one float32 ulp (2^-23 relative) of the twin;
* chamfer_dist: the nearest distances carry chamfer_3DDist's bits (re-asserted on one case); within one ulp of the float64 mean of those bits;
* rmse, mae, ssim, psnr: the project's criterion of the fused loss: the operator's distance to the twin is at most twice
  the distance of today's float32 path to the same twin, with a floor of one float32 ulp;
* wherever the twin is NaN (the SSIM of a constant ground truth, the Chamfer distance of an empty cloud) the operator is NaN.

Then the output discipline (every element written, the same bits twice, no host wait, rows of a table) and `evaluate(..., fused=True)` against
`evaluate(..., fused=False)`.  A line FUSEDMETRICS|case:figure|yardstick distance|operator distance is printed per compared figure (run with -s)."""
import math
import time

import numpy as np
import pytest
import torch

from lidar_rt_amd import evaluation, grid_chamfer as gc, metrics as mt, scenes, training

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 2.0 ** -23
SHAPES = [(7, 7), (8, 9), (13, 70), (23, 200)]
MASKS = ["random70", "all_hit", "no_predicted_return", "no_ground_truth_return", "mostly_dropped"]
COUNTS = {"rmse", "acc", "f1", "fscore", "n_pred", "n_gt"}


def make_case(H, W, mask, seed=0, special=None):
    """A seeded smooth range image plus noise on a `RangeFrames.range_rays` grid: (pred, gt_depth, gt_intensity, gt_mask, rays), float32 / bool on
    the device.  pred[2][H // 2, W // 2] is exactly 0.625: the ratio of the strict-`<` cases."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    pose = torch.as_tensor(scenes.pose_matrix((0.3, -0.2, 1.7), yaw=0.1), dtype=torch.float32, device=DEV)
    rays = training.RangeFrames.range_rays(H, W, (math.radians(-24.9), math.radians(2.0)), pose, "KITTI")
    yy, xx = np.mgrid[0:H, 0:W]
    gd = (20.0 + 12.0 * np.sin(xx / 9.0) + 1.5 * np.cos(yy / 3.0) + rng.uniform(0, 0.5, (H, W))).astype(np.float32)
    gd[rng.uniform(size=(H, W)) < 0.03] = 95.0                        # beyond max_depth: the upper clamp
    pd = (gd + rng.normal(0, 0.05, (H, W))).astype(np.float32)
    gi = rng.uniform(-0.1, 1.1, (H, W)).astype(np.float32)
    pi = (gi + rng.normal(0, 0.05, (H, W))).astype(np.float32)
    pr = rng.uniform(0, 1, (H, W)).astype(np.float32)
    gm = rng.uniform(size=(H, W)) < 0.7
    if mask == "all_hit":
        gm[:] = True; pr[:] = np.minimum(pr, np.float32(0.3))
    elif mask == "no_predicted_return":
        pr[:] = np.maximum(pr, np.float32(0.7))
    elif mask == "no_ground_truth_return":
        gm[:] = False
    elif mask == "mostly_dropped":                                    # 65 % dropped on both sides, ground truth 0 there: one tie group at error 0
        gm = rng.uniform(size=(H, W)) < 0.35
        pr = np.where(gm, np.float32(0.1), np.float32(0.9)).astype(np.float32)
        gd = gd * gm; gi = np.clip(gi, 0, 1) * gm
    pr[H // 2, W // 2] = np.float32(0.625)
    if special == "constant_gt":
        gd[:] = 7.0
    elif special == "middle_pair_apart":                              # half the errors ~0.01, half ~5: the middle pair differs in the top 11 bits
        gm[:] = True; pr[:] = np.float32(0.1)
        e = np.where(rng.permutation(H * W).reshape(H, W) < H * W // 2, rng.uniform(0.01, 0.02, (H, W)), rng.uniform(4, 6, (H, W)))
        gd = np.clip(gd, 0, 70).astype(np.float32); pd = (gd - e).astype(np.float32)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    return (t(pd), t(pi), t(pr)), t(gd.astype(np.float32)), t(gi.astype(np.float32)), t(gm), rays


def existing_row(pred, gd, gi, gm, rays, use_gt_mask, ratio, max_depth=80.0, points=True):
    """Today's float32 path: the lines of evaluation.evaluate on the same tensors, in the order of metrics.ROW[:15]."""
    pd, pi, pr = pred
    gt_hit = gm.bool(); pred_hit = pr < ratio
    mask = gt_hit if use_gt_mask else pred_hit
    mk = mask.to(pd.dtype)
    d = evaluation.depth_metrics(gd, pd * mk, max_depth=max_depth)
    i = evaluation.intensity_metrics(gi.clamp(0, 1), pi.clamp(0, 1.0) * mk)
    r = evaluation.raydrop_metrics(1 - gt_hit.float(), 1 - pred_hit.float())
    row = [d[k] for k in ("rmse", "mae", "medae", "ssim", "psnr")] + [i[k] for k in ("rmse", "mae", "medae", "ssim", "psnr")] + [r[k] for k in ("rmse", "acc", "f1")]
    if points:
        o, dd = rays
        pts = lambda rng_, m: (o + dd * rng_[..., None]).reshape(-1, 3)[m.reshape(-1)]
        p = evaluation.points_metrics(pts(gd, gt_hit), pts(pd, mask))
        row += [p["chamfer_dist"], p["fscore"]]
    return [float(v) for v in row]


def check_row(tag, got, twin, old, chamfer64=None):
    """The rules of this file's docstring on one row; `got` float32 values, `twin` float64, `old` today's path (None entries: not compared);
    `chamfer64`: the float64 mean of the operators' own distances.  Returns the printed lines."""
    lines = []
    for k, (g, m) in enumerate(mt.ROW):
        x, t = got[k], twin[k]
        what = f"{tag}:{g}.{m}"
        if t != t:
            assert x != x, (what, x)
            continue
        assert x == x, (what, x, t)
        if m == "medae":
            assert np.float32(x).tobytes() == np.float32(t).tobytes(), (what, x, t)
            if old is not None:
                assert np.float32(x).tobytes() == np.float32(old[k]).tobytes(), (what, x, old[k])
        elif m in COUNTS and not (g in ("depth", "intensity")):
            assert abs(x - t) <= EPS * abs(t), (what, x, t)
        elif m == "chamfer_dist":
            ref = t if chamfer64 is None else chamfer64
            assert abs(x - ref) <= EPS * abs(ref), (what, x, ref)
        else:
            assert old is not None and old[k] == old[k], (what, "the float32 path itself is not finite here")
            yard, dist = abs(old[k] - t), abs(x - t)
            lines.append(f"FUSEDMETRICS|{what}|{yard:.3e}|{dist:.3e}")
            print(lines[-1])
            assert dist <= max(2.0 * yard, EPS * abs(t)), (what, x, t, old[k])
    return lines


def run_case(H, W, mask, use_gt, ratio, special=None, points=True):
    pred, gd, gi, gm, rays = make_case(H, W, mask, special=special)
    out = torch.full((mt.N,), float("nan"), device=DEV)
    mt.frame_metrics(pred, gd, gi, gm, rays if points else None, raydrop_ratio=ratio, use_gt_mask=use_gt, out=out)
    twin = mt.frame_metrics_reference(pred, gd, gi, gm, rays if points else None, raydrop_ratio=ratio, use_gt_mask=use_gt)
    old = existing_row(pred, gd, gi, gm, rays, use_gt, ratio, points=points)
    got = out.tolist()
    assert not any(v != v for v, t in zip(got, twin.tolist()) if t == t)              # the NaN prefill is gone wherever a figure exists
    return got, twin.tolist(), old + [None] * (mt.N - len(old)), (pred, gd, gi, gm, rays)


@pytest.mark.parametrize("H,W", SHAPES)
def test_every_figure_against_the_twin_and_the_float32_path(H, W):
    n_empty = 0
    for mask in MASKS:
        for use_gt in (False, True):
            for ratio in (0.4, 0.625):
                got, twin, old, case = run_case(H, W, mask, use_gt, ratio)
                pred, gd, gi, gm, rays = case
                tag = f"{H}x{W}/{mask}/{'gt' if use_gt else 'pred'}_mask/{ratio}"
                hit_b = gm if use_gt else (pred[2] < ratio)
                assert float(pred[2][H // 2, W // 2]) == 0.625                         # at ratio 0.625 this pixel is a drop only under the strict `<`
                chamfer64 = None
                if twin[13] == twin[13]:
                    da, db = gc.grid_chamfer_nearest(rays[0], rays[1], gd, pred[0], gm, hit_b)[:2]
                    chamfer64 = float(da.double().sum() / gm.sum() + db.double().sum() / hit_b.sum())
                else:
                    n_empty += 1
                    assert got[14] == 0.0 and twin[14] == 0.0
                check_row(tag, got, twin, old, chamfer64)
                if mask == "mostly_dropped":
                    assert got[2] == 0.0 and got[7] == 0.0 and twin[2] == 0.0        # more than half the errors are exactly 0
    assert n_empty >= 4                                                                # both kinds of empty cloud were met


def test_the_two_middle_errors_in_different_level_one_bins_and_a_constant_ground_truth():
    got, twin, old, case = run_case(8, 9, "all_hit", False, 0.4, special="middle_pair_apart")
    pred, gd = case[0], case[1]
    v = (gd.clamp(1e-6, 80.0) - pred[0].clamp(1e-6, 80.0)).abs().flatten().sort().values
    lo, hi = v[35:37].cpu().numpy().view(np.uint32)
    assert (lo >> 20) != (hi >> 20)                                                   # the ranks part at level 1
    check_row("8x9/middle_pair_apart", got, twin, old)
    assert np.float32(got[2]) == np.float32(0.5) * (v[35].cpu().numpy() + v[36].cpu().numpy())
    # a constant ground truth: the float64 yardstick's SSIM is NaN (R = 0), and so is the operator's; everything else is compared as usual
    got, twin, old, _ = run_case(13, 70, "random70", False, 0.4, special="constant_gt")
    assert twin[3] != twin[3] and got[3] != got[3] and got[8] == got[8]
    check_row("13x70/constant_gt", got, twin, old)


def test_the_nearest_distances_carry_the_bits_of_the_existing_operator():
    from lidar_rt_amd.chamfer3D import chamfer_3DDist
    pred, gd, gi, gm, rays = make_case(23, 200, "random70")
    hit_b = pred[2] < 0.4
    o, d = rays
    pa = (o + d * gd[..., None]).reshape(-1, 3)[gm.reshape(-1)]
    pb = (o + d * pred[0][..., None]).reshape(-1, 3)[hit_b.reshape(-1)]
    d1, d2, _, _ = chamfer_3DDist()(pa[None].contiguous(), pb[None].contiguous())
    da, db = gc.grid_chamfer_nearest(o, d, gd, pred[0], gm, hit_b)[:2]
    assert torch.equal(da[gm], d1[0]) and torch.equal(db[hit_b], d2[0])
    row = mt.frame_metrics(pred, gd, gi, gm, rays).tolist()
    want = float(d1.double().mean() + d2.double().mean())
    assert abs(row[13] - want) <= EPS * want
    thr = torch.tensor(0.05, dtype=torch.float32, device=DEV)
    p1, p2 = float((d1 < thr).double().mean()), float((d2 < thr).double().mean())
    assert abs(row[14] - 2 * p1 * p2 / (p1 + p2)) <= EPS * row[14] and row[15] == pb.shape[0] and row[16] == pa.shape[0]
    # the twin's brute force finds the same distances
    twin = mt.frame_metrics_reference(pred, gd, gi, gm, rays).tolist()
    assert abs(twin[13] - want) <= 1e-9 * want and abs(twin[14] - 2 * p1 * p2 / (p1 + p2)) <= 1e-12


def test_the_full_size_image_once():
    H, W = 64, 2048
    pred, gd, gi, gm, rays = make_case(H, W, "random70")
    out = torch.full((mt.N,), float("nan"), device=DEV)
    mt.frame_metrics(pred, gd, gi, gm, rays, out=out)
    got = out.tolist()
    twin = mt.frame_metrics_reference(pred, gd, gi, gm, None).tolist()                # the brute-force neighbours are left to the smaller shapes
    old = existing_row(pred, gd, gi, gm, rays, False, 0.4)
    hit_b = pred[2] < 0.4
    from lidar_rt_amd.chamfer3D import chamfer_3DDist
    o, d = rays
    pa = (o + d * gd[..., None]).reshape(-1, 3)[gm.reshape(-1)]
    pb = (o + d * pred[0][..., None]).reshape(-1, 3)[hit_b.reshape(-1)]
    d1, d2, _, _ = chamfer_3DDist()(pa[None].contiguous(), pb[None].contiguous())
    thr = torch.tensor(0.05, dtype=torch.float32, device=DEV)
    p1, p2 = float((d1 < thr).double().mean()), float((d2 < thr).double().mean())
    twin[13], twin[14] = float(d1.double().mean() + d2.double().mean()), 2 * p1 * p2 / (p1 + p2)
    check_row("64x2048/random70", got, twin, old + [None, None])


# ---- output discipline ------------------------------------------------------------------------------------------------------------------------------

def bits(t):
    return t.contiguous().view(torch.int32)


def test_rows_of_a_table_are_written_whole_and_repeat_bit_for_bit():
    cases = [make_case(13, 70, m) for m in ("random70", "no_predicted_return", "mostly_dropped")]
    table = torch.full((3, mt.N), float("nan"), device=DEV)
    for i, (pred, gd, gi, gm, rays) in enumerate(cases):
        mt.frame_metrics(pred, gd, gi, gm, rays, out=table[i])
    again = torch.zeros((3, mt.N), device=DEV)
    for i in (2, 0, 1):                                                                 # another order, another prefill
        pred, gd, gi, gm, rays = cases[i]
        mt.frame_metrics(pred, gd, gi, gm, rays, out=again[i])
    assert torch.equal(bits(table), bits(again))
    single = [mt.frame_metrics(*c) for c in cases]
    for i in range(3):
        assert torch.equal(bits(table[i]), bits(single[i]))
    nan = torch.isnan(table)
    assert not bool(nan[0].any()) and nan[1].nonzero().flatten().tolist() == [13] and not bool(nan[2].any())   # only the empty cloud's Chamfer distance
    # without rays: the two points figures are NaN, the sizes of the clouds still written
    pred, gd, gi, gm, rays = cases[0]
    row = mt.frame_metrics(pred, gd, gi, gm, None, out=torch.full((mt.N,), 5.0, device=DEV))
    assert torch.isnan(row[13:15]).all() and torch.equal(bits(row[:13]), bits(table[0, :13])) and torch.equal(bits(row[15:]), bits(table[0, 15:]))


def test_a_call_behind_a_busy_stream_returns_without_waiting():
    pred, gd, gi, gm, rays = make_case(64, 2048, "random70")
    want = mt.frame_metrics(pred, gd, gi, gm, rays).clone()                           # sizes the workspaces
    torch.cuda.synchronize()
    torch.cuda._sleep(1_000_000); torch.cuda.synchronize()
    t0 = time.perf_counter(); torch.cuda._sleep(20_000_000); torch.cuda.synchronize(); rate = 20_000_000 / (time.perf_counter() - t0)
    torch.cuda._sleep(int(0.3 * rate))
    marker = torch.cuda.Event(); marker.record()
    t0 = time.perf_counter()
    table = torch.empty((4, mt.N), device=DEV)
    for i in range(4):
        mt.frame_metrics(pred, gd, gi, gm, rays, out=table[i])
    host = time.perf_counter() - t0
    assert not marker.query() and host < 0.1, f"{host * 1e3:.1f} ms to enqueue 4 frames behind a busy GPU"
    torch.cuda.synchronize()
    for i in range(4):
        assert torch.equal(bits(table[i]), bits(want))


# ---- evaluate ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_scene():
    """The small scene of tests/test_evaluation.py, built here: 40,000 Gaussians, three 32 x 256 frames, rendered once."""
    from lidar_rt_amd import renderer
    sc = scenes.make_scene(40_000, seed=3, radius_scale=0.4)
    t = lambda a: torch.as_tensor(a, device=DEV)
    asset = training.GaussianAsset.from_tensors(t(sc["means"]), t(sc["shs"][:, :1]).contiguous(), t(sc["shs"][:, 1:]).contiguous(),
                                                torch.log(t(sc["scales"])), t(sc["rotations"]), training.inverse_sigmoid(t(sc["opacities"])),
                                                max_sh_degree=3, extent=30.0)
    asset.active_sh_degree = 3
    bg = torch.tensor(scenes.BG_DEFAULT, device=DEV)
    renderer.tracer_2dgs = None
    H, W = 32, 256
    rays = {}
    blank = training.RangeFrames()
    for f in range(3):
        o, d = scenes.range_rays(H, W, (np.radians(-24.9), np.radians(2.0)), scenes.pose_matrix((0.2 * f, 0.0, 0.0), yaw=0.02 * f), "KITTI")
        rays[f] = (t(o), t(d))
        blank.add_frame(f, rays[f][0], rays[f][1], torch.zeros(H, W, device=DEV), torch.zeros(H, W, device=DEV), torch.ones(H, W, device=DEV))
    renders = evaluation.render_frames([asset], blank, range(3), bg)
    thr = float(torch.cat([renders[f]["raydrop"].flatten() for f in range(3)]).median())
    yield asset, bg, rays, renders, thr
    renderer.tracer_2dgs = None


def test_evaluate_fused_against_evaluate(small_scene, monkeypatch):
    asset, bg, rays, renders, thr = small_scene
    H, W = renders[0]["depth"].shape[:2]
    rng = np.random.default_rng(9)
    frames = training.RangeFrames()
    for f in range(3):                                                                  # a ground truth NEAR the rendering: noise, its own mask
        hit = torch.as_tensor(rng.uniform(size=(H, W)) < 0.8, device=DEV) & (renders[f]["raydrop"].squeeze(-1) < min(0.95, 2 * thr))
        noise = torch.as_tensor(rng.normal(0, 0.05, (H, W)).astype(np.float32), device=DEV)
        frames.add_frame(f, rays[f][0], rays[f][1], (renders[f]["depth"].squeeze(-1) + noise).clamp_min(0) * hit,
                         (renders[f]["intensity"].squeeze(-1) + 0.1 * noise).clamp(0, 1) * hit, hit)
    monkeypatch.setattr(evaluation, "render_frames", lambda *a, **k: renders)         # both runs see the same rendering: the metrics are what is compared
    for use_gt in (False, True):
        old = evaluation.evaluate([asset], frames, [0, 1, 2], bg, raydrop_ratio=thr, use_gt_mask=use_gt)
        new = evaluation.evaluate([asset], frames, [0, 1, 2], bg, raydrop_ratio=thr, use_gt_mask=use_gt, fused=True)
        assert list(new) == list(old) == ["frames", "mean"] and list(new["frames"]) == list(old["frames"]) == [0, 1, 2]
        assert {g: list(v) for g, v in new["mean"].items()} == {g: list(v) for g, v in old["mean"].items()}
        for f in range(3):
            assert {g: list(v) for g, v in new["frames"][f].items()} == {g: list(v) for g, v in old["frames"][f].items()}
            twin = mt.frame_metrics_reference(renders[f], frames.get_depth(f), frames.get_intensity(f), frames.get_mask(f), rays[f],
                                              raydrop_ratio=thr, use_gt_mask=use_gt).tolist()
            names = [gm for gm in mt.ROW if gm not in mt.EXTRAS]
            got = [new["frames"][f][g][m] for g, m in names] + twin[15:]
            was = [old["frames"][f][g][m] for g, m in names] + [None, None]
            assert all(v == v for v in was[:15])
            check_row(f"evaluate/frame{f}/{'gt' if use_gt else 'pred'}_mask", got, twin, was)
        for g in new["mean"]:
            for m in new["mean"][g]:
                xs = [new["frames"][f][g][m] for f in range(3)]
                assert new["mean"][g][m] == sum(xs) / 3                                 # the host's mean, formed as evaluate forms it
    assert evaluation.evaluate([asset], frames, [], bg, fused=True) == evaluation.evaluate([asset], frames, [], bg)


def test_a_scene_evaluated_against_its_own_rendering(small_scene, monkeypatch):
    asset, bg, rays, renders, thr = small_scene
    frames = training.RangeFrames()
    for f in range(3):
        hit = renders[f]["raydrop"].squeeze(-1) < thr
        frames.add_frame(f, rays[f][0], rays[f][1], renders[f]["depth"].squeeze(-1) * hit, renders[f]["intensity"].squeeze(-1).clamp(0, 1) * hit, hit)
    monkeypatch.setattr(evaluation, "render_frames", lambda *a, **k: renders)
    res = evaluation.evaluate([asset], frames, [0, 1, 2], bg, raydrop_ratio=thr, fused=True)
    for f in range(3):
        r = res["frames"][f]
        for g in ("depth", "intensity"):
            assert r[g]["rmse"] == 0.0 and r[g]["mae"] == 0.0 and r[g]["medae"] == 0.0 and abs(r[g]["ssim"] - 1.0) <= EPS, (f, g, r[g])
        assert r["raydrop"] == {"rmse": 0.0, "acc": 1.0, "f1": 1.0} and r["points"] == {"chamfer_dist": 0.0, "fscore": 1.0}, (f, r)
    assert res["mean"]["points"]["fscore"] == 1.0 and res["mean"]["depth"]["rmse"] == 0.0
