"""The fused evaluation metrics without a GPU: the fifth product library (`liblrt_metrics.so`: a source list and hash of its own that moves no
other hash, exports, resource gate, argument errors before the device is touched), the `fused` switch of `evaluation.evaluate` and its flag,
the float64 twin `metrics.frame_metrics_reference` against the existing `evaluation` functions and a numpy restatement of skimage's SSIM, and
the arithmetic header `lrt_metrics_math.h` compiled for the host: window statistics against float64 numpy, the rank selection against a sort."""
import ctypes as C
import hashlib
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from lidar_rt_amd import build as lrt_build, evaluation, metrics as mt, resources

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
EPS = 2.0 ** -23


# ---- build ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def metrics_lib():
    return lrt_build.build_metrics()


def test_the_library_has_a_source_list_of_its_own_and_moves_no_other_hash():
    assert lrt_build.METRICS_SOURCES == ["lrt_metrics.hip"] and "lrt_metrics_math.h" in lrt_build.METRICS_HEADERS
    others = (lrt_build.SOURCES + lrt_build.HEADERS + lrt_build.LOSS_SOURCES + lrt_build.LOSS_HEADERS + lrt_build.GRIDCD_SOURCES + lrt_build.GRIDCD_HEADERS
              + lrt_build.INIT_SOURCES + lrt_build.INIT_HEADERS)
    assert not any("lrt_metrics" in f for f in others)
    # the other libraries' hashes at the commit this library was added on: committed profiles are keyed by them
    assert lrt_build.source_hash() == "2c98b54882a7ff74"          # moved twice since: the non-finite-input fixes in lrt_chamfer.hip; a comment of include/lrt.h (lrt_xchg_apply, zero_only on an overflowed block)
    assert lrt_build.loss_source_hash() == "cc56b0c83f72d5ca"
    assert lrt_build.gridcd_source_hash() == "fd279d9f7ff67722"
    assert lrt_build.init_source_hash() == "0fd7105f5d08ab22"
    # the torch extension's hash also covers the installed torch version: what is pinned is the part the repository decides
    h = hashlib.sha256()
    for f in (lrt_build.EXT_SRC, os.path.join(REPO, "include", "lrt.h")):
        h.update(open(f, "rb").read())
    # (moved twice since: include/lrt.h documents selector 10 of lrt_debug_read, then what lrt_xchg_apply(zero_only) does to an overflowed block -- comments, no declaration changed)
    assert h.hexdigest()[:16] == "e07ee6ee3a64b52c"
    assert "lrt_metrics" not in open(lrt_build.EXT_SRC).read()
    assert lrt_build.metrics_source_hash() not in (lrt_build.source_hash(), lrt_build.loss_source_hash(), lrt_build.gridcd_source_hash(), lrt_build.init_source_hash())
    assert os.path.basename(lrt_build.METRICS_LIB) == "liblrt_metrics.so"
    assert lrt_build.METRICS_LIB not in (lrt_build.LIB, lrt_build.LOSS_LIB, lrt_build.GRIDCD_LIB, lrt_build.INIT_LIB)
    assert "build_metrics(force, verbose)" in open(lrt_build.__file__).read()          # _build_product builds it


def test_the_library_builds_and_exports_what_its_header_declares(metrics_lib):
    assert os.path.exists(metrics_lib) and not lrt_build.metrics_is_stale()
    assert open(lrt_build.METRICS_STAMP).read().strip() == lrt_build.metrics_source_hash()
    hdr = open(os.path.join(REPO, "include", "lrt_metrics.h")).read()
    declared = set(re.findall(r"\b(lrt_metrics_[a-z_]+)\s*\(", hdr))
    assert declared == set(mt.EXPORTS), declared ^ set(mt.EXPORTS)
    lib = mt.load()
    for n in declared:
        assert hasattr(lib, n), n
    exported = set(re.findall(r"\blrt_metrics_[a-z_]+\b", subprocess.run(["nm", "-D", "--defined-only", metrics_lib], capture_output=True, text=True, check=True).stdout))
    assert exported == declared, exported ^ declared
    assert lib.lrt_metrics_abi_version() == int(re.search(r"#define\s+LRT_METRICS_ABI_VERSION\s+(\d+)", hdr).group(1)) == mt.ABI_VERSION
    # the row: the header's indices are metrics.ROW
    idx = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+LRT_METRICS_([A-Z_0-9]+)\s+(\d+)\s*$", hdr, re.M)}
    assert idx.pop("N") == mt.N == len(mt.ROW) and idx.pop("ABI_VERSION") == 1
    assert {f"{g}_{m}".upper(): i for i, (g, m) in enumerate(mt.ROW)} == idx


def test_every_kernel_passes_the_resource_gate(metrics_lib):
    res = resources.kernel_resources(metrics_lib)
    own = sorted(n for n in res if resources.is_own_kernel(n))
    assert len(own) >= 8 and all(n.startswith("k_mt_") for n in own), own
    assert all(any(re.search(g_, n) for g_ in resources.GATED) for n in own)
    assert resources.violations(res) == []
    for n in own:
        assert res[n]["vgpr_spill"] == 0 and res[n]["scratch_bytes"] == 0 and not res[n]["dynamic_stack"], (n, res[n])
    resources.check(metrics_lib)


def test_work_bytes_and_argument_errors_without_a_device(metrics_lib):
    lib = mt.load()
    wb = lib.lrt_metrics_work_bytes
    assert wb(6, 100) == 0 and wb(100, 6) == 0 and wb(0, 0) == 0 and wb(1 << 14, 1 << 14) == 0
    assert wb(7, 7) > 0 and wb(7, 7) % 16 == 0
    nb = wb(64, 2048)
    assert nb >= 2 * 64 * 2048 * 4 + (2 * 2048 + 4 * 2048 + 4 * 512) * 4 and nb % 16 == 0       # the keys of both images and the histograms
    buf = (C.c_char * 4096)()
    p = C.c_void_p((C.addressof(buf) + 15) // 16 * 16)
    big = 1 << 40                                                    # a work_bytes that passes the size check: nothing is touched before the device check
    frame = lambda H, W, ptrs, out, work, wbytes: lib.lrt_metrics_frame(1 << 20, H, W, *ptrs, 0.4, 0, 80.0, 0.05, out, work, wbytes, None)
    img = [p, p, p, p, p, p]
    err = lambda: lib.lrt_metrics_last_error()
    assert frame(6, 64, img + [p, p], p, p, big) < 0 and b"image size 6 x 64" in err()
    assert frame(64, 6, img + [p, p], p, p, big) < 0 and b"image size 64 x 6" in err()
    for i in range(6):
        bad = list(img); bad[i] = None
        assert frame(8, 9, bad + [p, p], p, p, big) < 0 and b"null image / mask pointer" in err()
    assert frame(8, 9, img + [p, None], p, p, big) < 0 and b"both or neither" in err()
    assert frame(8, 9, img + [None, None], None, p, big) < 0 and b"null output pointer" in err()
    assert frame(8, 9, img + [None, None], p, None, big) < 0 and b"workspace" in err()
    assert frame(8, 9, img + [None, None], p, p, wb(8, 9) - 1) < 0 and b"workspace of" in err() and str(wb(8, 9)).encode() in err()
    assert frame(8, 9, img + [None, None], p, C.c_void_p(p.value + 4), big) < 0 and b"16-byte aligned" in err()
    assert lib.lrt_metrics_frame(0, 8, 9, *img, None, None, float("nan"), 0, 80.0, 0.05, p, p, big, None) < 0 and b"NaN" in err()
    # every argument in order: only now the device is looked for
    assert frame(8, 9, img + [None, None], p, p, big) < 0 and b"no HIP device" in err()


def test_python_entry_refuses_cpu_tensors_and_wrong_shapes():
    z = torch.zeros(8, 9)
    with pytest.raises(mt.MetricsError, match="float32 HIP tensor"):
        mt.frame_metrics((z, z, z), z, z, z)
    with pytest.raises(mt.MetricsError, match="SSIM window"):
        mt.frame_metrics_reference((z[:6], z[:6], z[:6]), z[:6], z[:6], z[:6])
    with pytest.raises(mt.MetricsError, match=r"pred depth must be a \(8, 9\)"):
        mt.frame_metrics_reference((z[:, :8], z, z), z, z, z)


# ---- the switch ---------------------------------------------------------------------------------------------------------------------------------------

def test_evaluate_has_the_switch_off_by_default_and_the_command_line_its_flag():
    sig = inspect.signature(evaluation.evaluate)
    assert sig.parameters["fused"].default is False and list(sig.parameters)[-1] == "fused"
    r = subprocess.run([sys.executable, "-m", "lidar_rt_amd.evaluate", "--help"], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "--fused-metrics" in r.stdout
    from lidar_rt_amd import evaluate as cli
    assert "fused=bool(args.fused_metrics)" in open(cli.__file__).read()


# ---- the twin -------------------------------------------------------------------------------------------------------------------------------------------

SHAPES = [(7, 7), (8, 9), (13, 70)]
MASKS = ["random70", "all_hit", "all_dropped"]


def make_case(H, W, mask, seed=0):
    """Seeded images: a smooth range image plus noise, a prediction near it, ray-drop probabilities; CPU float32 tensors.  One ray-drop value
    is exactly 0.4f, the float32 the default ratio rounds to (the strict `<`)."""
    rng = np.random.default_rng(seed + 100 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    gd = (20.0 + 12.0 * np.sin(xx / 9.0) + 1.5 * yy + rng.uniform(0, 0.5, (H, W))).astype(np.float32)
    gd[rng.uniform(size=(H, W)) < 0.05] = 95.0                        # beyond max_depth: the upper clamp
    pd = (gd + rng.normal(0, 0.2, (H, W))).astype(np.float32)
    gi = rng.uniform(-0.1, 1.1, (H, W)).astype(np.float32)            # both intensity clamps
    pi = (gi + rng.normal(0, 0.05, (H, W))).astype(np.float32)
    pr = rng.uniform(0, 1, (H, W)).astype(np.float32)
    pr[H // 2, W // 2] = np.float32(0.4)
    gm = {"random70": rng.uniform(size=(H, W)) < 0.7, "all_hit": np.ones((H, W), bool), "all_dropped": np.zeros((H, W), bool)}[mask]
    if mask == "all_dropped":
        pr[:] = np.maximum(pr, np.float32(0.4))                       # no predicted return either: both clouds empty
    t = torch.as_tensor
    return (t(pd), t(pi), t(pr)), t(gd), t(gi), t(gm)


def existing_row(pred, gd, gi, gm, use_gt_mask, ratio=0.4, max_depth=80.0):
    """evaluate's own lines on the same tensors (everything but the points, whose operator needs a device)."""
    pd, pi, pr = pred
    gt_hit = gm.bool(); pred_hit = pr < ratio
    mk = (gt_hit if use_gt_mask else pred_hit).to(pd.dtype)
    d = evaluation.depth_metrics(gd, pd * mk, max_depth=max_depth)
    i = evaluation.intensity_metrics(gi.clamp(0, 1), pi.clamp(0, 1.0) * mk)
    r = evaluation.raydrop_metrics(1 - gt_hit.float(), 1 - pred_hit.float())
    return [d[k] for k in ("rmse", "mae", "medae", "ssim", "psnr")] + [i[k] for k in ("rmse", "mae", "medae", "ssim", "psnr")] + [r[k] for k in ("rmse", "acc", "f1")]


def numpy_ssim(x, y):
    """skimage.metrics.structural_similarity(x, y, data_range=y.max() - y.min()) with its defaults, restated in float64 numpy (skimage is not a
    dependency): 7 x 7 uniform filter, sample covariance, K1 = 0.01, K2 = 0.03, the mean over the image cropped by 3 pixels."""
    x = x.astype(np.float64); y = y.astype(np.float64)
    f = lambda a: np.lib.stride_tricks.sliding_window_view(a, (7, 7)).mean((-1, -2))
    ux, uy = f(x), f(y)
    n = 49.0 / 48.0
    vx, vy, vxy = n * (f(x * x) - ux * ux), n * (f(y * y) - uy * uy), n * (f(x * y) - ux * uy)
    R = y.max() - y.min()
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    return float((((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))).mean())


@pytest.mark.parametrize("H,W", SHAPES)
def test_the_twin_restates_the_existing_functions(H, W):
    n = H * W
    # a float32 mean of n terms is within n 2^-24 of the exact one (relative; the terms are non-negative); 4 more roundings around it
    tol = (n + 4) * 2.0 ** -24
    for mask in MASKS:
        for use_gt in (False, True):
            pred, gd, gi, gm = make_case(H, W, mask)
            row = mt.frame_metrics_reference(pred, gd, gi, gm, use_gt_mask=use_gt)
            assert row.dtype == torch.float64 and row.shape == (mt.N,)
            old = existing_row(pred, gd, gi, gm, use_gt)
            tag = (H, W, mask, use_gt)
            assert all(bool(torch.isfinite(v)) for v in old), tag
            for k, ((g, m), new) in enumerate(zip(mt.ROW[:13], row[:13].tolist())):
                ref = float(old[k])
                if m == "medae":
                    assert np.float32(new) == np.float32(ref) and float(np.float32(new)) == new, (tag, g, m)      # the sort's bits
                elif g == "raydrop":
                    assert abs(new - ref) <= EPS * abs(new), (tag, g, m, new, ref)                             # ratios of exact counts, rounded once
                elif m == "psnr":
                    assert abs(new - ref) <= 10 / np.log(10) * 2 * tol + EPS * abs(new), (tag, g, m, new, ref)  # d psnr = 10 / ln 10 * d mse / mse
                elif m == "ssim":
                    assert abs(new - ref) <= 4 * EPS, (tag, g, m, new, ref)        # ssim_uniform is float64 inside: R's float32 subtraction and the final rounding
                else:
                    assert abs(new - ref) <= tol * abs(new), (tag, g, m, new, ref)
            # the counts behind acc and f1, exactly
            pd, pi, pr = pred
            gdrop, pdrop = ~gm.numpy(), ~(pr.numpy() < np.float32(0.4))
            tp, fp, fn, eq = (gdrop & pdrop).sum(), (~gdrop & pdrop).sum(), (gdrop & ~pdrop).sum(), (gdrop == pdrop).sum()
            assert pdrop[H // 2, W // 2]                                          # 0.4f < 0.4 is false: a drop
            assert row[11].item() == eq / n and row[10].item() == np.sqrt((n - eq) / n)
            P, Rc = tp / max(tp + fp, 1), tp / max(tp + fn, 1)
            assert abs(row[12].item() - 2 * P * Rc / max(P + Rc, 1e-30)) <= 1e-15
            mask_np = gm.numpy() if use_gt else ~pdrop
            assert row[15].item() == mask_np.sum() and row[16].item() == gm.numpy().sum()
            # SSIM against the numpy restatement, float64 against float64: another order of summation
            x = np.clip(pd.numpy() * mask_np.astype(np.float32), np.float32(1e-6), np.float32(80.0))
            y = np.clip(gd.numpy(), np.float32(1e-6), np.float32(80.0))
            assert abs(row[3].item() - numpy_ssim(x, y)) <= 1e-9, tag
            xi = np.clip(np.clip(pi.numpy(), 0, 1) * mask_np.astype(np.float32), np.float32(1e-6), np.float32(1.0))
            yi = np.clip(np.clip(gi.numpy(), 0, 1), np.float32(1e-6), np.float32(1.0))
            assert abs(row[8].item() - numpy_ssim(xi, yi)) <= 1e-9, tag
            assert np.isnan(row[13].item()) and np.isnan(row[14].item())          # no rays: the points are skipped


def test_the_twins_points_against_plain_numpy_and_the_empty_clouds():
    H, W = 8, 9
    pred, gd, gi, gm = make_case(H, W, "random70")
    rng = np.random.default_rng(3)
    d = rng.standard_normal((H, W, 3)); d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.broadcast_to(np.array([0.5, -1.0, 2.0]), (H, W, 3))
    rays = (torch.as_tensor(o.astype(np.float32).copy()), torch.as_tensor(d.astype(np.float32)))
    row = mt.frame_metrics_reference(pred, gd, gi, gm, rays, threshold=0.05)
    hit_b = pred[2].numpy() < np.float32(0.4)
    a = (rays[0].numpy() + rays[1].numpy() * gd.numpy()[..., None]).reshape(-1, 3)[gm.numpy().reshape(-1)].astype(np.float64)
    b = (rays[0].numpy() + rays[1].numpy() * pred[0].numpy()[..., None]).reshape(-1, 3)[hit_b.reshape(-1)].astype(np.float64)
    d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    da, db = d2.min(1), d2.min(0)
    assert abs(row[13].item() - (da.mean() + db.mean())) <= 4 * EPS * (da.mean() + db.mean())       # float32 distances against float64 ones
    assert min(abs(da - 0.05).min(), abs(db - 0.05).min()) > 1e-5                                   # no distance sits on the threshold
    p1, p2 = (da < 0.05).mean(), (db < 0.05).mean()
    assert 0 < p1 < 1 and abs(row[14].item() - 2 * p1 * p2 / (p1 + p2)) <= 1e-15
    assert row[15].item() == hit_b.sum() == b.shape[0] and row[16].item() == gm.numpy().sum()
    # an empty cloud, either one: NaN and 0, as points_metrics
    none = torch.zeros_like(gm)
    r1 = mt.frame_metrics_reference(pred, gd, gi, none, rays)
    r2 = mt.frame_metrics_reference((pred[0], pred[1], torch.ones_like(pred[2])), gd, gi, gm, rays)
    for r in (r1, r2):
        assert np.isnan(r[13].item()) and r[14].item() == 0.0
    assert r1[16].item() == 0 and r2[15].item() == 0
    # a constant ground truth: R = 0, NaN
    rc = mt.frame_metrics_reference(pred, torch.full_like(gd, 7.0), gi, gm)
    assert np.isnan(rc[3].item()) and np.isfinite(rc[8].item()) and np.isfinite(rc[0].item())


# ---- the arithmetic header on the host -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("metrics_check") / "libmetrics_check.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", lib, os.path.join(HERE, "host_check", "metrics_check.cpp")])
    lib = C.CDLL(lib)
    lib.mt_ssim_image.restype = C.c_double
    lib.mt_ssim_image.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    lib.mt_median_of.restype = C.c_float; lib.mt_median_of.argtypes = [C.c_uint32, C.c_uint32]
    lib.mt_find.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.mt_find_chunked.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_void_p]
    for f, n in (("mt_f1_of", 3), ("mt_fscore_of", 4), ("mt_psnr_of", 3), ("mt_rmse_of", 2)):
        getattr(lib, f).restype = C.c_double; getattr(lib, f).argtypes = [C.c_double] * n
    return lib


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("H,W", SHAPES)
def test_clamps_keys_and_window_statistics_on_the_host(host, H, W):
    for mask in MASKS:
        pred, gd, gi, gm = make_case(H, W, mask)
        m8 = (pred[2].numpy() < np.float32(0.4)).astype(np.uint8)
        for image, (p, g) in enumerate(((pred[0], gd), (pred[1], gi))):
            x, y = np.empty(H * W, np.float32), np.empty(H * W, np.float32)
            key = np.empty(H * W, np.uint32)
            host.mt_pairs(H * W, image, ptr(p.numpy()), ptr(g.numpy()), ptr(m8), C.c_float(80.0), ptr(x), ptr(y), ptr(key))
            mk = torch.as_tensor(m8.reshape(H, W)).float()
            if image == 0:
                wx, wy = (p * mk).clamp(1e-6, 80.0), g.clamp(1e-6, 80.0)
            else:
                wx, wy = (p.clamp(0, 1) * mk).clamp(1e-6, 1.0), g.clamp(0, 1).clamp(1e-6, 1.0)
            assert np.array_equal(x, wx.numpy().ravel()) and np.array_equal(y, wy.numpy().ravel())
            assert np.array_equal(key.view(np.float32), (wy - wx).abs().numpy().ravel())
            sums = np.empty((H - 6, W - 6, 5), np.float64)
            R = float(y.max()) - float(y.min())
            mean = host.mt_ssim_image(H, W, ptr(x), ptr(y), R, ptr(sums))
            X, Y = x.reshape(H, W).astype(np.float64), y.reshape(H, W).astype(np.float64)
            win = lambda a: np.lib.stride_tricks.sliding_window_view(a, (7, 7)).sum((-1, -2))
            for k, a in enumerate((X, Y, X * X, Y * Y, X * Y)):
                assert np.allclose(sums[..., k], win(a), rtol=1e-14, atol=0), (H, W, mask, image, k)
            assert abs(mean - numpy_ssim(X, Y)) <= 1e-9, (H, W, mask, image)


def test_scalar_formulas_on_the_host(host):
    assert host.mt_f1_of(0.0, 0.0, 0.0) == 0.0 and host.mt_f1_of(3.0, 1.0, 2.0) == 2 * 0.75 * 0.6 / (0.75 + 0.6)
    assert host.mt_fscore_of(0.0, 10.0, 0.0, 10.0) == 0.0 and host.mt_fscore_of(5.0, 0.0, 5.0, 10.0) == 0.0
    assert host.mt_fscore_of(5.0, 10.0, 10.0, 10.0) == 2 * 0.5 * 1.0 / 1.5
    assert host.mt_psnr_of(0.0, 10.0, 80.0) == 10 * np.log10(6400.0 / 1e-30) and np.isnan(host.mt_psnr_of(float("nan"), 10.0, 80.0))
    assert host.mt_rmse_of(40.0, 10.0) == 2.0


def select(host, values):
    """(the two middle elements as float32, split level) from the three-level selection of the header."""
    v = np.ascontiguousarray(values, np.float32)
    keys = v.view(np.uint32)
    out = np.zeros(2, np.uint32); split = C.c_int(-1)
    rc = host.mt_select(len(v), ptr(keys), ptr(out), C.byref(split))
    assert rc == 0, rc
    return out.view(np.float32), split.value, out


def selection_cases():
    rng = np.random.default_rng(11)
    nx = lambda x: np.nextafter(np.float32(x), np.float32(np.inf))
    c = {}
    c["odd_random_49"] = (rng.uniform(0, 3, 49), None)
    c["even_random_72"] = (rng.uniform(0, 3, 72), None)
    c["odd_random_4001_many_exponents"] = (10.0 ** rng.uniform(-6, 2, 4001), None)
    c["even_random_4000_with_zeros"] = (np.where(rng.uniform(size=4000) < 0.3, 0.0, rng.uniform(0, 80, 4000)), None)
    c["both_ranks_in_one_bin_at_every_level"] = (np.r_[np.full(20, 0.5), np.full(12, 1.25), np.full(20, 7.0)], 0)
    c["all_equal_72"] = (np.full(72, 0.3), 0)
    c["all_zero_49"] = (np.zeros(49), 0)
    c["split_at_level_1"] = (np.r_[rng.uniform(0.01, 0.02, 36), rng.uniform(5, 9, 36)], 1)              # the middle pair: ~0.02 and ~5
    c["split_at_level_2"] = (np.r_[np.full(36, 1.0), np.full(36, 1.0 + 2.0 ** -10)], 2)                # same top 11 bits, bit 13 of the mantissa differs
    c["split_at_level_3"] = (np.r_[np.full(36, 1.0), np.full(36, nx(1.0))], 3)                         # neighbours: the last bit
    c["more_than_half_zero_even"] = (np.r_[np.zeros(40), rng.uniform(0, 1, 32)], 0)
    c["zero_against_smallest_subnormal"] = (np.r_[np.zeros(36), np.full(36, nx(0.0))], 3)
    c["odd_with_infinity"] = (np.r_[rng.uniform(0, 1, 24), np.full(25, np.inf)], 0)
    return c


@pytest.mark.parametrize("name", list(selection_cases()))
def test_selection_returns_the_sorted_arrays_two_middle_elements(host, name):
    values, want_split = selection_cases()[name]
    v = np.asarray(values, np.float32)
    rng = np.random.default_rng(5)
    v = v[rng.permutation(len(v))]
    got, split, keys = select(host, v)
    s = np.sort(v)
    n = len(v)
    assert got[0].tobytes() == s[(n - 1) // 2].tobytes() and got[1].tobytes() == s[n // 2].tobytes(), (name, got, s[(n - 1) // 2], s[n // 2])
    if want_split is not None:
        assert split == want_split, (name, split)
    if n % 2:
        assert split == 0 and keys[0] == keys[1]
    med = host.mt_median_of(int(keys[0]), int(keys[1]))
    want = torch.as_tensor(v).sort().values
    want = 0.5 * (want[(n - 1) // 2] + want[n // 2])                                  # evaluation._median
    assert np.float32(med).tobytes() == want.numpy().tobytes() and np.float32(med) == np.median(v)


def test_find_bin_on_constructed_histograms(host):
    h = np.zeros(2048, np.uint32)
    h[[3, 700, 701, 2047]] = [5, 1, 2, 4]
    r = C.c_uint32(99)
    for k, (b, rank) in {0: (3, 0), 4: (3, 4), 5: (700, 0), 6: (701, 0), 7: (701, 1), 8: (2047, 0), 11: (2047, 3)}.items():
        assert host.mt_find(ptr(h), 2048, 0, k, C.byref(r)) == b and r.value == rank, k
        for per in (8, 2):
            assert host.mt_find_chunked(ptr(h), 2048, per, k, C.byref(r)) == b and r.value == rank, (k, per)     # exactly one chunk claims the rank
    assert host.mt_find(ptr(h), 2048, 0, 12, C.byref(r)) == -1 and host.mt_find_chunked(ptr(h), 2048, 8, 12, C.byref(r)) == -1
    assert host.mt_find(ptr(h), 2048, 6, 5, C.byref(r)) == -1                       # the rank lies before these bins
    assert host.mt_find(ptr(h), 2048, 6, 6, C.byref(r)) == 3 and r.value == 0
