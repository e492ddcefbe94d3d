"""The fused range-image loss without a GPU: the PyTorch restatement (`losses.range_image_loss_torch`) against the reference's recorded
numbers and against `training_step`'s expression, the second product library (`liblrt_loss.so`: builds, exports, resource gate, a source
list of its own), and the per-pixel math header compiled for the host."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lidar_rt_amd import build as lrt_build, losses, resources, training

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
G = np.load(os.path.join(HERE, "golden", "loop_golden.npz"))


def _opt(**kw):
    o = training.default_options()
    for k in ("lambda_depth_l1", "lambda_intensity_l1", "lambda_intensity_l2", "lambda_intensity_dssim", "lambda_raydrop_bce"):
        setattr(o, k, 0.0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_torch_restatement_reproduces_the_reference_loss_utils_numbers():
    """tests/golden/loop_golden.npz holds the reference's l1_loss / l2_loss / ssim / BCE on recorded inputs; tolerances of tests/test_loop_golden.py."""
    a, b = torch.as_tensor(G["loss_img_a"])[0], torch.as_tensor(G["loss_img_b"])[0]
    H, W = a.shape
    img = torch.zeros(H, W, 9); img[:, :, 0] = a
    ones = torch.ones(H, W, dtype=torch.bool)
    z = torch.zeros(H, W)
    term = lambda **kw: float(losses.range_image_loss_torch(img, z, b, ones, _opt(**kw))[2])
    assert abs(term(lambda_intensity_l1=1.0) - float(G["loss_l1"])) < 1e-7
    assert abs(term(lambda_intensity_l2=1.0) - float(G["loss_l2"])) < 1e-7
    assert abs((1.0 - term(lambda_intensity_dssim=1.0)) - float(G["loss_ssim"])) < 2e-6
    # BCE: the recorded probabilities as ray-drop logits (float64, so that sigmoid(logit(p)) returns p to far below the tolerance); label = 1 - mask
    p = torch.as_tensor(G["bce_preds"]).double().reshape(H, W)
    img64 = torch.zeros(H, W, 9, dtype=torch.float64); img64[:, :, 2] = torch.log(p / (1 - p))
    mask = ~torch.as_tensor(G["bce_labels"]).reshape(H, W)
    tot, _, _, drop, n = losses.range_image_loss_torch(img64, z.double(), z.double(), mask, _opt(lambda_raydrop_bce=1.0))
    assert abs(float(drop) - float(G["loss_bce"])) < 1e-6 and float(tot) == float(drop) and float(n) == float(mask.sum())


@pytest.mark.parametrize("use_rayhit", [False, True])
def test_torch_restatement_equals_the_training_step_expression_bit_for_bit(use_rayhit):
    """The same code moved: from the package renderer.raytracing returns (slices of the raw image + the ray-drop probability) through the lines of
    training_step's attempt(), on a seeded float32 case with a mask."""
    g = torch.Generator().manual_seed(5)
    H, W = 24, 70
    rendered = torch.randn(H, W, 9, generator=g)
    rendered[:, :, 0] = torch.rand(H, W, generator=g); rendered[:, :, 3] = 20 * torch.rand(H, W, generator=g)
    rendered[:, :, 2] *= 6.0
    gt_depth, gt_int = 20 * torch.rand(H, W, generator=g), torch.rand(H, W, generator=g)
    mask = torch.rand(H, W, generator=g) < 0.7
    opt = training.default_options(); opt.use_rayhit = use_rayhit; opt.lambda_intensity_l2 = 0.3
    # renderer.raytracing's tail
    if use_rayhit:
        raydrop = F.softmax(torch.cat([rendered[:, :, 1:2], rendered[:, :, 2:3]], dim=-1), dim=-1)[..., 1:2]
    else:
        raydrop = torch.sigmoid(rendered[:, :, 2:3])
    pkg = {"depth": rendered[:, :, 3:4], "intensity": rendered[:, :, 0:1], "raydrop": raydrop}
    # training_step's attempt()
    depth, intensity, raydrop = pkg["depth"].squeeze(-1), pkg["intensity"].squeeze(-1), pkg["raydrop"]
    mf = mask.to(depth.dtype)
    n_valid = mf.sum().clamp_min(1.0)
    mmean = lambda x: (x * mf).sum() / n_valid
    loss_depth = opt.lambda_depth_l1 * mmean(torch.abs(depth - gt_depth))
    loss_int = (opt.lambda_intensity_l1 * mmean(torch.abs(intensity - gt_int))
                + opt.lambda_intensity_l2 * mmean((intensity - gt_int) ** 2)
                + opt.lambda_intensity_dssim * (1 - training.ssim((intensity * mf).unsqueeze(0), (gt_int * mf).unsqueeze(0))))
    labels = (1.0 - mf).reshape(-1, 1)
    loss_drop = opt.lambda_raydrop_bce * F.binary_cross_entropy(raydrop.reshape(-1, 1).clamp(1e-7, 1 - 1e-7), labels)
    got = losses.range_image_loss_torch(rendered, gt_depth, gt_int, mask, opt)
    for want, have in zip((loss_depth + loss_int + loss_drop, loss_depth, loss_int, loss_drop, n_valid), got):
        assert torch.equal(want, have)


def test_torch_restatement_is_dtype_generic_and_differentiable():
    g = torch.Generator().manual_seed(2)
    rendered = torch.rand(7, 13, 9, generator=g, dtype=torch.float64).requires_grad_(True)
    tot = losses.range_image_loss_torch(rendered, torch.rand(7, 13, generator=g, dtype=torch.float64), torch.rand(7, 13, generator=g, dtype=torch.float64),
                                        torch.rand(7, 13, generator=g) < 0.5, training.default_options())[0]
    assert tot.dtype == torch.float64
    tot.backward()
    assert rendered.grad.abs().sum() > 0 and float(rendered.grad[:, :, 4:].abs().sum()) == 0.0 and float(rendered.grad[:, :, 1].abs().sum()) == 0.0


def test_default_options_keep_the_fused_loss_off():
    assert training.default_options().fused_loss is False


# ---- the library ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def loss_lib():
    return lrt_build.build_loss()


def test_the_loss_library_has_a_source_list_of_its_own():
    """liblrt_hip.so's source_hash() keys committed profiles: the loss sources must not be part of it."""
    for f in lrt_build.LOSS_SOURCES + lrt_build.LOSS_HEADERS:
        if os.path.basename(f) == "lrt_device_guard.h":
            continue                                                   # shared, unchanged
        assert f not in lrt_build.SOURCES and f not in lrt_build.HEADERS, f
    assert "lrt_loss.hip" in lrt_build.LOSS_SOURCES and "lrt_loss_math.h" in lrt_build.LOSS_HEADERS
    assert not any("lrt_loss" in f for f in lrt_build.SOURCES + lrt_build.HEADERS)
    assert lrt_build.loss_source_hash() != lrt_build.source_hash()
    assert os.path.basename(lrt_build.LOSS_LIB) == "liblrt_loss.so" and lrt_build.LOSS_LIB != lrt_build.LIB


def test_the_library_builds_and_exports_what_its_header_declares(loss_lib):
    assert os.path.exists(loss_lib) and not lrt_build.loss_is_stale()
    assert open(lrt_build.LOSS_STAMP).read().strip() == lrt_build.loss_source_hash()
    hdr = open(os.path.join(REPO, "include", "lrt_loss.h")).read()
    declared = set(re.findall(r"\b(lrt_loss_[a-z_]+)\s*\(", hdr))
    assert declared == set(losses.EXPORTS), declared ^ set(losses.EXPORTS)
    lib = losses.load()
    for n in declared:
        assert hasattr(lib, n), n
    from lidar_rt_amd import _capi
    assert not any(n.startswith("lrt_loss") for n in _capi.EXPORTS)
    assert lib.lrt_loss_abi_version() == int(re.search(r"#define\s+LRT_LOSS_ABI_VERSION\s+(\d+)", hdr).group(1))


def test_work_bytes_and_argument_errors_without_a_device(loss_lib):
    lib = losses.load()
    assert lib.lrt_loss_work_bytes(0, 5) == 0 and lib.lrt_loss_work_bytes(5, -1) == 0
    nb = lib.lrt_loss_work_bytes(66, 1030)
    assert nb >= 3 * 66 * 1030 * 4 + 5 * 33 * 6 * 8
    w = (C.c_double * 5)(0.1, 0.85, 0.0, 0.15, 0.01)
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    dev = 1 << 20                                     # no machine has this many devices; without any, device 0 gets the same answer
    for d in ((dev,) if torch.cuda.is_available() else (dev, 0)):
        rc = lib.lrt_loss_forward(d, 4, 4, p, p, p, p, w, 0, p, p, nb, None)
        assert rc < 0 and b"no HIP device" in lib.lrt_loss_last_error()
        rc = lib.lrt_loss_backward(d, 4, 4, p, p, p, p, w, 0, p, p, p, nb, None)
        assert rc < 0 and b"no HIP device" in lib.lrt_loss_last_error()


def test_every_kernel_of_the_loss_library_passes_the_resource_gate(loss_lib):
    res = resources.kernel_resources(loss_lib)
    own = sorted(n for n in res if resources.is_own_kernel(n))
    assert own == ["k_loss_bwd", "k_loss_fin", "k_loss_fwd"], own
    assert all(any(re.search(g_, n) for g_ in resources.GATED) for n in own)          # the gate looks at each of them
    assert resources.violations(res) == []
    for n in own:
        assert res[n]["vgpr_spill"] == 0 and res[n]["scratch_bytes"] == 0 and not res[n]["dynamic_stack"], (n, res[n])
        assert res[n]["lds_bytes"] <= 64 * 1024
    resources.check(loss_lib)


def test_range_image_loss_refuses_cpu_tensors():
    with pytest.raises(losses.LossError):
        losses.range_image_loss(torch.zeros(4, 4, 9), torch.zeros(4, 4), torch.zeros(4, 4), torch.ones(4, 4, dtype=torch.bool), training.default_options())


# ---- the math header on the host ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lc():
    src = os.path.join(HERE, "host_check", "loss_check.cpp")
    hdr = os.path.join(REPO, "lidar_rt_amd", "csrc", "lrt_loss_math.h")
    lib = os.path.join(HERE, "host_check", "libloss_check.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", lib, src])
    return C.CDLL(lib)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_window_weights(lc):
    w = np.zeros(11, np.float32)
    lc.lc_window(_p(w))
    assert abs(float(w.astype(np.float64).sum()) - 1.0) < 2e-7 and np.array_equal(w, w[::-1]) and w.argmax() == 5
    band = training._blur_matrix(40, 11, "cpu", torch.float32)
    for row in (0, 3, 20, 39):                       # row i of the banded matrix holds the window centred on i, cut at the borders (zero padding)
        for k in range(11):
            j = row + k - 5
            if 0 <= j < 40:
                assert float(band[row, j]) == float(w[k]), (row, k)
    exact = np.exp(-(np.arange(11) - 5.0) ** 2 / 4.5); exact /= exact.sum()
    assert np.abs(w - exact).max() < 1e-7


def _ssim_closed_form(mu1, mu2, e11, e22, e12):
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    s1, s2, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
    return ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))


def test_ssim_partials_against_float64_autograd(lc):
    rng = np.random.default_rng(3)
    n = 4000
    # window statistics of plausible images: means in [0, 1], variances >= 0, |covariance| <= sqrt(var1 var2); a quarter of them flat (masked) windows
    mu1, mu2 = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    v1, v2 = rng.uniform(0, 0.08, n), rng.uniform(0, 0.08, n)
    rho = rng.uniform(-1, 1, n)
    flat = rng.uniform(size=n) < 0.25
    mu1[flat] *= 1e-3; v1[flat] = 0
    inp = np.stack([mu1, mu2, v1 + mu1 ** 2, v2 + mu2 ** 2, rho * np.sqrt(v1 * v2) + mu1 * mu2], 1).copy()
    out = np.zeros((n, 4))
    lc.lc_ssim_f64(n, _p(inp), _p(out))
    t = torch.tensor(inp, requires_grad=True)
    S = _ssim_closed_form(*t.unbind(1))
    S.sum().backward()
    gr = t.grad.numpy()
    np.testing.assert_allclose(out[:, 0], S.detach().numpy(), rtol=1e-12, atol=1e-14)
    for col, k in ((1, 0), (2, 2), (3, 4)):                              # dS/dmu1 (total), dS/de11, dS/de12
        np.testing.assert_allclose(out[:, col], gr[:, k], rtol=1e-9, atol=1e-9 * np.abs(gr[:, k]).max())
    # the float32 instantiation: the same formulas at float32 precision (the cancellation e11 - mu1^2 costs digits: compared at the scale of the inputs)
    o32 = np.zeros((n, 4), np.float32)
    i32 = inp.astype(np.float32)
    lc.lc_ssim_f32(n, _p(i32), _p(o32))
    o64 = np.zeros((n, 4)); i64 = i32.astype(np.float64)
    lc.lc_ssim_f64(n, _p(i64), _p(o64))
    assert np.abs(o32[:, 0] - o64[:, 0]).max() < 1e-2 and np.median(np.abs(o32[:, 0] - o64[:, 0])) < 1e-5


@pytest.mark.parametrize("use_rayhit", [0, 1])
def test_bce_with_clamp_against_torch(lc, use_rayhit):
    rng = np.random.default_rng(9)
    n = 6000
    hit = (rng.standard_normal(n) * 3).astype(np.float32)
    drop = (rng.standard_normal(n) * 12).astype(np.float32)               # many probabilities beyond the clamp on both sides
    drop[:8] = [0.0, 16.0, 16.2, 17.0, -16.2, -17.0, 40.0, -40.0]
    label = (rng.uniform(size=n) < 0.4).astype(np.float32)
    out = np.zeros((n, 3), np.float32)
    lc.lc_bce(n, _p(hit), _p(drop), _p(label), use_rayhit, _p(out))
    th, td = torch.tensor(hit), torch.tensor(drop)
    p = F.softmax(torch.stack([th, td], -1), -1)[:, 1] if use_rayhit else torch.sigmoid(td)
    assert int((p < 1e-7).sum()) > 50 and int((p > 1 - 1e-7).sum()) > 50
    np.testing.assert_allclose(out[:, 0], p.numpy(), rtol=1e-5, atol=1e-37)
    # clamp + BCE and their backwards from the header's OWN probability (a one-ulp difference between two exponentials would flip the clamp's
    # decision at its thresholds): torch.clamp and F.binary_cross_entropy under autograd, times dp/dz = p (1 - p)
    pm = torch.tensor(out[:, 0], requires_grad=True)
    v = F.binary_cross_entropy(pm.clamp(1e-7, 1 - 1e-7), torch.tensor(label), reduction="none")
    v.sum().backward()
    dz = (pm.grad * (pm * (1 - pm)).detach()).numpy()
    np.testing.assert_allclose(out[:, 1], v.detach().numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(out[:, 2], dz, rtol=1e-5, atol=1e-12)
    outside = (out[:, 0] < np.float32(1e-7)) | (out[:, 0] > np.float32(1 - 1e-7))
    assert outside.sum() > 100 and np.all(out[outside, 2] == 0) and np.all(out[~outside, 2] != 0)     # gradient exactly where torch.clamp passes it
