"""The grid Chamfer operator without a GPU: the third product library (`liblrt_gridcd.so`: builds, exports, resource gate, a source list of its
own that leaves the other two libraries' hashes where they were), the PyTorch yardstick (`grid_chamfer.grid_chamfer_torch`) against an
independent numpy brute force, and the arithmetic header compiled for the host."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from lidar_rt_amd import build as lrt_build, grid_chamfer as gc, resources, training

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def gridcd_lib():
    return lrt_build.build_gridcd()


def test_the_library_has_a_source_list_of_its_own_and_moves_no_other_hash():
    for f in lrt_build.GRIDCD_SOURCES + lrt_build.GRIDCD_HEADERS:
        if os.path.basename(f) == "lrt_device_guard.h":
            continue                                                   # shared, unchanged
        for other in (lrt_build.SOURCES, lrt_build.HEADERS, lrt_build.LOSS_SOURCES, lrt_build.LOSS_HEADERS):
            assert f not in other, f
    assert "lrt_gridcd.hip" in lrt_build.GRIDCD_SOURCES and "lrt_gridcd_math.h" in lrt_build.GRIDCD_HEADERS
    assert not any("gridcd" in f for f in lrt_build.SOURCES + lrt_build.HEADERS + lrt_build.LOSS_SOURCES + lrt_build.LOSS_HEADERS)
    # the values of the commits the other two libraries were last changed by: committed profiles are keyed by them (the tracer library's:
    # 71ad66c6f4addc35 when this library was added, moved since by the sorted-key read-back of lrt_debug_read and then by
    # its read-back of the AoS nodes (selector 10) -- host code, no kernel changed either time: tests/test_resources.py holds unchanged)
    assert lrt_build.source_hash() == "2c98b54882a7ff74"          # moved twice since: the non-finite-input fixes in lrt_chamfer.hip; a comment of include/lrt.h (lrt_xchg_apply, zero_only on an overflowed block)
    assert lrt_build.loss_source_hash() == "cc56b0c83f72d5ca"
    assert lrt_build.gridcd_source_hash() not in (lrt_build.source_hash(), lrt_build.loss_source_hash())
    assert os.path.basename(lrt_build.GRIDCD_LIB) == "liblrt_gridcd.so" and lrt_build.GRIDCD_LIB not in (lrt_build.LIB, lrt_build.LOSS_LIB)


def test_the_library_builds_and_exports_what_its_header_declares(gridcd_lib):
    assert os.path.exists(gridcd_lib) and not lrt_build.gridcd_is_stale()
    assert open(lrt_build.GRIDCD_STAMP).read().strip() == lrt_build.gridcd_source_hash()
    hdr = open(os.path.join(REPO, "include", "lrt_gridcd.h")).read()
    declared = set(re.findall(r"\b(lrt_gridcd_[a-z_]+)\s*\(", hdr))
    assert declared == set(gc.EXPORTS), declared ^ set(gc.EXPORTS)
    lib = gc.load()
    for n in declared:
        assert hasattr(lib, n), n
    assert lib.lrt_gridcd_abi_version() == int(re.search(r"#define\s+LRT_GRIDCD_ABI_VERSION\s+(\d+)", hdr).group(1)) == gc.ABI_VERSION


def test_every_kernel_passes_the_resource_gate(gridcd_lib):
    res = resources.kernel_resources(gridcd_lib)
    own = sorted(n for n in res if resources.is_own_kernel(n))
    assert len(own) >= 6 and all(n.startswith("k_gc_") for n in own), own
    assert all(any(re.search(g_, n) for g_ in resources.GATED) for n in own)          # the gate looks at each of them
    assert resources.violations(res) == []
    for n in own:
        assert res[n]["vgpr_spill"] == 0 and res[n]["scratch_bytes"] == 0 and not res[n]["dynamic_stack"], (n, res[n])
        assert res[n]["lds_bytes"] <= 64 * 1024
    resources.check(gridcd_lib)


def test_work_bytes_and_argument_errors_without_a_device(gridcd_lib):
    lib = gc.load()
    assert lib.lrt_gridcd_work_bytes(0, 5) == 0 and lib.lrt_gridcd_work_bytes(5, -1) == 0 and lib.lrt_gridcd_work_bytes(1 << 14, 1 << 14) == 0
    nb = lib.lrt_gridcd_work_bytes(66, 1030)
    assert nb >= 2 * 66 * 1030 * 16 and nb % 16 == 0
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    dev = 1 << 20                                     # no machine has this many devices; without any, device 0 gets the same answer
    for d in ((dev,) if torch.cuda.is_available() else (dev, 0)):
        rc = lib.lrt_gridcd_forward(d, 4, 4, p, p, p, p, p, p, 1.0, p, p, p, p, p, p, nb, None)
        assert rc < 0 and b"no HIP device" in lib.lrt_gridcd_last_error()
        rc = lib.lrt_gridcd_backward(d, 4, 4, p, p, p, p, p, p, 1.0, p, p, p, p, p, p, p, nb, None)
        assert rc < 0 and b"no HIP device" in lib.lrt_gridcd_last_error()


def test_grid_chamfer_refuses_cpu_tensors_and_wrong_shapes():
    o, d, r, m = torch.zeros(4, 4, 3), torch.ones(4, 4, 3), torch.ones(4, 4), torch.ones(4, 4, dtype=torch.bool)
    with pytest.raises(gc.GridChamferError, match="HIP"):
        gc.grid_chamfer(o, d, r, r, m)
    with pytest.raises(gc.GridChamferError):
        gc.grid_chamfer_nearest(o, d, r.double(), r, m)


def test_default_options_keep_the_grid_operator_off():
    assert training.default_options().grid_chamfer is False


def test_train_has_the_two_flags_and_the_amended_help():
    from lidar_rt_amd import train
    src = open(train.__file__).read()
    assert '"--grid-chamfer"' in src and '"--chamfer-grad"' in src and "chamfer_points_detached=not args.chamfer_grad" in src
    assert "--grid-chamfer for lambda_cd != 0" in src


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------------------

def _numpy_brute(o, d, ra, rb, ma, mb, weight):
    """Independent restatement: loops over the queries, float64, first minimum in pixel order."""
    H, W = ra.shape
    pa = (o + d * ra[..., None]).reshape(-1, 3); pb = (o + d * rb[..., None]).reshape(-1, 3)
    ia, ib = np.flatnonzero(ma.reshape(-1)), np.flatnonzero(mb.reshape(-1))
    dist = [np.zeros(H * W), np.zeros(H * W)]
    idx = [np.full(H * W, -1), np.full(H * W, -1)]
    for k, (qi, q, ci, c) in enumerate(((ia, pa, ib, pb), (ib, pb, ia, pa))):
        for i in qi:
            if len(ci) == 0:
                continue
            dd = ((c[ci] - q[i]) ** 2).sum(1)
            j = int(np.argmin(dd))                               # numpy: the first occurrence
            dist[k][i], idx[k][i] = dd[j], ci[j]
    if len(ia) == 0 or len(ib) == 0:
        return 0.0, 0.0, 0.0, dist, idx
    m_a, m_b = dist[0][ia].mean(), dist[1][ib].mean()
    return weight * 0.5 * (m_a + m_b), m_a, m_b, dist, idx


@pytest.mark.parametrize("case", ["random", "ties", "two_masks", "one_pixel", "empty"])
def test_torch_yardstick_equals_numpy_brute_force(case):
    rng = np.random.default_rng(4)
    H, W = 6, 11
    o = np.broadcast_to(rng.standard_normal(3), (H, W, 3)).copy()
    d = rng.standard_normal((H, W, 3)); d /= np.linalg.norm(d, axis=-1, keepdims=True)
    ra, rb = rng.uniform(1, 30, (H, W)), rng.uniform(1, 30, (H, W))
    ma = rng.uniform(size=(H, W)) < 0.7
    mb = ma
    if case == "ties":                                  # rays quantised to a coarse grid, constant ranges: distinct pixels, identical points
        d = np.round(d * 2) / 2; d[np.abs(d).sum(-1) == 0] = (1.0, 0.0, 0.0)
        o[:] = 0.0; ra[:] = 4.0; rb[:] = 4.0
    elif case == "two_masks":
        mb = rng.uniform(size=(H, W)) < 0.5
    elif case == "one_pixel":
        ma = np.zeros((H, W), bool); ma[3, 5] = True; mb = ma
    elif case == "empty":
        mb = np.zeros((H, W), bool)
    want = _numpy_brute(o, d, ra, rb, ma, mb, 0.7)
    t = lambda x: torch.as_tensor(x)
    loss, m_a, m_b = gc.grid_chamfer_torch(t(o), t(d), t(ra), t(rb), t(ma), None if mb is ma else t(mb), weight=0.7)
    assert loss.dtype == torch.float64
    for have, w in zip((loss, m_a, m_b), want[:3]):
        assert abs(float(have) - w) <= 1e-12 * max(1.0, abs(w)), (float(have), w)
    if case == "empty":
        assert float(loss) == 0.0 and float(m_a) == 0.0 and float(m_b) == 0.0
        return
    # the neighbours the yardstick differentiates through: the first minimum, ties included
    pa = (t(o) + t(d) * t(ra)[..., None]).reshape(-1, 3); pb = (t(o) + t(d) * t(rb)[..., None]).reshape(-1, 3)
    ia, ib = np.flatnonzero(ma.reshape(-1)), np.flatnonzero(mb.reshape(-1))
    nn = gc._nearest_torch(pa[ia], pb[ib]).numpy()
    assert np.array_equal(ib[nn], want[4][0][ia])
    if case == "ties":
        dd = ((pb[ib][None] - pa[ia][:, None]) ** 2).sum(-1).numpy()
        assert ((dd == dd.min(1, keepdims=True)).sum(1) > 1).any()       # the case does hold exact ties


def test_torch_yardstick_is_differentiable_in_ranges_and_rays():
    g = torch.Generator().manual_seed(1)
    H, W = 5, 9
    o = torch.randn(3, generator=g, dtype=torch.float64).expand(H, W, 3).clone().requires_grad_(True)
    d = torch.nn.functional.normalize(torch.randn(H, W, 3, generator=g, dtype=torch.float64), dim=-1).requires_grad_(True)
    ra = (5 + torch.rand(H, W, generator=g, dtype=torch.float64)).requires_grad_(True)
    rb = 5 + torch.rand(H, W, generator=g, dtype=torch.float64)
    m = torch.rand(H, W, generator=g) < 0.8
    loss = gc.grid_chamfer_torch(o, d, ra, rb, m)[0]
    loss.backward()
    assert float(ra.grad.abs().sum()) > 0 and float(ra.grad[~m].abs().sum()) == 0.0
    assert float(o.grad.abs().sum()) > 0 and float(d.grad.abs().sum()) > 0
    # an empty cloud: exact zeros, gradients included
    ra.grad = None
    loss = gc.grid_chamfer_torch(o, d, ra, rb, torch.zeros(H, W, dtype=torch.bool))[0]
    loss.backward()
    assert float(loss.detach()) == 0.0 and float(ra.grad.abs().sum()) == 0.0


# ---- the arithmetic header on the host ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hc():
    src = os.path.join(HERE, "host_check", "gridcd_check.cpp")
    hdr = os.path.join(REPO, "lidar_rt_amd", "csrc", "lrt_gridcd_math.h")
    lib = os.path.join(HERE, "host_check", "libgridcd_check.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", lib, src])
    lib = C.CDLL(lib)
    lib.gc_empty.restype = C.c_float; lib.gc_big.restype = C.c_float
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_point_formation_equals_numpy_float32_bit_for_bit(hc):
    rng = np.random.default_rng(7)
    n = 200_000
    o = rng.uniform(-50, 50, n).astype(np.float32); d = rng.uniform(-1, 1, n).astype(np.float32); r = rng.uniform(0.5, 80, n).astype(np.float32)
    out = np.zeros(n, np.float32)
    hc.gc_points(n, _p(o), _p(d), _p(r), _p(out))
    want = o + d * r                                            # numpy float32: a rounded product, then a rounded sum
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    fused = (o.astype(np.float64) + d.astype(np.float64) * r.astype(np.float64)).astype(np.float32)
    assert (fused != want).any()                                 # the inputs do tell two roundings from one


def test_pair_distance_is_the_fma_chain_of_the_existing_operator(hc):
    rng = np.random.default_rng(8)
    n = 50_000
    q = rng.uniform(-40, 40, (n, 3)).astype(np.float32); p = (q + rng.normal(0, 0.3, (n, 3))).astype(np.float32)
    out = np.zeros(n, np.float32)
    hc.gc_pairs(n, _p(q), _p(p), _p(out))
    dv = (p - q).astype(np.float64)                              # the float32 differences, then each fma exact in float64 and rounded once
    t = (dv[:, 0] * dv[:, 0]).astype(np.float32).astype(np.float64)
    t = (dv[:, 1] * dv[:, 1] + t).astype(np.float32).astype(np.float64)
    want = (dv[:, 2] * dv[:, 2] + t).astype(np.float32)
    assert np.array_equal(out, want)


def test_tile_bound_never_exceeds_the_pair_expression_inside_the_box(hc):
    rng = np.random.default_rng(9)
    n = 400_000
    c = rng.uniform(-60, 60, (n, 3)); ext = rng.uniform(0, 3, (n, 3)) * (rng.uniform(size=(n, 3)) < 0.8)       # some degenerate (flat) boxes
    lo, hi = (c - ext).astype(np.float32), (c + ext).astype(np.float32)
    p = (lo + (hi - lo) * rng.uniform(0, 1, (n, 3)).astype(np.float32)).astype(np.float32)
    p = np.minimum(np.maximum(p, lo), hi)
    k = rng.integers(0, 4, (n, 3))                               # points on the faces and corners too
    p = np.where(k == 0, lo, np.where(k == 1, hi, p))
    # queries: far, near, inside, and exactly on the faces
    q = (c + rng.normal(0, 1, (n, 3)) * rng.choice([0.5, 4.0, 60.0], (n, 1))).astype(np.float32)
    q = np.where(rng.integers(0, 6, (n, 3)) == 0, lo, q)
    bound, pair = np.zeros(n, np.float32), np.zeros(n, np.float32)
    hc.gc_bounds(n, _p(np.ascontiguousarray(lo)), _p(np.ascontiguousarray(hi)), _p(np.ascontiguousarray(q)), _p(bound))
    hc.gc_pairs(n, _p(np.ascontiguousarray(q)), _p(np.ascontiguousarray(p)), _p(pair))
    assert np.all(bound <= pair)
    assert (bound == pair).any() and (bound > 0).mean() > 0.3     # tight on the faces, and not trivially zero
    # the wave's query box: a bound below every query's own
    qext = rng.uniform(0, 2, (n, 3)).astype(np.float32)
    qlo, qhi = np.minimum(q, q - qext).astype(np.float32), np.maximum(q, q + qext).astype(np.float32)
    bb = np.zeros(n, np.float32)
    hc.gc_bounds_box(n, _p(np.ascontiguousarray(lo)), _p(np.ascontiguousarray(hi)), _p(np.ascontiguousarray(qlo)), _p(np.ascontiguousarray(qhi)), _p(bb))
    assert np.all(bb <= bound)
    # an inverted (empty) box: +inf against any query, above the initial best
    e = float(hc.gc_empty())
    lo_e, hi_e = np.full((4, 3), e, np.float32), np.full((4, 3), -e, np.float32)
    be = np.zeros(4, np.float32)
    hc.gc_bounds(4, _p(lo_e), _p(hi_e), _p(np.ascontiguousarray(q[:4])), _p(be))
    assert np.all(np.isinf(be)) and float(hc.gc_big()) < np.inf
    hc.gc_bounds_box(4, _p(lo_e), _p(hi_e), _p(np.ascontiguousarray(qlo[:4])), _p(np.ascontiguousarray(qhi[:4])), _p(be))
    assert np.all(np.isinf(be))
