"""The reference's own Chamfer and simple-knn kernels, built for gfx950 by oracle/ref_build.py, against the CPU oracle: bit for bit.

Two builds of each module run here.  The build with -ffp-contract=off is IEEE arithmetic as the source is written, so it must
equal oracle variant 2 (no contraction) with no tolerance.  The build with the compiler's default contraction must equal ONE
variant on every case.  Measured on the MI355X: it equals none of the three variants the oracle had (0, 1, 2: on 2000 x 3000 random
points 233 / 501 / 199 of 2000 dist1 values differ, knn on 5000 points 475 / 898 / 373), because hipcc pairs dy*dy and dz*dz in
one packed multiply and fuses only the first addition.  The oracle therefore lists all six contractions of (dx*dx + dy*dy) + dz*dz
that need no re-association, and the default build equals variant 4, fmaf(dy,dy, dx*dx) + dz*dz, for both operators on every
case (DEFAULT_VARIANT).  Which contraction nvcc applies in the reference's CUDA binary is not observable here; the oracle's
variant 0, which the product follows, remains an assumption.

The whole file skips only when oracle/_ref/manifest.json does not exist (no reference tree at build time).  With a manifest, a
module that does not import is a failure.
"""
import functools
import os

import numpy as np
import pytest
import torch

from lidar_rt_amd import scenes
from oracle import chamfer as och
from oracle import ref_build
from tests import chamfer_nonfinite_cases as nf
from tests.test_chamfer_gpu import lidar_clouds

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not os.path.exists(ref_build.MANIFEST),
                                 reason="oracle/_ref/manifest.json does not exist: the reference binaries were not built (no reference tree)")]
DEV = torch.device("cuda:0")
DEFAULT_VARIANT = 4                                         # the oracle variant hipcc's default contraction produces (measured)
BUILDS = [("off", 2), ("default", DEFAULT_VARIANT)]         # (build of the reference module, oracle variant it must equal)


@functools.lru_cache(maxsize=None)
def ref_module(name, build):
    return ref_build.load(name, build)                      # an import error is an error, not a skip


def ref_chamfer(a, b, build):
    m = ref_module("ref_chamfer_3D", build)
    ta, tb = torch.as_tensor(a, device=DEV), torch.as_tensor(b, device=DEV)
    B, N, M = a.shape[0], a.shape[1], b.shape[1]
    d1 = torch.full((B, N), -1.0, device=DEV); d2 = torch.full((B, M), -1.0, device=DEV)
    i1 = torch.full((B, N), -7, device=DEV, dtype=torch.int32); i2 = torch.full((B, M), -7, device=DEV, dtype=torch.int32)
    assert m.forward(ta, tb, d1, d2, i1, i2) == 1
    torch.cuda.synchronize()
    return d1.cpu().numpy(), d2.cpu().numpy(), i1.cpu().numpy(), i2.cpu().numpy()


def ref_knn(p, build):
    out = ref_module("ref_simple_knn", build).distCUDA2(torch.as_tensor(p, device=DEV))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def assert_same(got, want, what):
    """Equal bits for floats (a NaN equals a NaN of any payload), equal values for indices."""
    for g, w, name in zip(got, want, ("dist1", "dist2", "idx1", "idx2")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        if g.dtype == np.float32:
            nan = np.isnan(w)
            assert np.array_equal(np.isnan(g), nan), f"{what} {name}: NaN at different places"
            bad = (g.view(np.int32) != w.view(np.int32)) & ~nan
        else:
            bad = g != w
        assert not bad.any(), f"{what} {name}: {bad.sum()} of {g.size} differ, first at {np.argwhere(bad)[0]}"


def check_chamfer(a, b, what):
    for build, variant in BUILDS:
        assert_same(ref_chamfer(a, b, build), och.chamfer_forward(a, b, variant), f"{what} [{build} build vs variant {variant}]")


# each shape is the smallest that reaches a distinct path of NmDistanceKernel
@pytest.mark.parametrize("B,N,M", [(1, 1, 1),              # smallest case
                                   (1, 5, 3),              # fewer than 4 candidates: only the tail loop, seeded there
                                   (1, 7, 511),            # just under one tile
                                   (1, 9, 512),            # the `end_ka==batch` branch alone
                                   (1, 9, 513),            # a second tile of one candidate
                                   (1, 600, 1027),         # a last tile of 3
                                   (1, 8193, 700),         # more queries than one grid pass of 16 x 512 threads
                                   (33, 17, 70),           # more batches than gridDim.x = 32
                                   (2, 513, 4097)])        # a mixed case
def test_chamfer_reference_equals_oracle_random(B, N, M):
    r = np.random.default_rng(1000 + 7 * N + M)
    a = (r.standard_normal((B, N, 3)) * 20).astype(np.float32); b = (r.standard_normal((B, M, 3)) * 20).astype(np.float32)
    check_chamfer(a, b, f"random ({B},{N},{M})")


def test_chamfer_reference_equals_oracle_lattice_ties_across_tiles():
    """Thousands of exact ties and duplicates with M > 1024: the first minimum wins across tile borders."""
    r = np.random.default_rng(3)
    b = r.integers(-5, 6, (1, 2500, 3)).astype(np.float32)
    a = r.integers(-5, 6, (1, 1500, 3)).astype(np.float32) + np.float32(0.5)
    check_chamfer(a, b, "lattice")
    w = och.chamfer_forward(a, b, 2)
    D = ((a[0, :, None] - b[0, None]) ** 2).sum(-1)           # exact in float32
    assert ((D == D.min(1, keepdims=True)).sum(1) > 1).sum() > 1000 and len(np.unique(w[2] // 512)) > 1
    check_chamfer(b, b.copy(), "both clouds equal")


def test_chamfer_reference_equals_oracle_lidar_pair():
    a, b = lidar_clouds(16, 512, 8)
    check_chamfer(a, b, "lidar")


def test_chamfer_reference_equals_oracle_non_finite():
    """NaN at candidate 0, at candidate 512 of 1100, mid-tile, a NaN query, +-inf without NaN, every candidate non-finite."""
    for name, (a, b) in nf.nonfinite_cases(300, 1100).items():
        check_chamfer(a, b, name)


@pytest.mark.parametrize("build", ["off", "default"])
def test_chamfer_reference_backward_matches_float64_and_accumulates(build):
    a, b = lidar_clouds(16, 512, 2)
    r = np.random.default_rng(4)
    N, M = a.shape[1], b.shape[1]
    g1 = r.standard_normal((1, N)).astype(np.float32); g2 = r.standard_normal((1, M)).astype(np.float32)
    _, _, i1, i2 = och.chamfer_forward(a, b)
    wa, wb = och.chamfer_backward(a, b, g1, g2, i1, i2, "f64")
    t = lambda x: torch.as_tensor(x, device=DEV)
    m = ref_module("ref_chamfer_3D", build)
    ga = torch.zeros(1, N, 3, device=DEV); gb = torch.zeros(1, M, 3, device=DEV)
    assert m.backward(t(a), t(b), ga, gb, t(g1), t(g2), t(i1), t(i2)) == 1
    scale = max(np.abs(wa).max(), np.abs(wb).max())
    np.testing.assert_allclose(ga.cpu().numpy(), wa, rtol=1e-5, atol=1e-5 * scale)
    np.testing.assert_allclose(gb.cpu().numpy(), wb, rtol=1e-5, atol=1e-5 * scale)
    assert m.backward(t(a), t(b), ga, gb, t(g1), t(g2), t(i1), t(i2)) == 1        # a second call adds, as the reference binding does
    np.testing.assert_allclose(ga.cpu().numpy(), 2 * wa, rtol=1e-5, atol=2e-5 * scale)
    np.testing.assert_allclose(gb.cpu().numpy(), 2 * wb, rtol=1e-5, atol=2e-5 * scale)


def check_knn(p, what):
    for build, variant in BUILDS:
        got, want = ref_knn(p, build), och.knn_mean_dist2(p, variant)
        assert_same((got,), (want,), f"knn {what} [{build} build vs variant {variant}]")


# the reference's box is 1024 points and its neighbour window +-3; P = 0 would launch an empty grid and is not sent
@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 8, 1023, 1024, 1025, 2049, 5000])
def test_knn_reference_equals_oracle_random(P):
    check_knn((np.random.default_rng(10 + P).standard_normal((P, 3)) * 10).astype(np.float32), f"random P={P}")


def test_knn_reference_equals_oracle_duplicates_lattice_lidar():
    r = np.random.default_rng(2)
    check_knn(np.repeat((r.standard_normal((50, 3)) * 10).astype(np.float32), 4, 0), "np.repeat duplicates")
    check_knn(np.random.default_rng(0).integers(-3, 4, (400, 3)).astype(np.float32), "lattice")
    _, d = scenes.kitti_rays(16, 512)
    pts = (d.reshape(-1, 3) * (5.0 + 40.0 * r.random(16 * 512) ** 2)[:, None]).astype(np.float32)
    check_knn(np.concatenate([pts, pts[r.integers(0, len(pts), 800)]], 0), "16 x 512 lidar cloud with duplicates")


def test_knn_reference_equals_oracle_with_a_nan_and_an_inf_point():
    """The finite points' results and the non-finite points' own results equal the oracle's."""
    p = nf.knn_nonfinite_cloud(3000, 7)
    check_knn(p, "one NaN and one +inf point in 3000")
    for build, _ in BUILDS:
        got = ref_knn(p, build)
        assert np.isinf(got[[1000, 2000]]).all() and np.isfinite(np.delete(got, [1000, 2000])).all()
