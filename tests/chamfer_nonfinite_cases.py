"""Clouds with non-finite coordinates for the Chamfer and knn tests (tests/test_chamfer_oracle.py, tests/test_chamfer_gpu.py,
tests/test_knn.py, tests/test_reference_pin_gpu.py), and the float32 pair distance of the oracle in NumPy.

Every case is a pair xyz1 (1,N,3), xyz2 (1,M,3).  Both directions are searched, so a non-finite candidate of one direction is a
non-finite query of the other.
"""
from __future__ import annotations

import numpy as np

NAN, INF = np.float32(np.nan), np.float32(np.inf)
TILE = 512                                                  # the reference scans candidates in tiles of 512 (chamfer3D.cu:12)


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays: the float64 product is exact, the float64 sum is rounded to odd (from TwoSum's exact error)
    so that the final rounding to float32 is the single rounding of a fused multiply-add."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c64 = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c64
        t = s - p
        err = (p - (s - t)) + (c64 - t)
        inexact = np.isfinite(s) & np.isfinite(err) & (err != 0)
        odd = np.where(inexact & ((s.view(np.int64) & 1) == 0), np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return odd.astype(np.float32)


def pair_d2(q, c, variant=0):
    """(N,3), (M,3) float32 -> (N,M) float32 squared distances, d = candidate - query, as the oracle's d2_v0 .. d2_v5."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = c[None, :, :] - q[:, None, :]
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        if variant == 0:
            return fma32(dz, dz, fma32(dy, dy, dx * dx))
        if variant == 1:
            return fma32(dz, dz, fma32(dx, dx, dy * dy))
        if variant == 2:
            return (dx * dx + dy * dy) + dz * dz
        if variant == 3:
            return fma32(dx, dx, dy * dy) + dz * dz
        if variant == 4:
            return fma32(dy, dy, dx * dx) + dz * dz
        return fma32(dz, dz, dx * dx + dy * dy)


def finite_pair(N, M, seed, scale=20.0):
    r = np.random.default_rng(seed)
    return (r.standard_normal((1, N, 3)) * scale).astype(np.float32), (r.standard_normal((1, M, 3)) * scale).astype(np.float32)


def nonfinite_cases(N, M, seed=0):
    """name -> (xyz1, xyz2).  Candidate positions are those of a 1100-point cloud (0, 512, mid-tile 700 and 100), clipped to M."""
    out = {}

    def case(name, fn):
        a, b = finite_pair(N, M, seed + len(out))
        fn(a[0], b[0])
        out[name] = (a, b)

    c512, mid = min(TILE, M - 1), min(700, M // 3)
    case("nan_candidate_0", lambda a, b: b.__setitem__((0, 1), NAN))
    case("nan_candidate_512", lambda a, b: b.__setitem__((c512, 0), NAN))
    case("nan_mid_tile", lambda a, b: (b.__setitem__((mid, 2), NAN), b.__setitem__((min(100, M - 2), slice(None)), NAN)))
    case("nan_query", lambda a, b: a.__setitem__((min(5, N - 1), 2), NAN))

    def inf_only(a, b):                                     # no NaN coordinate and no inf - inf: the infinities of one axis differ in sign
        b[0, 0] = INF; b[min(7, M - 1), 1] = -INF; b[c512, 0] = INF; b[M - 1, 2] = INF
        a[min(3, N - 1), 0] = -INF; a[N - 1, 2] = -INF
    case("inf_only", inf_only)
    case("inf_only_one_cloud", lambda a, b: (b.__setitem__((0, 2), -INF), b.__setitem__((mid, 0), INF), b.__setitem__((c512, 1), INF)))

    def all_nonfinite_inf0(a, b):
        b[0::2, 0] = INF; b[1::2, 1] = NAN
    case("all_nonfinite_inf_first", all_nonfinite_inf0)

    def all_nonfinite_nan0(a, b):
        b[0::2, 2] = NAN; b[1::2, 0] = -INF
    case("all_nonfinite_nan_first", all_nonfinite_nan0)
    return out


INF_ONLY = ("inf_only", "inf_only_one_cloud")              # the cases without any NaN distance


def knn_nonfinite_cloud(P, seed=0, scale=10.0):
    """A random cloud with one NaN point (index P // 3) and one +inf point (index 2 * P // 3)."""
    p = (np.random.default_rng(seed).standard_normal((P, 3)) * scale).astype(np.float32)
    p[P // 3, 1] = NAN
    p[2 * P // 3, 0] = INF
    return p
