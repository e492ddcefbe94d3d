"""The surface meshes on the GPU: `integrate` and `extract` of `liblrt_mesh.so` EQUAL to their numpy twins, bit for bit, on the cases of
tests/mesh_cases.py; the launch counts, equal bits for equal inputs, a stream of the caller's, and the command line writing the PLY of the
--device cpu run byte for byte."""
import filecmp
import functools
import os

import numpy as np
import pytest
import torch

from lidar_rt_amd import mesh
from tests import mesh_cases as mcs
from tests.test_mesh import run_cli, write_room_sequence
from tests.test_place_gpu import launches

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def same_bits(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


def same_grid(g, w):
    assert same_bits(g.tsdf, w.tsdf), int((g.tsdf.cpu().view(torch.int32) != w.tsdf.view(torch.int32)).sum())
    assert same_bits(g.weight, w.weight)
    assert (g.intensity is None) == (w.intensity is None)
    if w.intensity is not None:
        assert same_bits(g.intensity, w.intensity)


def same_mesh(m, w):
    assert same_bits(m.vertices, w.vertices), (tuple(m.vertices.shape), tuple(w.vertices.shape))
    assert same_bits(m.faces, w.faces), (tuple(m.faces.shape), tuple(w.faces.shape))
    assert (m.intensity is None) == (w.intensity is None)
    if w.intensity is not None:
        assert same_bits(m.intensity, w.intensity)
    assert np.array_equal(m.origin, w.origin)


# ---- 1. integrate -------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", mcs.SIZES)
@pytest.mark.parametrize("conv", mcs.CONVENTIONS)
@pytest.mark.parametrize("dims", list(mcs.GRIDS))
def test_integrate_is_the_twin(dims, conv, size):
    H, W = size
    for F in (0, 1, 3):
        want, margin = mcs.room_reference(dims, F, H, W, conv)
        assert margin >= mcs.MARGIN
        g = mcs.room_grid(dims, device=DEV)
        assert mesh.integrate(g, **mcs.frames_to(mcs.room_frames(F, H, W, conv), DEV)) is None
        same_grid(g, want)
        if F == 3:
            assert int((want.weight == 0).sum()) > 0 or dims == (3, 5, 7)       # voxels that no frame sees (all of 3 x 5 x 7 is seen by some frames)


@pytest.mark.parametrize("conv", mcs.CONVENTIONS)
@pytest.mark.parametrize("dims", list(mcs.GRIDS))
def test_integrate_without_intensity_and_a_second_call(dims, conv):
    H, W = 8, 64
    want, margin = mcs.room_reference(dims, 3, H, W, conv, False)
    assert margin >= mcs.MARGIN
    g = mcs.room_grid(dims, intensity=False, device=DEV)
    mesh.integrate(g, **mcs.frames_to(mcs.room_frames(3, H, W, conv), DEV, intensity=False))
    same_grid(g, want)
    want2, margin2 = mcs.room_reference(dims, 3, H, W, conv, True, 2)
    assert margin2 >= mcs.MARGIN
    g = mcs.room_grid(dims, device=DEV)
    for c in range(2):
        mesh.integrate(g, **mcs.frames_to(mcs.room_frames(3, H, W, conv, c), DEV))
    same_grid(g, want2)


def test_integrate_the_sphere():
    want, margin = mcs.sphere_reference()
    assert margin >= mcs.MARGIN
    g = mcs.sphere_grid(DEV)
    mesh.integrate(g, **mcs.frames_to(mcs.sphere_frames(), DEV))
    same_grid(g, want)


# ---- 2. extract ---------------------------------------------------------------------------------------------------------------------------------------------

def extract_cases():
    """{name: (CPU grid, min_weight)}, built once on first use."""
    cases = []
    for seed, dims in ((0, (1, 5, 6)), (1, (2, 7, 3)), (2, (5, 2, 9)), (3, (2, 2, 2)), (4, (6, 1, 1))):
        cases.append((f"thin{dims}", mcs.random_grid(seed, dims, border=False), 1))
    for seed in mcs.SEEDS:
        cases.append((f"random{seed}", mcs.random_grid(seed), 1))
    pos = mcs.random_grid(0)
    pos.tsdf.abs_()
    cases.append(("all_positive", pos, 1))
    unobs = mcs.random_grid(1)
    unobs.weight.zero_()
    cases.append(("all_unobserved", unobs, 1))
    w = mcs.random_grid(2, border=False)
    w.weight[:] = torch.from_numpy(np.random.default_rng(9).integers(0, 4, w.dims).astype(np.int32))
    cases.append(("weights_0_to_3", w, 2))
    cases.append(("sphere", mcs.sphere_reference()[0], 1))
    for conv in mcs.CONVENTIONS:
        cases.append((f"room_{conv}", mcs.room_reference((17, 19, 23), 3, 16, 128, conv)[0], 1))
    # 41^3 = 68921 voxels: 270 workgroups of the count, more than one pass (256) of the scan
    cases.append(("more_than_one_scan_pass", mcs.random_grid(5, (41, 41, 41)), 1))
    return {n: (g, mw) for n, g, mw in cases}


CASE_NAMES = ([f"thin{d}" for d in ((1, 5, 6), (2, 7, 3), (5, 2, 9), (2, 2, 2), (6, 1, 1))] + [f"random{s}" for s in mcs.SEEDS]
              + ["all_positive", "all_unobserved", "weights_0_to_3", "sphere"] + [f"room_{c}" for c in mcs.CONVENTIONS] + ["more_than_one_scan_pass"])


@functools.lru_cache(maxsize=None)
def _cases():
    cases = extract_cases()
    assert sorted(cases) == sorted(CASE_NAMES)
    return cases


@pytest.mark.parametrize("name", CASE_NAMES)
def test_extract_is_the_twin(name):
    grid, mw = _cases()[name]
    want = mesh.extract_reference(grid, mw)
    got = mesh.extract(grid.to(DEV), mw)
    same_mesh(got, want)
    if name in ("all_positive", "all_unobserved"):
        assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3)
    if name == "more_than_one_scan_pass":
        assert -(-grid.tsdf.numel() // mesh.BLOCK) > mesh.SCAN_PASS and want.faces.shape[0] > 0


def test_extract_without_intensity():
    g = mcs.random_grid(3, intensity=False)
    got = mesh.extract(g.to(DEV))
    same_mesh(got, mesh.extract_reference(g))


# ---- 3. launches, determinism, streams ----------------------------------------------------------------------------------------------------------------------

def test_launch_counts():
    fr = mcs.frames_to(mcs.room_frames(3, 16, 128, "kitti_bounds"), DEV)
    counts = {}
    for key, mask in (("seeded", fr["mask"]), ("empty", torch.zeros_like(fr["mask"])), ("full", torch.ones_like(fr["mask"]))):
        g = mcs.room_grid((17, 19, 23), device=DEV)
        ev = launches(lambda: mesh.integrate(g, **dict(fr, mask=mask)))
        assert all("k_mesh_" in k for k in ev), ev
        counts[("integrate", key)] = sum(ev.values())
        ev = launches(lambda: mesh.extract(g))
        assert all("k_mesh_" in k for k in ev), ev
        counts[("extract", key)] = sum(ev.values())
    print(counts)
    assert all(v == 1 for (op, _), v in counts.items() if op == "integrate")
    assert all(v <= 4 for (op, _), v in counts.items() if op == "extract")


def test_a_second_call_returns_the_same_bits():
    fr = mcs.frames_to(mcs.room_frames(3, 16, 128, "waymo_table"), DEV)
    a, b = mcs.room_grid((17, 19, 23), device=DEV), mcs.room_grid((17, 19, 23), device=DEV)
    mesh.integrate(a, **fr)
    held = [torch.full((1 << 20,), 0xAB, dtype=torch.uint8, device=DEV) for _ in range(2)]          # dirty memory for the next outputs to land in
    del held
    mesh.integrate(b, **fr)
    same_grid(a, b)
    m1, m2 = mesh.extract(a), mesh.extract(b)
    same_mesh(m1, m2)
    assert m1.faces.shape[0] > 0


def test_a_stream_of_the_callers_orders_against_the_torch_ops_around_it():
    want, _ = mcs.room_reference((17, 19, 23), 3, 16, 128, "kitti_bounds")
    wmesh = mesh.extract_reference(want)
    fr = mcs.frames_to(mcs.room_frames(3, 16, 128, "kitti_bounds"), DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        big = torch.randn(4096, 4096, device=DEV)
        for _ in range(4):
            big = big @ big * 1e-3                                                                      # work in front of the call, on the same stream
        depth = fr["depth"] + 0.0 * big[0, 0].nan_to_num(0.0, 0.0, 0.0)                                 # the input is made by a torch op of that stream
        g = mcs.room_grid((17, 19, 23), device=DEV)
        mesh.integrate(g, **dict(fr, depth=depth))
        m = mesh.extract(g)
        after = (m.vertices * 1.0, m.faces + 0)                                                         # torch ops that follow on the stream
    side.synchronize()
    same_grid(g, want)
    same_mesh(m, wmesh)
    assert same_bits(after[0], wmesh.vertices) and same_bits(after[1], wmesh.faces)


# ---- 4. the command line ------------------------------------------------------------------------------------------------------------------------------------

def test_the_command_line_on_the_gpu_writes_the_cpu_runs_ply(tmp_path):
    root = write_room_sequence(str(tmp_path / "seq"))
    cpu = run_cli(root, str(tmp_path / "cpu"), "cpu")
    gpu = run_cli(root, str(tmp_path / "gpu"), "cuda")
    assert os.path.getsize(gpu) > 10000
    assert filecmp.cmp(cpu, gpu, shallow=False)
