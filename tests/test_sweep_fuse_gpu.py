"""TSDF fusion under the sweep model on the GPU: `integrate_sweep` of `liblrt_sweepfuse.so` EQUAL to its numpy twin, bit for bit, on the cases
of tests/sweep_fuse_cases.py and to `mesh.integrate` at zero motion; the launch counts, equal bits for equal inputs, a stream of the caller's, the
workspace and the inputs left alone, and the command line writing the PLY of the --device cpu run byte for byte."""
import filecmp
import os

import numpy as np
import pytest
import torch

from lidar_rt_amd import mesh, sweep_fuse as sf
from tests import mesh_cases as mcs
from tests import sweep_fuse_cases as sfc
from tests.test_mesh_gpu import same_bits, same_grid
from tests.test_place_gpu import launches
from tests.test_sweep_fuse import run_mesh

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


# ---- 1. the twin ----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", sfc.SIZES)
@pytest.mark.parametrize("conv", sfc.CONVENTIONS)
@pytest.mark.parametrize("dims", sfc.GRIDS)
def test_integrate_sweep_is_the_twin(dims, conv, size):
    H, W = size
    for mo_name in sfc.MOTIONS:
        for F in (0, 1, 3):
            want, _ = sfc.reference(dims, F, H, W, conv, mo_name)
            g = mcs.room_grid(dims, device=DEV)
            assert sf.integrate_sweep(g, **sfc.fuse_kw(mcs.room_frames(F, H, W, conv), sfc.motion(mo_name, W, F), DEV)) is None
            same_grid(g, want)
            if F == 3:
                assert int((want.weight == 0).sum()) > 0 or dims == (3, 5, 7)   # voxels that no frame sees


@pytest.mark.parametrize("conv", sfc.CONVENTIONS)
@pytest.mark.parametrize("dims", sfc.GRIDS)
def test_integrate_sweep_without_intensity_and_a_second_call(dims, conv):
    H, W = 8, 64
    for mo_name in sfc.MOTIONS:
        want, _ = sfc.reference(dims, 3, H, W, conv, mo_name, False)
        g = mcs.room_grid(dims, intensity=False, device=DEV)
        sf.integrate_sweep(g, **sfc.fuse_kw(mcs.room_frames(3, H, W, conv), sfc.motion(mo_name, W), DEV, intensity=False))
        same_grid(g, want)
        one, _ = sfc.reference(dims, 3, H, W, conv, mo_name)
        two, _ = sfc.reference(dims, 3, H, W, conv, mo_name, True, 2)
        g = one.to(DEV).clone()                                                 # pre-filled by an earlier call: what the second call does not see keeps its bits
        sf.integrate_sweep(g, **sfc.fuse_kw(mcs.room_frames(3, H, W, conv, 1), sfc.motion(mo_name, W), DEV))
        same_grid(g, two)
        kept = (two.weight == one.weight) & (one.weight > 0)
        assert int(kept.sum()) > 0 and same_bits(g.tsdf.cpu()[kept], one.tsdf[kept]) and same_bits(g.intensity.cpu()[kept], one.intensity[kept])
        g = mcs.room_grid(dims, device=DEV)
        for c in range(2):
            sf.integrate_sweep(g, **sfc.fuse_kw(mcs.room_frames(3, H, W, conv, c), sfc.motion(mo_name, W), DEV))
        same_grid(g, two)


@pytest.mark.parametrize("size", sfc.SIZES)
@pytest.mark.parametrize("conv", sfc.CONVENTIONS)
@pytest.mark.parametrize("dims", sfc.GRIDS)
def test_without_motion_the_operator_is_mesh_integrate(dims, conv, size):
    H, W = size
    fr = mcs.frames_to(mcs.room_frames(3, H, W, conv), DEV)
    static = mcs.room_grid(dims, device=DEV)
    mesh.integrate(static, **fr)
    assert int((static.weight > 0).sum()) > 0
    for twist in (None, np.zeros((3, 6)), np.zeros(6)):
        g = mcs.room_grid(dims, device=DEV)
        sf.integrate_sweep(g, twist=twist, **fr)
        same_grid(g, static.to("cpu"))


# ---- 2. launches, determinism, streams ----------------------------------------------------------------------------------------------------------------------

def test_launch_counts():
    fr = mcs.room_frames(3, 16, 128, "kitti_bounds")
    counts = {}
    for key, twist in (("moving", sfc.motion("moderate_cw", 128)["twist"]), ("static", None)):
        g = mcs.room_grid((17, 19, 23), device=DEV)
        kw = dict(mcs.frames_to(fr, DEV), twist=twist)
        ev = launches(lambda: sf.integrate_sweep(g, **kw))
        assert len(ev) == 2 and any("k_sf_table" in k for k in ev) and any("k_sf_fuse" in k for k in ev), ev
        counts[key] = sum(ev.values())
    g = mcs.room_grid((17, 19, 23), device=DEV)
    kw0 = sfc.fuse_kw(mcs.room_frames(0, 16, 128, "kitti_bounds"), sfc.motion("moderate_cw", 128, 0), DEV)
    counts["no_frames"] = sum(launches(lambda: sf.integrate_sweep(g, **kw0)).values())
    print(counts)
    assert counts == {"moving": 2, "static": 2, "no_frames": 0}


def test_a_second_call_returns_the_same_bits():
    kw = sfc.fuse_kw(mcs.room_frames(3, 16, 128, "waymo_table"), sfc.motion("strong_ccw", 128), DEV)
    a, b = mcs.room_grid((17, 19, 23), device=DEV), mcs.room_grid((17, 19, 23), device=DEV)
    sf.integrate_sweep(a, **kw)
    held = [torch.full((1 << 20,), 0xAB, dtype=torch.uint8, device=DEV) for _ in range(2)]          # dirty memory for the next workspace to land in
    del held
    sf.integrate_sweep(b, **kw)
    same_grid(a, b.to("cpu"))
    assert int((a.weight > 0).sum()) > 0


def test_a_stream_of_the_callers_orders_against_the_torch_ops_around_it():
    want, _ = sfc.reference((17, 19, 23), 3, 16, 128, "kitti_bounds", "moderate_cw")
    kw = sfc.fuse_kw(mcs.room_frames(3, 16, 128, "kitti_bounds"), sfc.motion("moderate_cw", 128), DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        big = torch.randn(4096, 4096, device=DEV)
        for _ in range(4):
            big = big @ big * 1e-3                                                                      # work in front of the call, on the same stream
        depth = kw["depth"] + 0.0 * big[0, 0].nan_to_num(0.0, 0.0, 0.0)                                 # the input is made by a torch op of that stream
        g = mcs.room_grid((17, 19, 23), device=DEV)
        sf.integrate_sweep(g, **dict(kw, depth=depth))
        after = (g.tsdf * 1.0, g.weight + 0)                                                            # torch ops that follow on the stream
    side.synchronize()
    same_grid(g, want)
    assert same_bits(after[0], want.tsdf) and same_bits(after[1], want.weight)


# ---- 3. the workspace and the inputs ------------------------------------------------------------------------------------------------------------------------

def test_the_workspace_may_hold_anything_and_nothing_behind_it_is_written():
    dims, (H, W), conv = (17, 19, 23), (5, 37), "waymo_table"
    want, _ = sfc.reference(dims, 3, H, W, conv, "table")
    n = sf.work_bytes(3, W)
    assert n == 10752 and n > 3 * W * 96                                        # rounded up: the table ends inside the last 256 bytes
    buf = torch.full((n + 4096,), 0xFF, dtype=torch.uint8, device=DEV)          # all-ones bytes: NaN entries, should a stale one ever be read
    g = mcs.room_grid(dims, device=DEV)
    sf.integrate_sweep(g, workspace=buf[:n], **sfc.fuse_kw(mcs.room_frames(3, H, W, conv), sfc.motion("table", W), DEV))
    same_grid(g, want)
    assert bool((buf[n:] == 0xFF).all()) and bool((buf[3 * W * 96:n] == 0xFF).all()) and not bool((buf[:3 * W * 96] == 0xFF).all())
    with pytest.raises(mesh.MeshError, match="workspace"):
        sf.integrate_sweep(g, workspace=buf[:n - 1], **sfc.fuse_kw(mcs.room_frames(3, H, W, conv), sfc.motion("table", W), DEV))
    with pytest.raises(mesh.MeshError, match="workspace"):
        sf.integrate_sweep(g, workspace=buf[8:n + 8], **sfc.fuse_kw(mcs.room_frames(3, H, W, conv), sfc.motion("table", W), DEV))


def test_the_inputs_are_not_changed_and_a_twist_on_the_device_is_refused():
    dims, (H, W), conv = (17, 19, 23), (8, 64), "kitti_bounds"
    mo = sfc.motion("table", W)
    kw = sfc.fuse_kw(mcs.room_frames(3, H, W, conv), mo, DEV)
    held = {k: (v.clone() if torch.is_tensor(v) else np.array(v, copy=True)) for k, v in kw.items() if torch.is_tensor(v) or isinstance(v, np.ndarray)}
    assert {"depth", "mask", "intensity", "sensor2world", "twist", "tau"} <= set(held)
    g = mcs.room_grid(dims, device=DEV)
    sf.integrate_sweep(g, **kw)
    torch.cuda.synchronize()
    for k, v in held.items():
        assert (torch.equal(kw[k], v) if torch.is_tensor(v) else np.array_equal(kw[k], v)), k
    with pytest.raises(mesh.MeshError, match="host data"):
        sf.integrate_sweep(g, **dict(kw, twist=torch.zeros(3, 6, dtype=torch.float64, device=DEV)))
    with pytest.raises(mesh.MeshError, match="host data"):
        sf.integrate_sweep(g, **dict(kw, tau=torch.zeros(W, dtype=torch.float64, device=DEV)))


# ---- 4. the command line ------------------------------------------------------------------------------------------------------------------------------------

def test_mesh_sweep_stored_on_the_gpu_writes_the_cpu_runs_ply(tmp_path):
    root = sfc.write_sweep_sequence(str(tmp_path / "seq"))
    cpu = run_mesh(root, str(tmp_path / "cpu"), "cpu", ["--sweep", "stored"])
    sfc.check_sequence_margins(root, str(tmp_path / "cpu"))                      # the two margins over every fused frame
    gpu = run_mesh(root, str(tmp_path / "gpu"), "cuda", ["--sweep", "stored"])
    assert os.path.getsize(gpu) > 10000
    assert filecmp.cmp(cpu, gpu, shallow=False)
