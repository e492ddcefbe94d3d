"""The range-image projection on the GPU (`liblrt_project.so` through `lidar_rt_amd.range_image`): depth, intensity, mask, index and counts against
the float64 twin bit for bit on the cases of tests/range_image_cases.py (every one keeps its points off the rounding boundaries), the heaviest
contention on one word, a dirty workspace, equal bits for equal inputs and for any arrival order, the refused calls, no host wait inside a call,
and the ingest of point clouds on the device against the CPU path byte for byte."""
import os

import numpy as np
import pytest
import torch

from lidar_rt_amd import ingest, range_image as ri
from tests import range_image_cases as rc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
POINTS = [1, 63, 64, 65, 255, 256, 257, 1000, 70_000]          # around a wave, around a workgroup, several workgroups, many
ALL_SIZES = rc.SIZES + [(66, 1030)]


def bits(t):
    t = t.detach().contiguous()
    return (t.view(torch.int32) if t.dtype == torch.float32 else t).cpu()


def run(c, **over):
    pts = torch.tensor(c.points, device=DEV)
    keep = pts.clone()
    op = ri.project_points(pts, **{**c.kw, **over})
    torch.cuda.synchronize()
    assert torch.equal(bits(pts), bits(keep)), "the points changed"
    return op


def same(op, tw, label=""):
    assert op.depth.dtype == torch.float32 and op.intensity.dtype == torch.float32 and op.mask.dtype == torch.bool and op.index.dtype == torch.int32 \
        and op.counts.dtype == torch.int64, label
    assert op.depth.shape == tw.depth.shape and op.counts.shape == tw.counts.shape, label
    assert torch.equal(op.counts.cpu(), tw.counts), (label, op.counts.tolist(), tw.counts.tolist())
    assert torch.equal(op.mask.cpu(), tw.mask), label
    assert torch.equal(op.index.cpu(), tw.index), label
    assert torch.equal(bits(op.depth), bits(tw.depth)), label
    assert torch.equal(bits(op.intensity), bits(tw.intensity)), label


# ---- 1. the operator against the twin -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("N", POINTS)
def test_point_counts_and_ragged_frames_against_the_twin(N, F):
    c = rc.random_cloud(N, F, 8, 64, "kitti_bounds", 11)
    same(run(c), c.twin, f"N {N} F {F}")


@pytest.mark.parametrize("wrap,transform", [(True, False), (False, True), (True, True)], ids=["wrap", "no_wrap_transform", "wrap_transform"])
@pytest.mark.parametrize("conv", rc.CONVENTIONS)
@pytest.mark.parametrize("H,W", ALL_SIZES)
def test_image_sizes_conventions_wrap_and_transform_against_the_twin(H, W, conv, wrap, transform):
    c = rc.random_cloud(1000, 3, H, W, conv, 21, wrap=wrap, transform=transform)
    same(run(c), c.twin, f"{H} x {W} {conv} wrap {wrap} transform {transform}")
    cnt = c.twin.counts
    assert int(cnt[:, 5].sum()) > 0 and int(cnt[:, 3].sum()) > 0 and cnt[1].tolist() == [0] * 6


def test_seventy_thousand_points_into_66_x_1030_in_three_frames_with_transforms():
    c = rc.random_cloud(70_000, 3, 66, 1030, "waymo_table_yaw", 22, transform=True)
    same(run(c), c.twin, "70 000 points 66 x 1030")
    assert int(c.twin.counts[:, 4].sum()) > 1000 and int(c.twin.counts[:, 5].sum()) > 10_000


@pytest.mark.parametrize("posed", [False, True], ids=["sensor_frame", "posed"])
@pytest.mark.parametrize("conv", rc.CONVENTIONS)
@pytest.mark.parametrize("H,W", ALL_SIZES)
def test_the_round_trip_on_the_ray_grid(H, W, conv, posed):
    c = rc.grid(H, W, conv, 13, posed=posed)
    op = run(c)
    same(op, c.twin, f"grid {H} x {W} {conv}")
    assert torch.equal(op.index.reshape(-1).cpu(), torch.arange(H * W, dtype=torch.int32)) and bool(op.mask.all())


@pytest.mark.parametrize("wrap", [True, False], ids=["wrap", "no_wrap"])
@pytest.mark.parametrize("mode", ["bounds", "table"])
def test_constructed_points(mode, wrap):
    c = rc.constructed(mode, wrap)
    same(run(c), c.twin, f"constructed {mode} wrap {wrap}")


def test_three_columns_and_no_points():
    c = rc.random_cloud(1000, 1, 8, 64, "kitti_bounds", 11)
    op = ri.project_points(torch.tensor(c.points[:, :3], device=DEV), **c.kw)              # (N, 3): the intensity is 0
    tw = ri.project_points_reference(c.points[:, :3], **c.kw)
    same(op, tw, "(N, 3)")
    assert float(op.intensity.abs().sum()) == 0.0 and torch.equal(bits(op.depth), bits(c.twin.depth))
    empty = ri.project_points(torch.zeros((0, 4), device=DEV), 5, 37, list(rc.KITTI_INC), offsets=[0, 0, 0])
    same(empty, ri.project_points_reference(np.zeros((0, 4), np.float32), 5, 37, list(rc.KITTI_INC), offsets=[0, 0, 0]), "no points")
    assert empty.counts.tolist() == [[0] * 6] * 2 and not bool(empty.mask.any()) and bool((empty.index == -1).all())


# ---- 2. contention on one word ----------------------------------------------------------------------------------------------------------------------------------

def test_everything_into_one_pixel_and_equal_ranges():
    c = rc.one_ray(1000)
    op = run(c)
    same(op, c.twin, "1000 points on one ray")
    assert op.counts.tolist() == [1000, 0, 0, 0, 999, 1] and int(op.index[3, 20]) == int(np.argmin(c.ranges))
    e = rc.one_ray(300, equal=True)
    op = run(e)
    same(op, e.twin, "300 equal ranges")
    assert op.counts.tolist() == [300, 0, 0, 0, 299, 1] and int(op.index[3, 20]) == 0


# ---- 3. a dirty workspace, repeated calls, the arrival order ------------------------------------------------------------------------------------------------------

def test_a_dirty_workspace_does_not_leak_and_equal_inputs_give_equal_bits():
    big = rc.random_cloud(70_000, 1, 8, 64, "kitti_bounds", 11)
    small = rc.random_cloud(63, 1, 8, 64, "kitti_bounds", 11)
    ws = torch.zeros(ri.work_bytes(1, 8, 64) + 512, dtype=torch.uint8, device=DEV)          # zeros: the SMALLEST key everywhere, were it read
    same(run(big, workspace=ws), big.twin, "large cloud, zeroed workspace")
    first = run(small, workspace=ws)
    same(first, small.twin, "small cloud on the large cloud's workspace")
    assert int(small.twin.counts[5]) < int(big.twin.counts[5])
    for _ in range(3):
        again = run(small, workspace=ws)
        for a, b in zip(again, first):
            assert torch.equal(bits(a), bits(b))
    fresh = run(small)
    for a, b in zip(fresh, first):
        assert torch.equal(bits(a), bits(b))


def test_a_permuted_point_order_gives_what_the_twin_gives_on_it():
    c = rc.random_cloud(70_000, 1, 8, 64, "kitti_bounds", 11)
    perm = np.random.default_rng(4).permutation(c.points.shape[0])
    pts = np.ascontiguousarray(c.points[perm])
    tw = ri.project_points_reference(pts, **c.kw)
    assert tw.margin >= rc.MARGIN
    op = ri.project_points(torch.tensor(pts, device=DEV), **c.kw)
    same(op, tw, "permuted")
    # the image is that of the original order wherever no two winners tie; the index follows the permutation
    assert torch.equal(bits(op.depth), bits(c.twin.depth)) and torch.equal(op.counts.cpu(), c.twin.counts)
    m = c.twin.mask
    assert np.array_equal(perm[op.index.cpu().numpy()[m.numpy()]], c.twin.index.numpy()[m.numpy()])


# ---- 4. inputs and refusals -----------------------------------------------------------------------------------------------------------------------------------------

def test_refused_calls_raise_and_launch_nothing():
    c = rc.random_cloud(1000, 3, 8, 64, "waymo_table_yaw", 21)
    pts = torch.tensor(c.points, device=DEV)
    kw = dict(c.kw)
    ws = torch.full((ri.work_bytes(3, 8, 64),), 0x5A, dtype=torch.uint8, device=DEV)
    with pytest.raises(ri.ProjectionError, match="contiguous float32"):
        ri.project_points(pts.double(), **kw, workspace=ws)
    with pytest.raises(ri.ProjectionError, match="not contiguous"):
        ri.project_points(torch.zeros((4, 1000), device=DEV).t(), **kw, workspace=ws)
    with pytest.raises(ri.ProjectionError, match=r"\(N, 4\)"):
        ri.project_points(pts.reshape(-1), **kw, workspace=ws)
    with pytest.raises(ri.ProjectionError, match=r"\(N, 4\)"):
        ri.project_points(pts[:, :2].contiguous(), **kw, workspace=ws)
    with pytest.raises(ri.ProjectionError, match="offsets is host data"):
        ri.project_points(pts, **{**kw, "offsets": torch.as_tensor(kw["offsets"]).to(DEV)}, workspace=ws)
    with pytest.raises(ri.ProjectionError, match="offsets must ascend"):
        ri.project_points(pts, **{**kw, "offsets": [0, 600, 400, 1000]}, workspace=ws)
    with pytest.raises(ri.ProjectionError, match="offsets must ascend"):
        ri.project_points(pts, **{**kw, "offsets": [0, 400, 600, 999]}, workspace=ws)
    with pytest.raises(ri.ProjectionError, match="inclination holds 2 bounds or one angle per row"):
        ri.project_points(pts, **{**kw, "inclination": kw["inclination"][:7]}, workspace=ws)
    with pytest.raises(ri.ProjectionError, match="strictly monotonic"):
        ri.project_points(pts, **{**kw, "inclination": kw["inclination"][:6] + kw["inclination"][:2]}, workspace=ws)
    with pytest.raises(ri.ProjectionError, match="3 frames of 30000 x 30000"):
        ri.project_points(pts, **{**kw, "H": 30000, "W": 30000, "inclination": list(rc.KITTI_INC)}, workspace=ws)
    with pytest.raises(ri.ProjectionError, match="2147483648 points"):
        ri.project_points(torch.zeros((1, 4), device=DEV).expand(2 ** 31, 4), **{**kw, "offsets": None})
    with pytest.raises(ri.ProjectionError, match="workspace must be a contiguous uint8 tensor"):
        ri.project_points(pts, **kw, workspace=ws.cpu())
    with pytest.raises(ri.ProjectionError, match="workspace must be a contiguous uint8 tensor"):
        ri.project_points(pts, **kw, workspace=ws[:100])
    with pytest.raises(ri.ProjectionError, match=r"points2sensor must be \(3, 3, 4\)"):
        ri.project_points(pts, **{**kw, "points2sensor": np.zeros((2, 3, 4))}, workspace=ws)
    torch.cuda.synchronize()
    assert bool((ws == 0x5A).all()), "a refused call wrote to the workspace"
    # the library's own refusal, on the device that exists, and a valid call after it
    lib = ri.load()
    assert lib.lrt_project_points(0, 10, None, 1, None, None, 8, 64, None, 2, 0.0, 0.0, 0.0, 80.0, 1, None, None, None, None, None, None, 0, None) < 0
    assert b"null points" in lib.lrt_project_last_error()
    same(ri.project_points(pts, **kw, workspace=ws), c.twin, "after the refusals")


# ---- 5. no host wait ------------------------------------------------------------------------------------------------------------------------------------------------

def test_a_call_does_not_wait_for_the_device():
    c = rc.random_cloud(70_000, 3, 66, 1030, "waymo_table_yaw", 22, transform=True)
    pts = torch.tensor(c.points, device=DEV)
    ri.project_points(pts, **c.kw)                                                         # warm: the loaded library, the allocators
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        op = ri.project_points(pts, **c.kw)
        op3 = ri.project_points(pts[:, :3].contiguous(), **c.kw)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    same(op, c.twin, "under the sync debug mode")
    assert torch.equal(bits(op3.depth), bits(c.twin.depth))


# ---- 6. ingest ------------------------------------------------------------------------------------------------------------------------------------------------------

def test_ingest_on_the_device_writes_what_the_cpu_path_writes(tmp_path):
    ic = rc.ingest_clouds()
    roots = {}
    for dev in ("cpu", "cuda"):
        roots[dev] = str(tmp_path / dev)
        rep = ingest.ingest_point_clouds(roots[dev], ((f.id, f.points, f.sensor2world) for f in ic.frames), ic.H, ic.W, ic.inclination, device=dev, batch=3,
                                         test_frames=[7])
        assert rep["device"] == dev
    for f in ic.frames:
        za, zb = (np.load(os.path.join(roots[d], "frames", f"{f.id:06d}.npz")) for d in ("cpu", "cuda"))
        assert sorted(za.files) == sorted(zb.files)
        for k in za.files:
            assert za[k].dtype == zb[k].dtype and za[k].shape == zb[k].shape and za[k].tobytes() == zb[k].tobytes(), (f.id, k)
        assert np.array_equal(zb["mask"], f.mask)
    for name in ("meta.json",):
        assert open(os.path.join(roots["cpu"], name)).read() == open(os.path.join(roots["cuda"], name)).read()
    import json
    a, b = (json.load(open(os.path.join(roots[d], "ingest.json"))) for d in ("cpu", "cuda"))
    assert a["frames"] == b["frames"] and a["total"] == b["total"] and a["extent"] == b["extent"]
