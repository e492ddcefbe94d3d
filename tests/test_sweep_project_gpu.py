"""The range-image projection under the sweep model on the GPU (`liblrt_sweepproj.so` through `lidar_rt_amd.sweep_project`): depth, intensity, mask,
index and the seven counts against the float64 twin bit for bit on the cases of tests/sweep_project_cases.py (every one keeps its column and row
coordinates off the rounding boundaries and its kept ranges off the float32 ones), zero motion against the static operator on the device, the
round trip on the sweep-ray grid and on the rays of the HIP sweep_rays operator itself, the heaviest contention on one word, a dirty workspace,
equal bits for equal inputs, the refused calls, no host wait inside a call, and the ingest of compensated clouds against the CPU path byte for
byte."""
import json
import os

import numpy as np
import pytest
import torch

from lidar_rt_amd import ingest, range_image as ri, sweep, sweep_project as sp
from tests import range_image_cases as rc, sweep_project_cases as sc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
POINTS = [1, 63, 64, 65, 255, 256, 257, 1000, 70_000]          # around a wave, around a workgroup, several workgroups, many
ALL_SIZES = sc.SIZES + [(66, 1030)]


def bits(t):
    t = t.detach().contiguous()
    return (t.view(torch.int32) if t.dtype == torch.float32 else t).cpu()


def run(c, **over):
    pts = torch.tensor(c.points, device=DEV)
    keep = pts.clone()
    op = sp.project_points_sweep(pts, **{**c.kw, **over})
    torch.cuda.synchronize()
    assert torch.equal(bits(pts), bits(keep)), "the points changed"
    return op


def same(op, tw, label=""):
    assert op.depth.dtype == torch.float32 and op.intensity.dtype == torch.float32 and op.mask.dtype == torch.bool and op.index.dtype == torch.int32 \
        and op.counts.dtype == torch.int64, label
    assert op.depth.shape == tw.depth.shape and op.counts.shape == tw.counts.shape and op.counts.shape[-1] == sp.N_COUNTS, label
    assert torch.equal(op.counts.cpu(), tw.counts), (label, op.counts.tolist(), tw.counts.tolist())
    assert torch.equal(op.mask.cpu(), tw.mask), label
    assert torch.equal(op.index.cpu(), tw.index), label
    assert torch.equal(bits(op.depth), bits(tw.depth)), label
    assert torch.equal(bits(op.intensity), bits(tw.intensity)), label


# ---- 1. the operator against the twin -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("N", POINTS)
def test_point_counts_and_ragged_frames_against_the_twin(N, F):
    c = sc.random_cloud(N, F, 8, 64, "kitti_bounds", sc.CLOUD_SEEDS.get((N, F), 11), "moderate_cw")
    same(run(c), c.twin, f"N {N} F {F}")


@pytest.mark.parametrize("mo", ["moderate_cw", "strong_ccw", "table"])
@pytest.mark.parametrize("wrap,transform", [(True, False), (False, True), (True, True)], ids=["wrap", "no_wrap_transform", "wrap_transform"])
@pytest.mark.parametrize("conv", sc.CONVENTIONS)
@pytest.mark.parametrize("H,W", ALL_SIZES)
def test_image_sizes_conventions_wrap_transform_and_motions_against_the_twin(H, W, conv, wrap, transform, mo):
    c = sc.random_cloud(1000, 3, H, W, conv, 21, mo, wrap=wrap, transform=transform)
    same(run(c), c.twin, f"{H} x {W} {conv} wrap {wrap} transform {transform} {mo}")
    cnt = c.twin.counts
    assert int(cnt[:, 6].sum()) > 0 and int(cnt[:, 3].sum()) > 0 and int(cnt[:, 4].sum()) > 0 and cnt[1].tolist() == [0] * 7
    assert np.ndim(c.kw["twist"]) == 2                                                      # a twist per frame


def test_the_closed_form_branch_of_the_exponential():
    c = sc.random_cloud(1000, 1, 8, 64, "kitti_bounds", 11, "closed")
    tau = sc.column_times(c.kw, 64)
    assert float(((tau * sc.CLOSED[5]) ** 2).max()) >= sweep.SERIES_TH2 > float(((tau * sc.CLOSED[5]) ** 2).min())      # both branches of sw_coef
    same(run(c), c.twin, "closed")


def test_seventy_thousand_points_into_66_x_1030_in_three_frames_with_transforms():
    c = sc.random_cloud(70_000, 3, 66, 1030, "waymo_table_yaw", 25, "moderate_cw", transform=True)
    same(run(c), c.twin, "70 000 points 66 x 1030")
    assert int(c.twin.counts[:, 5].sum()) > 1000 and int(c.twin.counts[:, 6].sum()) > 10_000 and int(c.twin.counts[:, 4].sum()) > 100


# ---- 2. zero motion is the static operator ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("twist", [None, sc.ZERO], ids=["no_twist", "zero_twist"])
def test_zero_motion_equals_project_points_on_the_device(twist):
    cases = [rc.random_cloud(1000, 3, H, W, cn, 21, wrap=wrap, transform=tr) for H, W in ALL_SIZES for cn in rc.CONVENTIONS
             for wrap, tr in ((True, False), (False, True))] + [rc.constructed(m, w) for m in ("bounds", "table") for w in (True, False)]
    for c in cases:
        pts = torch.tensor(c.points, device=DEV)
        want = ri.project_points(pts, **c.kw)
        got = sp.project_points_sweep(pts, twist=twist, **c.kw)
        torch.cuda.synchronize()
        for k in ("depth", "intensity", "mask", "index"):
            assert torch.equal(bits(getattr(got, k)), bits(getattr(want, k))), (c.key, k)
        cnt = got.counts.reshape(-1, sp.N_COUNTS).cpu()
        assert torch.equal(cnt[:, [0, 1, 2, 3, 5, 6]], want.counts.reshape(-1, ri.N_COUNTS).cpu()) and int(cnt[:, 4].sum()) == 0, c.key


# ---- 3. the round trip ----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mo,posed", [("moderate_cw", False), ("moderate_ccw", True), ("strong_cw", False), ("minus_strong_ccw", False)])
@pytest.mark.parametrize("conv", sc.CONVENTIONS)
@pytest.mark.parametrize("H,W", sc.SIZES)
def test_the_round_trip_on_the_sweep_ray_grid(H, W, conv, mo, posed):
    c = sc.grid(H, W, conv, sc.GRID_SEED, mo, posed=posed)
    op = run(c)
    same(op, c.twin, f"grid {H} x {W} {conv} {mo}")
    assert torch.equal(op.index.reshape(-1).cpu(), torch.arange(H * W, dtype=torch.int32)) and bool(op.mask.all())


@pytest.mark.parametrize("H,W", sc.SIZES)
def test_the_strong_turn_whose_seam_overlaps(H, W):
    for mo in ("strong_ccw", "minus_strong_cw"):
        c = sc.grid(H, W, "kitti_bounds", sc.GRID_SEED, mo, own_pixel=False)
        same(run(c), c.twin, f"overlap {H} x {W} {mo}")


@pytest.mark.parametrize("mo", ["moderate_cw", "strong_cw"])
@pytest.mark.parametrize("H,W", sc.SIZES)
def test_points_made_by_the_hip_sweep_rays_operator_return_to_their_own_pixels(H, W, mo):
    """The other library's own output (float32 o and d on the device) times a range: no code is shared between the two."""
    conv = rc.convention("kitti_bounds", H)
    m = sc.motion(mo, W)
    o, d = sweep.sweep_rays(torch.eye(4, device=DEV)[:3], torch.tensor(m["twist"], dtype=torch.float32, device=DEV), H, W, conv["inclination"], "KITTI", None,
                            t_ref=m["t_ref"])
    r = torch.tensor(np.random.default_rng([sc.GRID_SEED, H, W]).uniform(2.0, 62.0, (H, W, 1)), dtype=torch.float32, device=DEV)
    pts = torch.cat([(o + d * r).reshape(-1, 3), torch.full((H * W, 1), 0.5, device=DEV)], 1).contiguous()
    tw = sp.project_points_sweep_reference(pts, H, W, conv["inclination"], m["twist"], t_ref=m["t_ref"], direction=m["direction"])
    assert tw.margin >= sc.MARGIN and tw.range_margin >= sc.RANGE_MARGIN
    op = sp.project_points_sweep(pts, H, W, conv["inclination"], m["twist"], t_ref=m["t_ref"], direction=m["direction"])
    same(op, tw, f"sweep_rays {H} x {W} {mo}")
    assert torch.equal(op.index.reshape(-1).cpu(), torch.arange(H * W, dtype=torch.int32)) and op.counts.tolist() == [H * W, 0, 0, 0, 0, 0, H * W]
    assert float(((op.depth.reshape(-1) - r.reshape(-1)).abs() / r.reshape(-1)).max()) <= 1e-5


def test_the_constructed_points():
    b = sc.between_columns()
    op = run(b)
    same(op, b.twin, "between two columns")
    assert op.counts.tolist() == [3, 0, 0, 0, 2, 0, 1]
    e = sc.beyond_the_edge()
    op = run(e)
    same(op, e.twin, "beyond the edge")
    assert op.counts.tolist() == [2, 0, 0, 1, 0, 0, 1]


def test_three_columns_and_no_points():
    c = sc.random_cloud(1000, 1, 8, 64, "kitti_bounds", 11)
    op = sp.project_points_sweep(torch.tensor(c.points[:, :3], device=DEV), **c.kw)        # (N, 3): the intensity is 0
    tw = sp.project_points_sweep_reference(c.points[:, :3], **c.kw)
    same(op, tw, "(N, 3)")
    assert float(op.intensity.abs().sum()) == 0.0 and torch.equal(bits(op.depth), bits(c.twin.depth))
    kw = dict(H=5, W=37, inclination=list(rc.KITTI_INC), twist=np.array(sc.MODERATE), offsets=[0, 0, 0])
    empty = sp.project_points_sweep(torch.zeros((0, 4), device=DEV), **kw)
    same(empty, sp.project_points_sweep_reference(np.zeros((0, 4), np.float32), **kw), "no points")
    assert empty.counts.tolist() == [[0] * 7] * 2 and not bool(empty.mask.any()) and bool((empty.index == -1).all())


# ---- 4. contention on one word --------------------------------------------------------------------------------------------------------------------------------------

def test_everything_into_one_pixel_and_equal_ranges():
    c = sc.one_ray(1000)
    op = run(c)
    same(op, c.twin, "1000 points on one sweep ray")
    assert op.counts.tolist() == [1000, 0, 0, 0, 0, 999, 1] and int(op.index[3, 20]) == int(np.argmin(c.ranges))
    e = sc.one_ray(300, equal=True)
    op = run(e)
    same(op, e.twin, "300 equal ranges")
    assert op.counts.tolist() == [300, 0, 0, 0, 0, 299, 1] and int(op.index[3, 20]) == 0


# ---- 5. a dirty workspace, repeated calls ---------------------------------------------------------------------------------------------------------------------------

def test_a_dirty_workspace_does_not_leak_and_equal_inputs_give_equal_bits():
    big = sc.random_cloud(70_000, 1, 8, 64, "kitti_bounds", sc.CLOUD_SEEDS[(70_000, 1)])
    small = sc.random_cloud(63, 1, 8, 64, "kitti_bounds", 11, "strong_ccw")
    ws = torch.zeros(sp.work_bytes(1, 8, 64) + 512, dtype=torch.uint8, device=DEV)          # zeros: the SMALLEST key everywhere, a table of zeros
    same(run(big, workspace=ws), big.twin, "large cloud, zeroed workspace")
    first = run(small, workspace=ws)                                                        # another motion on the large cloud's keys and table
    same(first, small.twin, "small cloud on the large cloud's workspace")
    assert int(small.twin.counts[6]) < int(big.twin.counts[6])
    static = run(small, workspace=ws, twist=None)                                           # no twist: the table left behind is not read
    same(static, sp.project_points_sweep_reference(small.points, **{**small.kw, "twist": None}), "no twist on a used workspace")
    for _ in range(3):
        again = run(small, workspace=ws)
        for a, b in zip(again, first):
            assert torch.equal(bits(a), bits(b))
    fresh = run(small)
    for a, b in zip(fresh, first):
        assert torch.equal(bits(a), bits(b))


def test_a_permuted_point_order_gives_what_the_twin_gives_on_it():
    c = sc.random_cloud(70_000, 3, 8, 64, "kitti_bounds", 11)
    off = c.kw["offsets"]
    rng = np.random.default_rng(4)
    perm = np.concatenate([off[f] + rng.permutation(off[f + 1] - off[f]) for f in range(3)])          # within every frame
    pts = np.ascontiguousarray(c.points[perm])
    tw = sp.project_points_sweep_reference(pts, **c.kw)
    assert tw.margin >= sc.MARGIN and tw.range_margin >= sc.RANGE_MARGIN
    op = sp.project_points_sweep(torch.tensor(pts, device=DEV), **c.kw)
    same(op, tw, "permuted")
    assert torch.equal(bits(op.depth), bits(c.twin.depth)) and torch.equal(op.counts.cpu(), c.twin.counts)


# ---- 6. inputs and refusals -----------------------------------------------------------------------------------------------------------------------------------------

def test_refused_calls_raise_and_launch_nothing():
    c = sc.random_cloud(1000, 3, 8, 64, "waymo_table_yaw", 21)
    pts = torch.tensor(c.points, device=DEV)
    kw = dict(c.kw)
    ws = torch.full((sp.work_bytes(3, 8, 64),), 0x5A, dtype=torch.uint8, device=DEV)
    with pytest.raises(ri.ProjectionError, match="contiguous float32"):
        sp.project_points_sweep(pts.double(), **kw, workspace=ws)
    with pytest.raises(ri.ProjectionError, match="not contiguous"):
        sp.project_points_sweep(torch.zeros((4, 1000), device=DEV).t(), **kw, workspace=ws)
    with pytest.raises(ri.ProjectionError, match=r"\(N, 4\)"):
        sp.project_points_sweep(pts.reshape(-1), **kw, workspace=ws)
    with pytest.raises(ri.ProjectionError, match="offsets is host data"):
        sp.project_points_sweep(pts, **{**kw, "offsets": torch.as_tensor(kw["offsets"]).to(DEV)}, workspace=ws)
    with pytest.raises(ri.ProjectionError, match="twist is host data"):
        sp.project_points_sweep(pts, **{**kw, "twist": torch.as_tensor(kw["twist"]).to(DEV)}, workspace=ws)
    with pytest.raises(ri.ProjectionError, match="tau is host data"):
        sp.project_points_sweep(pts, **{**kw, "tau": sweep.column_times(64).to(DEV)}, workspace=ws)
    with pytest.raises(ri.ProjectionError, match="a non-finite twist"):
        sp.project_points_sweep(pts, **{**kw, "twist": [0.0, 0.0, float("inf"), 0.0, 0.0, 0.0]}, workspace=ws)
    with pytest.raises(ri.ProjectionError, match="a non-finite tau"):
        sp.project_points_sweep(pts, **{**kw, "tau": [float("nan")] * 64}, workspace=ws)
    with pytest.raises(ri.ProjectionError, match=r"twist must be \(6,\) or \(3, 6\)"):
        sp.project_points_sweep(pts, **{**kw, "twist": np.zeros((2, 6))}, workspace=ws)
    with pytest.raises(ri.ProjectionError, match="offsets must ascend"):
        sp.project_points_sweep(pts, **{**kw, "offsets": [0, 600, 400, 1000]}, workspace=ws)
    with pytest.raises(ri.ProjectionError, match="inclination holds 2 bounds or one angle per row"):
        sp.project_points_sweep(pts, **{**kw, "inclination": kw["inclination"][:7]}, workspace=ws)
    with pytest.raises(ri.ProjectionError, match="3 frames of 30000 x 30000"):
        sp.project_points_sweep(pts, **{**kw, "H": 30000, "W": 30000, "inclination": list(rc.KITTI_INC), "tau": None}, workspace=ws)
    with pytest.raises(ri.ProjectionError, match="workspace must be a contiguous uint8 tensor"):
        sp.project_points_sweep(pts, **kw, workspace=ws.cpu())
    with pytest.raises(ri.ProjectionError, match="workspace must be a contiguous uint8 tensor"):
        sp.project_points_sweep(pts, **kw, workspace=ws[:sp.work_bytes(3, 8, 64) - 256])    # the key image alone is not enough
    with pytest.raises(ri.ProjectionError, match=r"points2sensor must be \(3, 3, 4\)"):
        sp.project_points_sweep(pts, **{**kw, "points2sensor": np.zeros((2, 3, 4))}, workspace=ws)
    torch.cuda.synchronize()
    assert bool((ws == 0x5A).all()), "a refused call wrote to the workspace"
    # the library's own refusals, on the device that exists, and a valid call after them
    lib = sp.load()
    args = (8, 64, None, 2, 0.0, 0.0, 0.0, 80.0, 1, None, None, None, None, None, None, 0, None)
    assert lib.lrt_sweepproj_points(0, 10, None, 1, None, None, None, None, *args) < 0 and b"null points" in lib.lrt_sweepproj_last_error()
    d = torch.zeros(64, dtype=torch.float64, device=DEV)
    out = [torch.zeros(8 * 64, dtype=torch.float64, device=DEV) for _ in range(5)]
    assert lib.lrt_sweepproj_points(0, 4, d.data_ptr(), 1, d.data_ptr(), None, d.data_ptr(), None, 8, 64, d.data_ptr(), 2, 0.0, 0.0, 0.0, 80.0, 1,
                                    *[o.data_ptr() for o in out], ws.data_ptr(), ws.numel(), None) < 0
    assert b"null tau pointer with a twist" in lib.lrt_sweepproj_last_error()
    torch.cuda.synchronize()
    assert bool((ws == 0x5A).all()) and all(float(o.abs().sum()) == 0.0 for o in out)
    same(sp.project_points_sweep(pts, **kw, workspace=ws), c.twin, "after the refusals")


# ---- 7. no host wait ------------------------------------------------------------------------------------------------------------------------------------------------

def test_a_call_does_not_wait_for_the_device():
    c = sc.random_cloud(70_000, 3, 66, 1030, "waymo_table_yaw", 25, "moderate_cw", transform=True)
    pts = torch.tensor(c.points, device=DEV)
    sp.project_points_sweep(pts, **c.kw)                                                   # warm: the loaded library, the allocators
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        op = sp.project_points_sweep(pts, **c.kw)
        op3 = sp.project_points_sweep(pts[:, :3].contiguous(), **c.kw)
        op0 = sp.project_points_sweep(pts, **{**c.kw, "twist": None})
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    same(op, c.twin, "under the sync debug mode")
    assert torch.equal(bits(op3.depth), bits(c.twin.depth)) and int(op0.counts[:, 4].sum()) == 0


# ---- 8. ingest ------------------------------------------------------------------------------------------------------------------------------------------------------

def test_ingest_of_compensated_clouds_on_the_device_writes_what_the_cpu_path_writes(tmp_path):
    ic = sc.ingest_clouds()
    roots = {}
    for dev in ("cpu", "cuda"):
        roots[dev] = str(tmp_path / dev)
        rep = ingest.ingest_point_clouds(roots[dev], ((f.id, f.points, f.sensor2world) for f in ic.frames), ic.H, ic.W, ic.inclination,
                                         twists={f.id: f.twist for f in ic.frames}, compensated=True, sweep_ref=ic.t_ref, sweep_direction=ic.direction, device=dev,
                                         batch=3, test_frames=[7])
        assert rep["device"] == dev and rep["compensated"] is True
    for f in ic.frames:
        za, zb = (np.load(os.path.join(roots[d], "frames", f"{f.id:06d}.npz")) for d in ("cpu", "cuda"))
        assert sorted(za.files) == sorted(zb.files) and "tau" in za.files
        for k in za.files:
            assert za[k].dtype == zb[k].dtype and za[k].shape == zb[k].shape and za[k].tobytes() == zb[k].tobytes(), (f.id, k)
        assert np.array_equal(zb["mask"], f.mask)
    assert open(os.path.join(roots["cpu"], "meta.json")).read() == open(os.path.join(roots["cuda"], "meta.json")).read()
    a, b = (json.load(open(os.path.join(roots[d], "ingest.json"))) for d in ("cpu", "cuda"))
    assert a["frames"] == b["frames"] and a["total"] == b["total"] and a["extent"] == b["extent"] and set(a["total"]) == set(sp.COUNT_NAMES)
