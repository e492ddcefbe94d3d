"""The un-projection operator on the GPU: `liblrt_unproject.so` against the numpy twin bit for bit on every case of tests/unproject_cases.py,
a scan longer than its workgroup, a dirty workspace, equal bits for equal inputs, unchanged inputs, world mode against
``inverse_projection_with_range`` on the device, the refused calls and no host wait inside a call."""
import numpy as np
import pytest
import torch

from lidar_rt_amd import unproject as up
from lidar_rt_amd.training import RangeFrames
from tests import unproject_cases as uc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def dev(x):
    return None if x is None else (x if torch.is_tensor(x) else torch.tensor(np.asarray(x))).to(DEV)


def run(c, workspace=None, **over):
    kw = {**c.kw, **over}
    return up.points_from_range_images(dev(c.depth), dev(c.o), dev(c.d), intensity=dev(kw["intensity"]), keep=dev(kw["keep"]), raydrop=dev(kw["raydrop"]),
                                       raydrop_ratio=kw["raydrop_ratio"], world2out=kw["world2out"], min_depth=kw["min_depth"], max_depth=kw["max_depth"],
                                       workspace=workspace)


def same(op, twin, what):
    """points, pixel, offsets and counts bit for bit; the rows behind offsets[-1] are nobody's."""
    assert torch.equal(op.offsets.cpu(), twin.offsets), what
    assert torch.equal(op.counts.cpu(), twin.counts), what
    n = int(twin.offsets[-1])
    assert op.points.shape == twin.points.shape and op.pixel.shape == twin.pixel.shape and op.points.dtype == torch.float32 and op.pixel.dtype == torch.int32
    assert torch.equal(op.pixel[:n].cpu(), twin.pixel[:n]), what
    assert torch.equal(op.points[:n].cpu().view(torch.int32), twin.points[:n].view(torch.int32)), what


COMBOS = [(p, u, t) for p in uc.PATTERNS for u in uc.USES for t in uc.TRANSFORMS]      # the whole product: 45


# ---- 1. against the twin ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", uc.GPU_SIZES)
def test_every_pattern_use_and_transform_against_the_twin(H, W):
    big = H * W > 4096                                                       # built for this test and not kept
    for F in (1, 3):
        for p, u, t in COMBOS:
            c = uc.random_frames(F, H, W, p, u, t, cache=not big)
            same(run(c), c.twin, f"{F} x {H} x {W} {p} {u} {t}")


def test_more_workgroups_than_the_scan_has_threads():
    c = uc.random_frames(3, 64, 2048, "random", "both", "column", cache=False)
    assert 3 * (64 * 2048 // up.BLOCK) > up.BLOCK
    same(run(c), c.twin, "3 x 64 x 2048")
    c = uc.random_frames(3, 64, 2048, "gap", "keep", "none", cache=False)
    same(run(c), c.twin, "3 x 64 x 2048 gap")


def test_one_image_without_a_frame_axis_and_without_intensity():
    c = uc.random_frames(1, 8, 64, "random", "both", "column")
    twin = up.points_from_range_images_reference(c.depth[0], c.o[0], c.d[0], keep=c.kw["keep"][0], raydrop=c.kw["raydrop"][0], raydrop_ratio=uc.RATIO,
                                                 world2out=c.kw["world2out"][0], min_depth=0.5, max_depth=80.0)
    op = up.points_from_range_images(dev(c.depth[0]), dev(c.o[0]), dev(c.d[0]), keep=dev(c.kw["keep"][0]).view(torch.uint8), raydrop=dev(c.kw["raydrop"][0]),
                                     raydrop_ratio=uc.RATIO, world2out=torch.tensor(c.kw["world2out"][0]), min_depth=0.5, max_depth=80.0)
    assert op.counts.shape == (5,) and op.offsets.shape == (2,)
    same(op, twin, "one image")
    one = op.trim()
    n = int(twin.offsets[-1])
    assert one.points.shape == (n, 4) and not one.points[:, 3].any() and one.points.data_ptr() == op.points.data_ptr()
    assert torch.equal(twin.points[:n, :3], c.twin.points[:n, :3])            # the same points as with the frame axis


# ---- 2. workspace, repeatability, inputs ----------------------------------------------------------------------------------------------------------------------

def test_a_dirty_workspace_does_not_leak_and_equal_inputs_give_equal_bits():
    big = uc.random_frames(3, 66, 1030, "random", "both", "frame", cache=False)
    small = uc.random_frames(3, 5, 37, "random", "keep", "column")
    ws = torch.empty(up.work_bytes(3, 66, 1030), dtype=torch.uint8, device=DEV)
    a = run(big, workspace=ws)
    same(a, big.twin, "big, fresh")
    same(run(small, workspace=ws), small.twin, "small, in the big one's workspace")
    ws.fill_(0xFF)
    same(run(small, workspace=ws), small.twin, "small, ones")
    ws.fill_(0x7F)
    b = run(big, workspace=ws)
    same(b, big.twin, "big, dirty")
    n = int(big.twin.offsets[-1])
    assert torch.equal(a.points[:n].view(torch.int32), b.points[:n].view(torch.int32)) and torch.equal(a.pixel[:n], b.pixel[:n])
    with pytest.raises(up.UnprojectError, match="workspace"):
        run(big, workspace=ws[:-256])
    with pytest.raises(up.UnprojectError, match="workspace"):
        run(big, workspace=ws[1:])


def test_the_inputs_are_not_changed():
    c = uc.random_frames(3, 8, 64, "random", "both", "column")
    t = [dev(x) for x in (c.depth, c.o, c.d, c.kw["intensity"], c.kw["keep"], c.kw["raydrop"])]
    before = [x.clone() for x in t]
    T = c.kw["world2out"].copy()
    up.points_from_range_images(t[0], t[1], t[2], intensity=t[3], keep=t[4], raydrop=t[5], raydrop_ratio=uc.RATIO, world2out=T, min_depth=0.5, max_depth=80.0)
    torch.cuda.synchronize()
    for x, y in zip(t, before):
        assert torch.equal(x.view(torch.uint8) if x.dtype == torch.bool else x.view(torch.int32), y.view(torch.uint8) if y.dtype == torch.bool else y.view(torch.int32))
    assert np.array_equal(T, c.kw["world2out"])


# ---- 3. world mode is the expression it replaces -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(5, 37), (66, 1030)])
def test_world_mode_equals_inverse_projection_with_range_on_the_device(H, W):
    c = uc.random_frames(3, H, W, "random", "keep", "none", empty_middle=False, cache=H * W <= 4096)
    op = run(c)
    off = op.offsets.cpu().tolist()
    rf = RangeFrames()
    for f in range(3):
        rf.add_frame(f, dev(c.o[f]), dev(c.d[f]), dev(c.depth[f]), dev(c.kw["intensity"][f]), torch.ones(H, W, dtype=torch.bool, device=DEV))
        kept = dev(c.twin.cls[f] == up.KEEP)
        want = rf.inverse_projection_with_range(f, dev(c.depth[f]), kept)
        got = op.points[off[f]:off[f + 1], :3].contiguous()
        assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32))


# ---- 4. refused calls ------------------------------------------------------------------------------------------------------------------------------------------

def test_refused_calls_raise_and_launch_nothing():
    c = uc.random_frames(3, 8, 64, "random", "both", "frame")
    depth, o, d, keep, drop = dev(c.depth), dev(c.o), dev(c.d), dev(c.kw["keep"]), dev(c.kw["raydrop"])
    E = up.UnprojectError
    with pytest.raises(E, match="float32"):
        up.points_from_range_images(depth.double(), o, d)
    with pytest.raises(E, match="float32"):
        up.points_from_range_images(depth, o, d.half())
    with pytest.raises(E, match="bool or uint8"):
        up.points_from_range_images(depth, o, d, keep=keep.to(torch.int32))
    with pytest.raises(E, match="not contiguous"):
        up.points_from_range_images(depth.transpose(1, 2).contiguous().transpose(1, 2), o, d)
    with pytest.raises(E, match="not contiguous"):
        up.points_from_range_images(depth, o, d, raydrop=torch.stack([drop, drop], -1)[..., 0])
    with pytest.raises(E, match="host data"):
        up.points_from_range_images(depth, o, d, world2out=dev(c.kw["world2out"]))
    with pytest.raises(E, match="is on"):
        up.points_from_range_images(depth, o.cpu(), d)
    z = torch.zeros(1, device=DEV)
    with pytest.raises(E, match="int32"):
        up.points_from_range_images(z.expand(2 ** 31, 1, 1), z.expand(2 ** 31, 1, 1, 3), z.expand(2 ** 31, 1, 1, 3))
    with pytest.raises(E, match="workgroups"):                                # fewer than 2^31 pixels, but a grid of 2^32 threads
        up.points_from_range_images(z.expand(2 ** 24, 1, 1), z.expand(2 ** 24, 1, 1, 3), z.expand(2 ** 24, 1, 1, 3))
    with pytest.raises(E):
        up.work_bytes(2, 2 ** 15, 2 ** 15)
    with pytest.raises(E):
        up.work_bytes(2 ** 24, 1, 100)
    # the library's own checks, behind the wrapper's: a refused call returns a code and a message
    lib = up.load()
    ws = torch.empty(up.work_bytes(3, 8, 64), dtype=torch.uint8, device=DEV)
    pts, pix = torch.empty((3 * 512, 4), device=DEV), torch.empty(3 * 512, dtype=torch.int32, device=DEV)
    offs, cnt = torch.empty(4, dtype=torch.int64, device=DEV), torch.empty((3, 5), dtype=torch.int64, device=DEV)
    import ctypes as C

    def call(F=3, depth_=depth, min_depth=0.0, max_depth=80.0, per_column=0, T=None, nbytes=ws.numel(), wsp=ws.data_ptr(), points=pts.data_ptr()):
        return lib.lrt_unproject_points(0, F, 8, 64, depth_.data_ptr() if depth_ is not None else None, o.data_ptr(), d.data_ptr(), None, None, None, 0.4, T, per_column,
                                        min_depth, max_depth, points, pix.data_ptr(), offs.data_ptr(), cnt.data_ptr(), wsp, nbytes,
                                        C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    cnt.fill_(-7)
    for kw in (dict(F=0), dict(F=2 ** 24), dict(depth_=None), dict(min_depth=-1.0), dict(max_depth=float("inf")), dict(per_column=1), dict(per_column=2), dict(nbytes=256),
               dict(wsp=ws.data_ptr() + 8), dict(points=pts.data_ptr() + 4)):
        assert call(**kw) == -1 and lib.lrt_unproject_last_error().decode().startswith("lrt_unproject_points:"), kw
    torch.cuda.synchronize()
    assert bool((cnt == -7).all())                                            # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert cnt[:, 0].tolist() == [512, 512, 512]


# ---- 5. no host wait -------------------------------------------------------------------------------------------------------------------------------------------

def test_a_call_does_not_wait_for_the_device():
    c = uc.random_frames(3, 66, 1030, "random", "both", "column", cache=False)
    t = [dev(x) for x in (c.depth, c.o, c.d, c.kw["intensity"], c.kw["keep"], c.kw["raydrop"])]
    up.work_bytes(3, 66, 1030)                                                # the library is loaded
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        op = up.points_from_range_images(t[0], t[1], t[2], intensity=t[3], keep=t[4], raydrop=t[5], raydrop_ratio=uc.RATIO, world2out=c.kw["world2out"],
                                         min_depth=0.5, max_depth=80.0)
        with pytest.raises(RuntimeError):
            op.trim()                                                         # the one place that waits
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    same(op, c.twin, "under the sync debug mode")
    assert [x.points.shape[0] for x in op.trim()] == c.twin.counts[:, 4].tolist()
