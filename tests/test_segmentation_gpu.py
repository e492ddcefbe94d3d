"""Range-image segmentation on the GPU: every operator of `liblrt_segment.so` EQUAL to its numpy twin, int for int, on the cases of
tests/segment_cases.py; frames in one call against frames one by one, equal bits for equal inputs, the launch counts, and `actors.discover` on the
device returning the twin's boxes bit for bit."""
import math

import numpy as np
import pytest
import torch

from lidar_rt_amd import actors, segmentation as sg
from tests import segment_cases as sc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def device_label(key):
    c = sc.label_case(key)
    return c, sg.label(c.points.to(DEV), c.mask.to(DEV), **c.kw)


def same_stats(got, want):
    return (torch.equal(got.seg.cpu(), want.seg) and torch.equal(got.n_seg.cpu(), want.n_seg) and torch.equal(got.overflow.cpu(), want.overflow)
            and torch.equal(got.table.cpu(), want.table))


@pytest.mark.parametrize("key", sc.LABEL_KEYS)
def test_label_and_stats_are_the_twin(key):
    c, lab = device_label(key)
    want = sc.label_reference(key)
    assert lab.dtype == torch.int32 and lab.shape == (c.H, c.W)
    assert torch.equal(lab.cpu(), want), (key, int((lab.cpu() != want).sum()))
    if c.expected is not None:
        assert torch.equal(lab.cpu(), c.expected)
    st = sg.stats(c.points.to(DEV), lab, tuple(e.to(DEV) for e in c.ev), 512)
    assert st.table.dtype == torch.int64 and st.table.shape == (512, sg.NCOL)
    assert same_stats(st, sc.stats_reference(key)), key
    assert int(st.overflow) == 0 and not st.table[int(st.n_seg):].any()


def test_the_capacity_overflows_into_its_count():
    c, lab = device_label("checker")
    st = sg.stats(c.points.to(DEV), lab, tuple(e.to(DEV) for e in c.ev), 16)
    want = sc.stats_reference("checker", 16)
    assert same_stats(st, want)
    assert int(st.n_seg) == 16 and int(st.overflow) == 256 - 16 and int((st.seg >= 0).sum()) == 16
    one = sg.stats(c.points.to(DEV), lab, (c.ev[0].to(DEV),), 16)                    # one evidence image: the second pair of columns is zero
    assert not one.table[:, sg.COL_EV + 2:sg.COL_EV + 4].any() and torch.equal(one.table[:, :sg.COL_EV + 2], st.table[:, :sg.COL_EV + 2])


def test_a_batch_is_its_frames_and_two_calls_give_the_same_bits():
    cs = [sc.label_case(k) for k in sc.RANDOM_KEYS]
    pts, mask = torch.stack([c.points for c in cs]).to(DEV), torch.stack([c.mask for c in cs]).to(DEV)
    ev = tuple(torch.stack([c.ev[k] for c in cs]).to(DEV) for k in range(2))
    kw = cs[0].kw
    lab = sg.label(pts, mask, **kw)
    st = sg.stats(pts, lab, ev, 512)
    for f, k in enumerate(sc.RANDOM_KEYS):
        one = sg.label(pts[f], mask[f], **kw)
        assert torch.equal(one, lab[f]) and torch.equal(one.cpu(), sc.label_reference(k)), k
        s1 = sg.stats(pts[f], one, tuple(e[f] for e in ev), 512)
        assert torch.equal(s1.seg, st.seg[f]) and torch.equal(s1.table, st.table[f]) and int(s1.n_seg) == int(st.n_seg[f])
    again = sg.label(pts, mask, **kw)
    ws = torch.full((sg.work_bytes(3, 16, 128) + 256,), 0xAB, dtype=torch.uint8, device=DEV)                  # a dirty workspace of the caller
    st2 = sg.stats(pts, again, ev, 512, workspace=ws)
    assert torch.equal(again, lab) and torch.equal(st2.table, st.table) and torch.equal(st2.seg, st.seg)
    ex = (torch.arange(16 * 128, device=DEV).reshape(16, 128) % 7 == 0).expand(3, 16, 128).contiguous()      # an exclusion image
    assert torch.equal(sg.label(pts, mask, exclude=ex, **kw).cpu(), sg.label_reference(pts.cpu(), mask.cpu(), exclude=ex.cpu(), **kw))


def test_ground_is_the_twin():
    p, m, inc, want = sc.ground_columns()
    assert torch.equal(sg.ground(p.to(DEV), m.to(DEV), sc.SENSOR_HEIGHT, inc).cpu(), want)
    flipped = sg.ground(p.flip(0).contiguous().to(DEV), m.flip(0).contiguous().to(DEV), sc.SENSOR_HEIGHT, [0.1, -0.4])        # the other row order
    assert torch.equal(flipped.cpu(), want.flip(0))
    for key in sc.FREE_KEYS:                                                               # the world's frames, bounds and a per-beam table
        c = sc.free_case(key)
        got = sg.ground(c.src[0].to(DEV), c.src[1].to(DEV), sc.SENSOR_HEIGHT, c.kw["inclination"])
        assert torch.equal(got.cpu(), sg.ground_reference(c.src[0], c.src[1], sc.SENSOR_HEIGHT, c.kw["inclination"])), key
    s = sc.scenario()
    pts, mask = torch.stack([s.frames[i][0] for i in s.ids]), torch.stack([s.frames[i][2] for i in s.ids])
    tilted = dict(up=(0.0, math.sin(0.05), math.cos(0.05)), slope=0.3, z_lo=-2.0, z_hi=-1.5)
    assert torch.equal(sg.ground(pts.to(DEV), mask.to(DEV), None, s.kw["inclination"], **tilted).cpu(), sg.ground_reference(pts, mask, None, s.kw["inclination"], **tilted))


@pytest.mark.parametrize("key", sc.FREE_KEYS)
def test_freespace_is_the_twin(key):
    c = sc.free_case(key)
    src, tgt = tuple(t.to(DEV) for t in c.src), tuple(t.to(DEV) for t in c.tgt)
    for window in (sg.DEFAULT_WINDOW, (4, 16), (0, 0)):
        got = sg.freespace(src, tgt, c.X.to(DEV), window=window, **c.kw)
        want = sg.freespace_reference(c.src, c.tgt, c.X, window=window, **c.kw)
        assert got.dtype == torch.int8 and torch.equal(got.cpu(), want), (key, window, int((got.cpu() != want).sum()))
    if key == "empty":
        assert bool((got == -1).all())


def test_track_bounds_are_the_twin():
    b = sc.bounds_case()
    bounds, count = sg.track_bounds(b.points.to(DEV), b.seg.to(DEV), b.track_of.to(DEV), b.pose.to(DEV))
    w_bounds, w_count = sg.track_bounds_reference(b.points, b.seg, b.track_of, b.pose)
    assert torch.equal(bounds.cpu(), w_bounds) and torch.equal(count.cpu(), w_count)
    none = torch.full_like(b.track_of, -1)
    none[0, 0] = 1                                                                         # track 0 has no pixel
    bounds, count = sg.track_bounds(b.points.to(DEV), b.seg.to(DEV), none.to(DEV), b.pose.to(DEV))
    assert int(count[0]) == 0 and bounds[0].tolist() == [sg.I64_MAX] * 3 + [sg.I64_MIN] * 3 and int(count[1]) > 0


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = {e.key: e.count for e in prof.key_averages() if e.device_time_total > 0}
    return {k: v for k, v in ev.items() if "memcpy" not in k.lower() and "memset" not in k.lower()}


def test_every_operator_launches_a_fixed_number_of_its_own_kernels():
    counts = {}
    for key in ("empty", "serpent", "checker"):
        c = sc.label_case(key)
        p, m, ev = c.points.to(DEV), c.mask.to(DEV), tuple(e.to(DEV) for e in c.ev)
        lab = sg.label(p, m, **c.kw)
        st = sg.stats(p, lab, ev, 512)
        depth = torch.linalg.norm(p, dim=-1)
        X = torch.eye(4, dtype=torch.float64, device=DEV)[:3].contiguous()
        track_of = torch.zeros(512, dtype=torch.int32, device=DEV)
        ops = {"label": lambda: sg.label(p, m, **c.kw), "stats": lambda: sg.stats(p, lab, ev, 512),
               "ground": lambda: sg.ground(p, m, 1.8, [-0.4, 0.1]),
               "freespace": lambda: sg.freespace((p, m), (depth, m), X, inclination=[-0.4, 0.1]),
               "track_bounds": lambda: sg.track_bounds(p, st.seg, track_of, X[None])}
        for name, fn in ops.items():
            ev_ = launches(fn)
            assert all("k_seg_" in k for k in ev_), (key, name, ev_)
            counts.setdefault(name, {})[key] = sum(ev_.values())
    print(counts)
    for name, per_case in counts.items():
        assert len(set(per_case.values())) == 1, (name, per_case)
    assert {n: v["empty"] for n, v in counts.items()} == {"label": 3, "stats": 5, "ground": 1, "freespace": 1, "track_bounds": 2}


def test_discover_on_the_device_returns_the_twins_boxes_bit_for_bit():
    s = sc.scenario()
    want, w_rep = sc.scenario_result()
    got, g_rep = actors.discover({i: tuple(t.to(DEV) for t in f) for i, f in s.frames.items()}, s.poses, sc.SENSOR_HEIGHT, **s.kw)
    assert g_rep == w_rep
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k


def test_the_discovered_boxes_give_every_actor_asset_real_returns(tmp_path):
    from lidar_rt_amd import sequence
    s = sc.scenario()
    boxes, _ = sc.scenario_result()
    root = str(tmp_path / "seq")
    sequence.write_sequence(root, [{"id": i, "depth": s.frames[i][1], "intensity": torch.full_like(s.frames[i][1], 0.5), "mask": s.frames[i][2],
                                    "inclination": s.kw["inclination"], "sensor2world": s.poses[i]} for i in s.ids], extent=20.0)
    sequence.write_boxes(root, boxes)
    seq = sequence.load_sequence(root, device=DEV)
    scene = sequence.scene_from_sequence(seq, init_from_frames=True)
    assert len(seq.boxes) == 2 and len(scene.gaussians_assets) == 3
    for a in range(2):
        assert seq.init_report[f"actor_{a:02d}"]["real"] >= actors.DEFAULTS["min_points"], seq.init_report
