"""Range-image segmentation without a GPU: the twins on the cases whose answer is known, the conditioning of the seeded cases, the rules' header
compiled for the host against the twins, the sixteenth product library (`liblrt_segment.so`), and the refusals."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

from lidar_rt_amd import build as lrt_build, registration as rg, resources, segmentation as sg
from tests import segment_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


# ---- 1. the twins -----------------------------------------------------------------------------------------------------------------------------------------------

def test_the_flood_gives_the_smallest_index_of_every_component():
    for key, root in (("seam", 2 * 40), ("serpent", 0), ("u_shape", 10), ("full", 0)):
        c, lab = sc.label_case(key), sc.label_reference(key)
        assert bool((lab[c.mask] == root).all()) and bool((lab[~c.mask] == -1).all()), key
    for key in ("checker", "diagonal"):                                       # contacts by corners only are no contacts
        c, lab = sc.label_case(key), sc.label_reference(key)
        own = torch.arange(c.H * c.W, dtype=torch.int32).reshape(c.H, c.W)
        assert torch.equal(lab, torch.where(c.mask, own, torch.full_like(own, -1))), key
    assert bool((sc.label_reference("empty") == -1).all())
    c = sc.label_case("seam")
    cut = c.mask.clone()
    cut[2, 0] = False                                                          # without the pixel at the joint the component falls in two
    assert sorted(set(sg.label_reference(c.points, cut, **c.kw)[cut].tolist())) == [2 * 40 + 1, 2 * 40 + 37]
    assert int(c.mask.sum()) == 6 and int(sc.label_case("serpent").mask.sum()) > 1000
    for key in ("threshold_abs", "threshold_dir"):
        assert torch.equal(sc.label_reference(key), sc.label_case(key).expected), key
    for key in sc.RANDOM_KEYS + ("odd",):                                      # every label is the smallest index carrying it, and labels are roots
        lab = sc.label_reference(key).reshape(-1)
        kept = lab >= 0
        idx = torch.arange(lab.numel())
        assert bool((lab[kept] <= idx[kept]).all()) and bool((lab[lab[kept].long()] == lab[kept]).all())
        assert 1 < int(sc.stats_reference(key).n_seg) < int(kept.sum())


def test_the_table_rows_are_what_numpy_counts():
    key = "random_6"
    c, lab, st = sc.label_case(key), sc.label_reference(key), sc.stats_reference(key)
    n = int(st.n_seg)
    roots = torch.unique(lab[lab >= 0])
    assert n == roots.numel() and torch.equal(st.table[:n, sg.COL_ROOT], roots.long()) and not st.table[n:].any() and int(st.overflow) == 0
    for s in (0, n // 2, n - 1):
        sel = lab == roots[s]
        assert bool((st.seg[sel] == s).all()) and int(st.table[s, sg.COL_COUNT]) == int(sel.sum())
        q = np.rint(c.points[sel].numpy().astype(np.float64) * 1024.0).astype(np.int64)
        assert st.table[s, sg.COL_SUM:sg.COL_SUM + 3].tolist() == q.sum(0).tolist()
        assert st.table[s, sg.COL_MIN:sg.COL_MIN + 3].tolist() == q.min(0).tolist() and st.table[s, sg.COL_MAX:sg.COL_MAX + 3].tolist() == q.max(0).tolist()
        for k in range(2):
            assert int(st.table[s, sg.COL_EV + 2 * k]) == int((c.ev[k][sel] == 1).sum()) and int(st.table[s, sg.COL_EV + 2 * k + 1]) == int((c.ev[k][sel] >= 0).sum())
        assert int(st.table[s, 15]) == 0
    small = sc.stats_reference("checker", 16)
    assert int(small.n_seg) == 16 and int(small.overflow) == 240 and int((small.seg >= 0).sum()) == 16 and small.table.shape == (16, sg.NCOL)


def test_ground_columns_and_defaults():
    p, m, inc, want = sc.ground_columns()
    assert torch.equal(sg.ground(p, m, 1.8, inc), want)                       # CPU tensors: the twin
    assert torch.equal(sg.ground(p.flip(0).contiguous(), m.flip(0).contiguous(), 1.8, [0.1, -0.4]), want.flip(0))
    assert torch.equal(sg.ground(p, m, None, inc, z_lo=-2.2, z_hi=-1.4), want)
    assert sg.DEFAULT_SLOPE == pytest.approx(np.tan(np.radians(10.0))) and sg.default_thresholds(64, 2048, [-0.4, 0.1]) == pytest.approx((4 * 2 * np.pi / 2048, 4 * 0.5 / 63))
    with pytest.raises(sg.SegmentationError, match="sensor_height is required"):
        sg.ground(p, m, None, inc)
    with pytest.raises(sg.SegmentationError, match="unit vector"):
        sg.ground(p, m, 1.8, inc, up=(0, 0, 2))


def test_freespace_sees_through_where_the_slab_was():
    c = sc.free_case("room")
    ev = sg.freespace(c.src, c.tgt, c.X, **c.kw)
    counts = {v: int((ev == v).sum()) for v in (-1, 0, 1)}
    assert counts[1] > 50 and counts[0] > 1000 and bool((ev[~c.src[1]] == -1).all()), counts
    assert bool((sg.freespace(c.src, sc.free_case("empty").tgt, c.X, **c.kw) == -1).all())
    wide = sg.freespace(c.src, c.tgt, c.X, window=(4, 16), **c.kw)           # a larger window only ever withdraws a "free"
    assert bool((wide[ev == 0] == 0).all()) and int((wide == 1).sum()) <= counts[1]


def test_the_seeded_cases_are_conditioned():
    """No float64 decision of a case within 1e-9 (relative) of its threshold, no llrint argument within 1e-6 of a half (the quantised float32
    coordinates of the tables are exact products, and both sides round an exact half to even)."""
    p, m, inc, _ = sc.ground_columns()
    assert sg.ground_reference(p, m, 1.8, inc, return_margin=True)[1] > 1e-9
    for key in sc.FREE_KEYS:
        c = sc.free_case(key)
        assert sg.ground_reference(c.src[0], c.src[1], 1.8, c.kw["inclination"], return_margin=True)[1] > 1e-9, key
        for window in (sg.DEFAULT_WINDOW, (4, 16), (0, 0)):
            assert sg.freespace_reference(c.src, c.tgt, c.X, window=window, return_margin=True, **c.kw)[1] > 1e-9, (key, window)
    b = sc.bounds_case()
    assert sg.track_bounds_reference(b.points, b.seg, b.track_of, b.pose, return_margin=True)[2] > 1e-6


# ---- 2. the rules' header on the host -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("segment_check") / "segment_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "host_check", "segment_check.cpp")])
    return exe


@pytest.mark.parametrize("key", ("room", "waymo", "yaw"))
def test_the_rule_header_on_the_host_against_the_twins(host_check, key, tmp_path):
    c = sc.free_case(key)
    H, W = c.H, c.W
    inc, off, yaw, lo, hi = rg._model(H, W, c.kw["inclination"], c.kw["data_type"], c.kw["sensor2ego"], 0.0, rg.FLT_MAX)
    c_h, c_v = sg.default_thresholds(H, W, inc)
    up, slope, z_lo, z_hi = sg._ground_arguments(1.8, (0.0, 0.0, 1.0), sg.DEFAULT_SLOPE, None, None)
    pose = sc.rc.exp4(sc.rc.twist(91, 4.0, 25.0))[:3]
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as fh:
        fh.write(struct.pack("<8i", H, W, inc.size, 1, 2, 0, 0, 0))
        fh.write(struct.pack("<16d", off, yaw, lo, hi, sg.DEFAULT_M_ABS, sg.DEFAULT_M_REL, sg.DEFAULT_D_ABS, c_h, c_v, *up, z_lo, z_hi, slope, 0.0))
        fh.write(inc.tobytes()); fh.write(c.X.numpy().tobytes()); fh.write(np.ascontiguousarray(pose).tobytes())
        fh.write(c.src[0].numpy().tobytes()); fh.write(c.src[1].numpy().astype(np.uint8).tobytes())
        fh.write(c.tgt[0].numpy().tobytes()); fh.write(c.tgt[1].numpy().astype(np.uint8).tobytes())
    res = subprocess.run([host_check, inp, out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "SEGCHECK ok" in res.stdout, res.stdout + res.stderr
    raw = open(out, "rb").read()
    HW = H * W
    ground, jr, jd = (np.frombuffer(raw, np.uint8, HW, k * HW).reshape(H, W) for k in range(3))
    ev = np.frombuffer(raw, np.int8, HW, 3 * HW).reshape(H, W)
    q = np.frombuffer(raw, np.int64, 3 * HW, 4 * HW).reshape(H, W, 3)
    aq = np.frombuffer(raw, np.int64, 3 * HW, 4 * HW + 24 * HW).reshape(H, W, 3)
    p, m = c.src[0].numpy(), c.src[1].numpy()
    assert np.array_equal(ground, sg.ground_reference(c.src[0], c.src[1], 1.8, inc).numpy())
    assert np.array_equal(ev, sg.freespace_reference(c.src, c.tgt, c.X, **c.kw).numpy())
    assert np.array_equal(jr.astype(bool), m & np.roll(m, -1, 1) & sg.join_reference(p, np.roll(p, -1, 1), sg.DEFAULT_D_ABS, c_h))
    assert np.array_equal(jd[:-1].astype(bool), m[:-1] & m[1:] & sg.join_reference(p[:-1], p[1:], sg.DEFAULT_D_ABS, c_v)) and not jd[-1].any()
    assert np.array_equal(q, sg.quant_reference(p.astype(np.float64)))
    d = p.astype(np.float64) - pose[:, 3]
    a = np.stack([pose[0, k] * d[..., 0] + pose[1, k] * d[..., 1] + pose[2, k] * d[..., 2] for k in range(3)], -1)
    assert np.array_equal(aq, sg.quant_reference(a))
    lab = sg.label_reference(c.src[0], c.src[1], exclude=torch.from_numpy(ground.copy()), inclination=inc)       # the flood over the host's own joins
    kept = m & (ground == 0)
    assert np.array_equal(sg._flood(kept, kept & np.roll(kept, -1, 1) & jr.astype(bool), np.concatenate([kept[:-1] & kept[1:] & jd[:-1].astype(bool), np.zeros((1, W), bool)])),
                          lab.numpy())


# ---- 3. the library -----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def seg_lib():
    return lrt_build.build_segment()


def test_the_library_has_a_source_list_of_its_own_and_leaves_the_borrowed_headers_alone():
    assert lrt_build.SEGMENT_SOURCES == ["lrt_segment.hip"]
    assert {os.path.basename(h) for h in lrt_build.SEGMENT_HEADERS} == {"lrt_segment_math.h", "lrt_project_math.h", "lrt_sweep_math.h", "lrt_device_guard.h", "lrt_segment.h"}
    others = [getattr(lrt_build, n) for n in dir(lrt_build) if n.endswith(("SOURCES", "HEADERS")) and not n.startswith("SEGMENT_")]
    assert len(others) >= 30 and not any("lrt_segment" in f for lst in others for f in lst)
    assert os.path.basename(lrt_build.SEGMENT_LIB) == "liblrt_segment.so" and os.path.basename(lrt_build.SEGMENT_STAMP) == "liblrt_segment.srchash"
    assert re.fullmatch(r"[0-9a-f]{16}", lrt_build.segment_source_hash())
    src = open(lrt_build.__file__).read()
    assert "build_segment(force, verbose)" in src[src.index("def _build_product"):src.index("def _build_lib")]
    assert "csrc/liblrt_segment.so" in open(os.path.join(REPO, "setup.py")).read()
    body = src[src.index("def build_segment"):src.index("EXT_SRC =")]
    assert "CODEGEN_FLAGS" in body and "resources.check(SEGMENT_LIB)" in body
    mh = open(os.path.join(REPO, "lidar_rt_amd", "csrc", "lrt_segment_math.h")).read()
    assert '#include "lrt_project_math.h"' in mh and '#include "lrt_sweep_math.h"' in mh
    import hashlib
    for hdr, want in (("lrt_project_math.h", "cf3f97d820b9cdb3acd5c41202d19c9938c3057a72a5e7f8a23bb06e350d7b0c"),
                      ("lrt_sweep_math.h", "143796d2b4c11a794fdc7911f614fbc2561cb884c07e521b335c67f6466f52a1")):
        assert hashlib.sha256(open(os.path.join(REPO, "lidar_rt_amd", "csrc", hdr), "rb").read()).hexdigest() == want, hdr


def test_the_library_builds_and_exports_what_its_header_declares(seg_lib):
    assert os.path.exists(seg_lib) and not lrt_build.segment_is_stale()
    hdr = open(os.path.join(REPO, "include", "lrt_segment.h")).read()
    declared = set(re.findall(r"\b(lrt_seg(?:ment)?_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(sg.EXPORTS), declared ^ set(sg.EXPORTS)
    lib = sg.load()
    exported = set(re.findall(r"\blrt_seg(?:ment)?_[a-z_]+\b", subprocess.run(["nm", "-D", "--defined-only", seg_lib], capture_output=True, text=True, check=True).stdout))
    assert exported == declared, exported ^ declared
    assert lib.lrt_segment_abi_version() == int(re.search(r"#define\s+LRT_SEGMENT_ABI_VERSION\s+(\d+)", hdr).group(1)) == sg.ABI_VERSION
    for name, val in (("BLOCK", sg.BLOCK), ("NCOL", sg.NCOL), ("MAX_RH", sg.MAX_RH), ("MAX_RW", sg.MAX_RW), ("MAX_FRAMES", sg.MAX_FRAMES), ("MAX_PIXELS", sg.MAX_PIXELS),
                      ("MAX_SEGMENTS", sg.MAX_SEGMENTS), ("MAX_TRACKS", sg.MAX_TRACKS)):
        assert int(re.search(rf"#define\s+LRT_SEGMENT_{name}\s+(\d+)", hdr).group(1)) == val, name


def test_the_kernels_pass_the_resource_gate(seg_lib):
    res = resources.kernel_resources(seg_lib)
    own = sorted(n for n in res if resources.is_own_kernel(n))
    assert own == ["k_seg_accumulate", "k_seg_bounds", "k_seg_bounds_fill", "k_seg_count", "k_seg_fill", "k_seg_freespace", "k_seg_ground", "k_seg_label_flatten",
                   "k_seg_label_init", "k_seg_label_merge", "k_seg_number", "k_seg_scan"], own
    assert all(any(re.search(g_, n) for g_ in resources.GATED) for n in own)
    assert resources.violations(res) == []
    for n in own:
        r = res[n]
        assert r["vgpr_spill"] == 0 and r["scratch_bytes"] == 0 and not r["dynamic_stack"], (n, r)
    resources.check(seg_lib)


def test_argument_errors_come_before_the_device_and_launch_nothing(seg_lib):
    lib = sg.load()
    buf = (C.c_char * 8192)()
    p = (C.addressof(buf) + 255) // 256 * 256
    err = lambda: lib.lrt_segment_last_error()
    nodev = 1 << 20                                                            # a device that does not exist: what passes the checks ends there
    wb = lib.lrt_seg_work_bytes
    assert wb(0, 8, 64) < 0 and wb(1, 0, 64) < 0 and wb(1, 8, 0) < 0 and wb(3, 30000, 30000) < 0 and wb(65536, 1, 1) < 0
    assert wb(3, 5, 37) == 2 * 256 and wb(16, 64, 2048) == 2 * 4 * 16 * 512
    need = wb(1, 8, 64)

    def ground(F=1, H=8, W=64, inc=p, n_inc=2, pts=p, mask=p, up=(0.0, 0.0, 1.0), z=(-2.2, -1.4), slope=0.17, out=p):
        return lib.lrt_seg_ground(nodev, F, H, W, inc, n_inc, pts, mask, *up, *z, slope, out, None)

    def label(F=1, H=8, W=64, pts=p, mask=p, d_abs=0.15, c_h=0.01, c_v=0.01, out=p):
        return lib.lrt_seg_label(nodev, F, H, W, pts, mask, None, d_abs, c_h, c_v, out, None)

    def free(F=1, H=8, W=64, inc=p, n_inc=2, off=0.0, yaw=0.0, lo=0.0, hi=80.0, sp=p, sm=p, tr=p, tm=p, X=p, rh=1, rw=2, m_abs=0.5, m_rel=0.02, ev=p):
        return lib.lrt_seg_freespace(nodev, F, H, W, inc, n_inc, off, yaw, lo, hi, sp, sm, tr, tm, X, rh, rw, m_abs, m_rel, ev, None)

    def stats(F=1, H=8, W=64, pts=p, lab=p, s_max=16, outs=(p, p, p, p), ws=p, ws_bytes=need):
        return lib.lrt_seg_stats(nodev, F, H, W, pts, lab, None, None, s_max, *outs, ws, ws_bytes, None)

    def bounds(F=1, H=8, W=64, pts=p, seg=p, s_max=16, track_of=p, nt=2, pose=p, outs=(p, p)):
        return lib.lrt_seg_track_bounds(nodev, F, H, W, pts, seg, s_max, track_of, nt, pose, *outs, None)
    for call in (ground, label, free, stats, bounds):
        assert call(F=0) < 0 and b"0 frames of 8 x 64" in err()
        assert call(F=70000, H=1, W=1) < 0 and b"70000 frames" in err()
        assert call(pts=None) < 0 and b"null" in err() if call is not free else call(sp=None) < 0 and b"null src_points / src_mask" in err()
        assert call() < 0 and b"no HIP device" in err()
    assert ground(n_inc=3) < 0 and b"3 inclinations" in err()
    assert ground(inc=None) < 0 and b"null inclination" in err()
    assert ground(up=(0.0, 0.0, 2.0)) < 0 and b"not a unit vector" in err()
    assert ground(z=(-1.0, -2.0)) < 0 and b"height band" in err()
    assert ground(slope=-1.0) < 0 and b"slope" in err()
    assert label(d_abs=-1.0) < 0 and label(c_h=float("nan")) < 0 and b"thresholds" in err()
    assert label(out=None) < 0 and b"null points / mask / label" in err()
    assert free(off=1.0) < 0 and b"pixel offset" in err()
    assert free(yaw=float("nan")) < 0 and b"yaw" in err()
    assert free(lo=5.0, hi=5.0) < 0 and b"depths" in err()
    assert free(tm=None) < 0 and b"null tgt_range / tgt_mask" in err()
    assert free(X=None) < 0 and b"null X / ev" in err()
    assert free(rh=5) < 0 and b"a window of 5 rows" in err() and free(rw=17) < 0 and b"17 columns" in err()
    assert free(m_abs=-0.1) < 0 and b"margins" in err()
    assert stats(s_max=0) < 0 and b"a capacity of 0 segments" in err()
    assert stats(outs=(p, None, p, p)) < 0 and b"null seg / n_seg / overflow / table" in err()
    assert stats(ws=p + 8) < 0 and b"256-byte aligned" in err()
    assert stats(ws_bytes=need - 1) < 0 and (b"a workspace of %d bytes, 1 frames of 8 x 64 need %d" % (need - 1, need)) in err()
    assert bounds(nt=0) < 0 and b"0 tracks" in err()
    assert bounds(track_of=None) < 0 and b"null points / seg / track_of / pose" in err()
    assert bounds(outs=(p, None)) < 0 and b"null bounds / count" in err()


def test_the_python_side_refuses_before_it_computes():
    c = sc.label_case("odd")
    with pytest.raises(sg.SegmentationError, match="float32"):
        sg.label(c.points.double(), c.mask, **c.kw)
    with pytest.raises(sg.SegmentationError, match="mask must be"):
        sg.label(c.points, c.mask[:-1], **c.kw)
    with pytest.raises(sg.SegmentationError, match="inclination is required"):
        sg.label(c.points, c.mask)
    lab = sc.label_reference("odd")
    with pytest.raises(sg.SegmentationError, match="capacity"):
        sg.stats(c.points, lab, c.ev, 0)
    with pytest.raises(sg.SegmentationError, match="at most two"):
        sg.stats(c.points, lab, c.ev + c.ev, 16)
    with pytest.raises(sg.SegmentationError, match="must be torch.int32"):
        sg.stats(c.points, lab.long(), c.ev, 16)
    f = sc.free_case("waymo")
    with pytest.raises(sg.SegmentationError, match="window"):
        sg.freespace(f.src, f.tgt, f.X, window=(5, 2), **f.kw)
    with pytest.raises(sg.SegmentationError, match="inclination is required"):
        sg.freespace(f.src, f.tgt, f.X)
    b = sc.bounds_case()
    with pytest.raises(sg.SegmentationError, match="pose must be"):
        sg.track_bounds(b.points, b.seg, b.track_of, b.pose[:, :2])
    with pytest.raises(sg.SegmentationError, match="a workspace with tensors on cpu"):
        sg.stats(c.points, lab, c.ev, 16, workspace=torch.empty(8, dtype=torch.uint8))
