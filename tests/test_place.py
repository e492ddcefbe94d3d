"""The place matcher without a GPU: the twins on the cases whose answer is known, the rules' header compiled for the host against the twins, the
seventeenth product library (`liblrt_place.so`), and the refusals."""
import ctypes as C
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

from lidar_rt_amd import build as lrt_build, place, resources
from tests import place_cases as pc, registration_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


# ---- 1. the twins -----------------------------------------------------------------------------------------------------------------------------------------------

def one_point(x, y, z, **kw):
    """The descriptor of a 1 x 4 frame with the point in column 0 (4 rings, 4 sectors, r in [2, 80), z_lo = -1.75, steps of 0.25 m)."""
    p = torch.zeros(1, 4, 3)
    p[0, 0] = torch.tensor([x, y, z], dtype=torch.float32)
    m = torch.tensor([[True, False, False, False]])
    rule = dict(rings=4, sectors=4, r_min=2.0, r_max=80.0, z_step=0.25)
    rule.update(kw)
    desc, total = place.describe(p, m, -1.75, **rule)
    assert int(desc.sum()) == int(total) and not desc[1:].any()
    return desc[0].tolist()


def test_the_boundaries_behave_exactly_as_the_rule_says():
    below = float(np.nextafter(np.float32(80.0), np.float32(0.0)))
    assert one_point(2.0, 0.0, -1.75) == [1, 0, 0, 0]                         # on r_min and on z_lo: kept, ring 0, value 1
    assert one_point(float(np.nextafter(np.float32(2.0), np.float32(0.0))), 0.0, 0.0) == [0, 0, 0, 0]
    assert one_point(80.0, 0.0, 0.0) == [0, 0, 0, 0]                          # on r_max: not kept
    assert one_point(below, 0.0, -1.75) == [0, 0, 0, 1]                       # just inside: the last ring
    assert one_point(0.0, -21.5, -1.5) == [0, 2, 0, 0]                        # (21.5 - 2) * 4 / 78 = 1: on a ring's edge, the outer ring; 0.25 / 0.25 = 1: value 2
    assert one_point(3.0, 0.0, float(np.nextafter(np.float32(-1.75), np.float32(-2.0)))) == [0, 0, 0, 0]      # below z_lo
    for bad in ((float("nan"), 0.0, 0.0), (3.0, float("nan"), 0.0), (3.0, 0.0, float("nan")), (float("inf"), 0.0, 0.0), (3.0, 0.0, float("inf"))):
        assert one_point(*bad) == [0, 0, 0, 0], bad                           # a NaN keeps nothing; an infinite height makes g a NaN
    assert one_point(3.0, 0.0, float("-inf")) == [0, 0, 0, 0]
    tilted = (0.0, math.sin(0.3), math.cos(0.3))                              # h and rho are taken along and across `up`
    assert one_point(0.0, 10.0 * math.cos(0.3) + 0.1 * math.sin(0.3), -10.0 * math.sin(0.3) + 0.1 * math.cos(0.3), up=tilted) == [1 + int((0.1 + 1.75) / 0.25), 0, 0, 0]
    assert one_point(0.0, 85.0 * math.cos(0.3), -85.0 * math.sin(0.3), up=tilted) == [0, 0, 0, 0]       # 85 m across `up`: beyond r_max, though |y| < 80


def test_the_value_clamps_at_255():
    assert one_point(3.0, 0.0, -1.75 + 253.0 * 0.25) == [254, 0, 0, 0]
    assert one_point(3.0, 0.0, -1.75 + 254.0 * 0.25) == [255, 0, 0, 0]
    assert one_point(3.0, 0.0, -1.75 + 255.0 * 0.25) == [255, 0, 0, 0]
    assert one_point(3.0, 0.0, 3.0e38) == [255, 0, 0, 0]
    p = torch.tensor([[[3.0, 0.0, 0.0], [3.0, 0.0, 70.0], [3.0, 0.0, 1.0], [0.0, 3.0, 1.0]]])          # a cell keeps the maximum over its pixels
    desc, total = place.describe(p, torch.ones(1, 4, dtype=torch.bool), -1.75, rings=4, sectors=2, r_min=2.0, r_max=80.0, z_step=0.25)
    assert desc[:, 0].tolist() == [255, 12] and int(total) == 267 and desc.shape == (2, 4)


def test_the_layout_is_sector_major_with_padded_rings():
    p, m = pc.frames(5, 16, 128)
    desc, sums = pc.described(5, 16, 128, *pc.ODD_GRID)
    assert desc.shape == (5, 8, 8) and desc.dtype == torch.uint8 and sums.dtype == torch.int32 and not desc[:, :, 5:].any()
    assert sums.tolist() == desc.long().sum((1, 2)).tolist()
    one, s1 = place.describe(p[3], m[3], pc.Z_LO, *pc.ODD_GRID, **pc.RULE)    # without a frame axis in, without one out; a frame does not see its neighbours
    assert torch.equal(one, desc[3]) and int(s1) == int(sums[3])
    cols = torch.arange(128)[None, :].expand(16, 128)
    for c in (0, 3, 7):                                                       # a sector is its band of columns
        sel = m[0] & (cols * 8 // 128 == c)
        only, _ = place.describe(p[0], sel, pc.Z_LO, *pc.ODD_GRID, **pc.RULE)
        assert torch.equal(only[c], desc[0, c]) and int(only.sum()) == int(desc[0, c].sum())
    assert pc.margin(5, 16, 128, 20, 60) > 1e-7 and pc.margin(9, 8, 40, 4, 8) > 1e-7 and pc.margin(1, 5, 37, 20, 30) > 1e-7


def test_an_empty_mask_gives_a_zero_descriptor_and_no_candidate():
    desc, sums = pc.described(5, 16, 128, 20, 60)
    assert not desc[2].any() and int(sums[2]) == 0 and int(sums[0]) > 0
    zeros = torch.zeros(3, 60, 20, dtype=torch.uint8)
    bd, bs = place.match(zeros, 0)
    assert bd.tolist() == [[0, -1, -1], [0, 0, -1], [0, 0, 0]] and bs.tolist() == [[0, -1, -1], [0, 0, -1], [0, 0, 0]]
    sc = place.score(bd, torch.zeros(3, dtype=torch.int32))
    assert sc[1, 0] == 1.0 and sc[2, 2] == 1.0 and math.isnan(sc[0, 1])        # 0 / 0 is defined as 1
    assert place.candidates(bd, bs, torch.zeros(3, dtype=torch.int32), top=3, max_score=1.0) == []


def test_a_yaw_is_a_shift_and_shift_to_init_maps_it_back():
    p, m = pc.column_frame()
    NR, NS, W = pc.COLUMN["NR"], pc.COLUMN["NS"], pc.COLUMN["W"]
    d_local = rc.local_directions(pc.COLUMN["H"], W, list(rc.BOUNDS), "KITTI", None).numpy().astype(np.float64)
    az = np.arctan2(d_local[..., 1], d_local[..., 0])
    assert np.abs(np.angle(np.exp(1j * (az - pc.column_azimuth(W)[None, :])))).max() < 1e-6     # the cases' columns are the ray grid's
    base, _ = place.describe(p, m, pc.Z_LO, NR, NS, **pc.RULE)
    assert int((base > 0).sum()) > 300
    for k in (1, 7, 31, 59):
        q, qm, X = pc.yawed(p, m, k)
        desc, sums = place.describe(torch.stack([p, q]), torch.stack([m, qm]), pc.Z_LO, NR, NS, **pc.RULE)
        assert torch.equal(desc[1], torch.roll(desc[0], k, 0)) and torch.equal(desc[0], base)          # rolled by k W / NS columns: rolled by k sectors
        bd, bs = place.match(desc, 1)
        assert int(bd[1, 0]) == 0 and int(bs[1, 0]) == k and int(bd[0, 0]) == -1
        assert np.abs(place.shift_to_init(k, NS) - X).max() < 1e-15                                      # X = T_j^-1 T_i, source i = the yawed frame
        assert float(place.score(bd, sums)[1, 0]) == 0.0
    assert np.array_equal(place.shift_to_init(0, NS), np.eye(4)[:3])
    up = np.array([0.0, math.sin(0.2), math.cos(0.2)])
    X = place.shift_to_init(15, 60, up)                                          # a quarter turn about a tilted axis keeps the axis
    assert np.abs(X[:, :3] @ up - up).max() < 1e-15 and abs(np.trace(X[:, :3]) - 1.0) < 1e-15 and not X[:, 3].any()


def test_two_shifts_with_equal_distance_return_the_lower():
    rng = np.random.default_rng(3)
    half = rng.integers(0, 256, size=(4, 8)).astype(np.uint8)
    a = np.concatenate([half, half])                                             # period 4 of 8 sectors: D(s) = D(s + 4)
    desc = torch.from_numpy(np.stack([a, np.roll(a, 1, 0), np.roll(a, 3, 0)]))
    bd, bs = place.match(desc, 0)
    assert bd.tolist() == [[0, -1, -1], [0, 0, -1], [0, 0, 0]] and bs.tolist() == [[0, -1, -1], [1, 0, -1], [3, 2, 0]]
    desc[2, 0, 0] ^= 1                                                           # one bit off: both shifts still tie, one above zero
    bd, bs = place.match(desc, 1)
    assert bd[2].tolist() == [1, 1, -1] and bs[2].tolist() == [3, 2, -1] and bd[1].tolist() == [0, -1, -1]


def test_candidates_take_the_lowest_scores_and_the_lower_j_on_a_tie():
    F, H, W = 9, 8, 40
    desc, sums = pc.described(F, H, W, 4, 8)
    bd, bs = pc.matched(F, H, W, 4, 8, 1)
    sc = place.score(bd, sums)
    assert np.nanmin(sc) == 0.0 and np.nanmax(sc) <= 1.0 and sc[8, 0] == 0.0 and sc[8, 4] == 1.0 and math.isnan(sc[3, 3])      # frame 8 = frame 0; frame 4 is empty
    twin = torch.cat([desc, desc[1:2]])                                          # frames 1 and 9 are equal too: query 9 ties on them
    s2 = torch.cat([sums, sums[1:2]])
    bd2, bs2 = place.match(twin, 1)
    sc2 = place.score(bd2, s2)
    got = place.candidates(bd2, bs2, s2, top=2, max_score=1.0)
    by_query = {i: [(j, s) for q, j, _, s in got if q == i] for i in range(10)}
    assert by_query[0] == [] and len(by_query[1]) == 1 and all(len(by_query[i]) == 2 for i in range(2, 10))
    assert by_query[9][0] == (1, 0) and by_query[8][0] == (0, 0)
    d = {j: sc2[3, j] for j in range(3)}
    assert [j for j, _ in by_query[3]] == sorted(d, key=lambda j: (d[j], j))[:2]
    tie = torch.zeros(3, 8, 4, dtype=torch.uint8)
    tie[:, 0, 0] = 9                                                             # three equal frames: query 2 takes candidate 0 before candidate 1
    bd3, bs3 = place.match(tie, 1)
    assert [(i, j) for i, j, _, _ in place.candidates(bd3, bs3, [9, 9, 9], top=1, max_score=0.0)] == [(1, 0), (2, 0)]
    assert place.candidates(bd2, bs2, s2, top=2, max_score=0.0) == [(8, 0, 0.0, 0), (9, 1, 0.0, 0)]
    with pytest.raises(place.PlaceError, match="top 0"):
        place.candidates(bd, bs, sums, top=0)
    with pytest.raises(place.PlaceError, match="max_score"):
        place.candidates(bd, bs, sums, max_score=1.5)
    with pytest.raises(place.PlaceError, match="an \\(F, F\\) table"):
        place.score(bd, sums[:-1])


def test_the_gap_bounds_the_triangle():
    F = 9
    for gap in (0, 1, 3, F):
        bd, bs = pc.matched(F, 8, 40, 4, 8, gap)
        i, j = np.meshgrid(np.arange(F), np.arange(F), indexing="ij")
        inside = torch.from_numpy(j + gap <= i)
        assert bool((bd[inside] >= 0).all()) and bool((bd[~inside] == -1).all()) and bool((bs[~inside] == -1).all()) and bool((bs[inside] < 8).all())
    assert bool((pc.matched(F, 8, 40, 4, 8, 0)[0].diagonal() == 0).all())


# ---- 2. the rules' header on the host -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("place_check") / "place_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "host_check", "place_check.cpp")])
    return exe


@pytest.mark.parametrize("shape,grid,gap", (((1, 5, 37), (20, 30), 0), ((5, 16, 128), (32, 128), 1), ((9, 8, 40), pc.ODD_GRID, 2), ((5, 16, 128), (20, 60), 0)))
def test_the_rule_header_on_the_host_against_the_twins(host_check, shape, grid, gap, tmp_path):
    (F, H, W), (NR, NS) = shape, grid
    p, m = pc.frames(F, H, W)
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as fh:
        fh.write(struct.pack("<8i", F, H, W, NR, NS, gap, 0, 0))
        fh.write(struct.pack("<8d", *pc.RULE["up"], pc.RULE["r_min"], pc.RULE["r_max"], pc.Z_LO, pc.RULE["z_step"], 0.0))
        fh.write(p.numpy().tobytes()); fh.write(m.numpy().astype(np.uint8).tobytes())
    res = subprocess.run([host_check, inp, out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "PLACECHECK ok" in res.stdout, res.stdout + res.stderr
    raw = open(out, "rb").read()
    NRP = place.padded(NR)
    n = F * NS * NRP
    desc = np.frombuffer(raw, np.uint8, n).reshape(F, NS, NRP)
    sums = np.frombuffer(raw, np.int32, F, n)
    bd = np.frombuffer(raw, np.int32, F * F, n + 4 * F).reshape(F, F)
    bs = np.frombuffer(raw, np.int32, F * F, n + 4 * F + 4 * F * F).reshape(F, F)
    w_desc, w_sums = pc.described(F, H, W, NR, NS)
    w_bd, w_bs = pc.matched(F, H, W, NR, NS, gap)
    assert np.array_equal(desc, w_desc.numpy()) and np.array_equal(sums, w_sums.numpy().reshape(-1))
    assert np.array_equal(bd, w_bd.numpy()) and np.array_equal(bs, w_bs.numpy())
    assert int(w_sums.sum()) > 0 and (F == 1 or int(w_bd.max()) > 0)


# ---- 3. the library -----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def place_lib():
    return lrt_build.build_place()


def test_the_library_has_a_source_list_of_its_own():
    assert lrt_build.PLACE_SOURCES == ["lrt_place.hip"]
    assert {os.path.basename(h) for h in lrt_build.PLACE_HEADERS} == {"lrt_place_math.h", "lrt_device_guard.h", "lrt_place.h"}
    others = [getattr(lrt_build, n) for n in dir(lrt_build) if n.endswith(("SOURCES", "HEADERS")) and not n.startswith("PLACE_")]
    assert len(others) >= 32 and not any("lrt_place" in f for lst in others for f in lst)
    assert os.path.basename(lrt_build.PLACE_LIB) == "liblrt_place.so" and os.path.basename(lrt_build.PLACE_STAMP) == "liblrt_place.srchash"
    assert re.fullmatch(r"[0-9a-f]{16}", lrt_build.place_source_hash())
    src = open(lrt_build.__file__).read()
    assert "build_place(force, verbose)" in src[src.index("def _build_product"):src.index("def _build_lib")]
    assert "csrc/liblrt_place.so" in open(os.path.join(REPO, "setup.py")).read() and "``csrc/liblrt_place.so``" in lrt_build.__doc__
    body = src[src.index("def build_place"):src.index("EXT_SRC =")]
    assert "CODEGEN_FLAGS" in body and "resources.check(PLACE_LIB)" in body
    mh = open(os.path.join(REPO, "lidar_rt_amd", "csrc", "lrt_place_math.h")).read()
    assert "#include \"lrt_" not in mh                                         # the rule header reads no other


def test_the_library_builds_and_exports_what_its_header_declares(place_lib):
    assert os.path.exists(place_lib) and not lrt_build.place_is_stale()
    hdr = open(os.path.join(REPO, "include", "lrt_place.h")).read()
    declared = set(re.findall(r"\b(lrt_place_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(place.EXPORTS), declared ^ set(place.EXPORTS)
    lib = place.load()
    exported = set(re.findall(r"\blrt_place_[a-z_]+\b", subprocess.run(["nm", "-D", "--defined-only", place_lib], capture_output=True, text=True, check=True).stdout))
    assert exported == declared, exported ^ declared
    assert lib.lrt_place_abi_version() == int(re.search(r"#define\s+LRT_PLACE_ABI_VERSION\s+(\d+)", hdr).group(1)) == place.ABI_VERSION
    for name, val in (("BLOCK", place.BLOCK), ("DESCRIBE_BLOCK", place.DESCRIBE_BLOCK), ("TILE", place.TILE), ("MAX_RINGS", place.MAX_RINGS),
                      ("MAX_SECTORS", place.MAX_SECTORS), ("MAX_FRAMES", place.MAX_FRAMES), ("MAX_PIXELS", place.MAX_PIXELS)):
        assert int(re.search(rf"#define\s+LRT_PLACE_{name}\s+(\d+)", hdr).group(1)) == val, name


def test_the_kernels_pass_the_resource_gate(place_lib):
    res = resources.kernel_resources(place_lib)
    own = sorted(n for n in res if resources.is_own_kernel(n))
    assert own == ["k_place_describe", "k_place_match"], own
    assert all(any(re.search(g_, n) for g_ in resources.GATED) for n in own)
    assert resources.violations(res) == []
    for n in own:
        r = res[n]
        assert r["vgpr_spill"] == 0 and r["scratch_bytes"] == 0 and not r["dynamic_stack"], (n, r)
    resources.check(place_lib)


def test_argument_errors_come_before_the_device_and_launch_nothing(place_lib):
    lib = place.load()
    buf = (C.c_char * 8192)()
    p = (C.addressof(buf) + 255) // 256 * 256
    err = lambda: lib.lrt_place_last_error()
    nodev = 1 << 20                                                            # a device that does not exist: what passes the checks ends there

    def describe(F=1, H=8, W=64, pts=p, mask=p, NR=20, NS=60, up=(0.0, 0.0, 1.0), r=(2.0, 80.0), z_lo=-1.8, z_step=0.025, desc=p, total=p):
        return lib.lrt_place_describe(nodev, F, H, W, pts, mask, NR, NS, *up, *r, z_lo, z_step, desc, total, None)

    def match(F=4, NR=20, NS=60, desc=p, gap=1, bd=p, bs=p):
        return lib.lrt_place_match(nodev, F, NR, NS, desc, gap, bd, bs, None)
    assert describe(F=0) < 0 and b"0 frames of 8 x 64" in err()
    assert describe(F=40000, H=1, W=64) < 0 and b"40000 frames" in err()
    assert describe(F=3, H=30000, W=30000) < 0 and b"F H W at most" in err()
    assert describe(NR=33) < 0 and b"33 rings x 60 sectors" in err() and describe(NR=0) < 0 and describe(NS=129, W=256) < 0 and b"129 sectors" in err()
    assert describe(NS=65) < 0 and b"65 sectors over 64 columns" in err()
    assert describe(pts=None) < 0 and b"null points / mask" in err() and describe(total=None) < 0 and b"null desc / sum" in err()
    assert describe(desc=p + 2) < 0 and b"4-byte aligned" in err()
    assert describe(up=(0.0, 0.0, 2.0)) < 0 and b"not a unit vector" in err()
    assert describe(r=(5.0, 5.0)) < 0 and b"ground range" in err() and describe(r=(-1.0, 5.0)) < 0 and describe(r=(1.0, float("inf"))) < 0
    assert describe(z_lo=float("nan")) < 0 and b"z_lo" in err()
    assert describe(z_step=0.0) < 0 and b"z_step" in err()
    assert describe() < 0 and b"no HIP device" in err()
    assert match(F=0) < 0 and b"0 frames" in err() and match(F=40000) < 0
    assert match(NS=0) < 0 and b"rings x 0 sectors" in err()
    assert match(gap=-1) < 0 and b"a gap of -1" in err()
    assert match(desc=None) < 0 and b"null desc" in err() and match(desc=p + 1) < 0 and b"4-byte aligned" in err()
    assert match(bs=None) < 0 and b"null best_d / best_s" in err()
    assert match() < 0 and b"no HIP device" in err()


def test_the_python_side_refuses_before_it_computes():
    p, m = pc.frames(1, 5, 37)
    with pytest.raises(place.PlaceError, match="float32"):
        place.describe(p.double(), m, pc.Z_LO)
    with pytest.raises(place.PlaceError, match="mask must be"):
        place.describe(p, m[:, :-1], pc.Z_LO)
    with pytest.raises(place.PlaceError, match="z_lo is required"):
        place.describe(p, m, sectors=30)
    for NR, NS in pc.GRIDS[1:]:                                                  # 60 and 128 sectors over 37 columns
        with pytest.raises(place.PlaceError, match=f"{NS} sectors over 37 columns"):
            place.describe(p, m, pc.Z_LO, NR, NS)
    with pytest.raises(place.PlaceError, match="33 rings"):
        place.describe(p, m, pc.Z_LO, 33, 8)
    with pytest.raises(place.PlaceError, match="unit vector"):
        place.describe(p, m, pc.Z_LO, 4, 8, up=(0, 0, 2))
    with pytest.raises(place.PlaceError, match="ground range"):
        place.describe(p, m, pc.Z_LO, 4, 8, r_min=3.0, r_max=3.0)
    with pytest.raises(place.PlaceError, match="z_step"):
        place.describe(p, m, pc.Z_LO, 4, 8, z_step=-1.0)
    desc, _ = pc.described(1, 5, 37, 4, 8)
    with pytest.raises(place.PlaceError, match="uint8"):
        place.match(desc.int())
    with pytest.raises(place.PlaceError, match="a multiple of 4"):
        place.match(torch.zeros(2, 8, 6, dtype=torch.uint8))
    with pytest.raises(place.PlaceError, match="gap of -2"):
        place.match(desc, -2)
    with pytest.raises(place.PlaceError, match="shift 60 of 60"):
        place.shift_to_init(60, 60)


def test_a_missing_library_is_an_error(monkeypatch, tmp_path):
    monkeypatch.setattr(place, "_lib", None)
    monkeypatch.setattr(place, "LIB_PATH", str(tmp_path / "liblrt_place.so"))
    with pytest.raises(place.PlaceError, match="is missing"):
        place.load()
