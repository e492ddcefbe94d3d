"""Actor discovery on the twins (no GPU): the analytic scenario of tests/segment_cases.py -- two moving boxes found, the parked one and the room
not -- the recorded accuracy, and the round trip through a sequence directory, `write_boxes`, the `actors` command and `ingest --discover-actors`."""
import json
import math
import os

import numpy as np
import pytest
import torch

from lidar_rt_amd import actors, ingest, sequence
from tests import segment_cases as sc

TRUE = {"A": 0, "B": 1}                                                       # scenario_boxes(k)[.]


def in_box(p_world, boxes, a, k, slack=0.0):
    """Is the world point inside actor a's box in frame index k?  (N, 3) -> (N,) bool."""
    w, z = boxes["quaternion"][a, k][0], boxes["quaternion"][a, k][3]
    yaw = 2.0 * math.atan2(z, w)
    cy, sy = math.cos(yaw), math.sin(yaw)
    d = np.atleast_2d(p_world) - boxes["translation"][a, k]
    local = np.stack([cy * d[:, 0] + sy * d[:, 1], -sy * d[:, 0] + cy * d[:, 1], d[:, 2]], 1)
    return (np.abs(local) <= 0.5 * boxes["size"][a] + slack).all(1)


@pytest.fixture(scope="module")
def found():
    boxes, report = sc.scenario_result()
    match = {}
    for name, b in TRUE.items():
        hits = [a for a in range(boxes["translation"].shape[0])
                if all(in_box(sc.scenario_boxes(k)[b][0], boxes, a, k)[0] for k in range(sc.SCENARIO["F"]) if boxes["valid"][a, k])]
        match[name] = hits
    return boxes, report, match


def test_exactly_the_two_moving_boxes_are_found(found):
    boxes, report, match = found
    assert boxes["translation"].shape[0] == 2 and report["n_actors"] == 2
    assert all(len(v) == 1 for v in match.values()) and match["A"] != match["B"], match       # one to one; C and the room produce no actor
    assert boxes["valid"].sum(1).min() >= actors.DEFAULTS["min_track"]
    assert np.array_equal(boxes["frames"], np.asarray(sc.scenario().ids))
    assert np.allclose(np.linalg.norm(boxes["quaternion"], axis=-1), 1.0) and not boxes["quaternion"][..., 1:3].any()     # roll and pitch are zero


def test_every_return_on_a_moving_box_lies_inside_its_discovered_box(found):
    boxes, _, match = found
    s = sc.scenario()
    for name, b in TRUE.items():
        a = match[name][0]
        for k, fid in enumerate(s.ids):
            if not boxes["valid"][a, k]:
                continue
            on = s.prim[fid] == 8 + b
            p = s.frames[fid][0].numpy()[on].astype(np.float64) @ s.poses[fid][:3, :3].T + s.poses[fid][:3, 3]
            inside = in_box(p, boxes, a, k)                                    # the size already holds the pad: it is the only slack
            assert inside.all(), (name, fid, int((~inside).sum()), int(on.sum()))


def test_the_parked_box_is_a_track_that_free_space_rejects(found):
    boxes, report, match = found
    min_free = report["parameters"]["min_free"]
    c_true = sc.scenario_boxes(0)[2][0]
    near = [t for t in report["tracks"] if np.linalg.norm(np.asarray(t["first_centroid"])[:2] - c_true[:2]) < 2.5 and t["length"] >= actors.DEFAULTS["min_track"]]
    assert len(near) == 1 and near[0]["dropped"] == "static" and near[0]["free_fraction"] < min_free, near
    kept = [t for t in report["tracks"] if t["dropped"] is None]
    assert len(kept) == 2 and all(t["free_fraction"] >= min_free for t in kept)


def accuracy(boxes, a, b):
    """(largest centre error, largest yaw error, largest size excess) of actor a against true box b."""
    ce = ye = 0.0
    for k in range(sc.SCENARIO["F"]):
        if boxes["valid"][a, k]:
            c, yaw = sc.scenario_boxes(k)[b]
            ce = max(ce, float(np.linalg.norm(boxes["translation"][a, k] - c)))
            got = 2.0 * math.atan2(boxes["quaternion"][a, k][3], boxes["quaternion"][a, k][0])
            ye = max(ye, abs(math.remainder(got - yaw, 2.0 * math.pi)))
    return ce, ye, float((boxes["size"][a] - sc.BOX_SIZE).max())


def test_the_accuracy_is_what_was_recorded(found):
    """Twice what the committed twin gave when the case was recorded (segment_cases.RECORDED), and nothing looser.  One box per track is the union of
    partial views around a drifting centroid: looser than a labelled box, as the module says."""
    boxes, _, match = found
    for name, b in TRUE.items():
        got = accuracy(boxes, match[name][0], b)
        print(name, "centre error %.4f m, yaw error %.4f rad, size excess %.4f m" % got)
        for g, r in zip(got, sc.RECORDED[name]):
            assert g <= 2.0 * r, (name, got, sc.RECORDED[name])


def test_the_tracker_is_greedy_by_distance_and_closes_after_the_gap():
    c = lambda x, y: np.array([x, y, 0.0])
    cands = [[(0, c(0, 0)), (1, c(5, 0))], [(0, c(1, 0)), (1, c(5, 0.1))], [], [(3, c(3, 0))], [], [], [(0, c(6, 0))]]
    tracks = actors._track(cands, len(cands), 2.0, 1)
    assert [(k, s) for k, s, _ in tracks[0]] == [(0, 0), (1, 0), (3, 3)]                     # the prediction carries it across the empty frame
    assert [(k, s) for k, s, _ in tracks[1]] == [(0, 1), (1, 1)]
    assert [(k, s) for k, s, _ in tracks[2]] == [(6, 0)] and len(tracks) == 3                # closed after more than max_gap frames: a new track


# ---- the round trip ---------------------------------------------------------------------------------------------------------------------------------------------

def scenario_frames():
    s = sc.scenario()
    return [{"id": i, "depth": s.frames[i][1], "intensity": torch.full_like(s.frames[i][1], 0.5), "mask": s.frames[i][2], "inclination": s.kw["inclination"],
             "sensor2world": s.poses[i]} for i in s.ids]


@pytest.fixture(scope="module")
def seq_dir(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("actors_seq"))
    sequence.write_sequence(root, scenario_frames(), extent=20.0)
    return root


def test_write_boxes_round_trip_and_the_command(seq_dir):
    before = json.load(open(os.path.join(seq_dir, "meta.json")))
    assert before["dynamic"] is False and before["n_actors"] == 0
    assert actors.main(["--data", seq_dir, "--sensor-height", str(sc.SENSOR_HEIGHT), "--device", "cpu"]) == 0
    meta = json.load(open(os.path.join(seq_dir, "meta.json")))
    assert meta["dynamic"] is True and meta["n_actors"] == 2 and {k: v for k, v in meta.items() if k not in ("dynamic", "n_actors")} == \
        {k: v for k, v in before.items() if k not in ("dynamic", "n_actors")}
    rep = json.load(open(os.path.join(seq_dir, "actors.json")))
    assert rep["n_actors"] == 2 and rep["format"] == actors.ACTORS_FORMAT
    seq = sequence.load_sequence(seq_dir, device="cpu")
    assert len(seq.boxes) == 2 and all(isinstance(b, sequence.TrackingBox) and len(b.frame) >= actors.DEFAULTS["min_track"] for b in seq.boxes)
    # scene_from_sequence(..., init_from_frames=True) needs a HIP device (the Gaussian assets have no CPU path): tests/test_segmentation_gpu.py runs it
    assert actors.main(["--data", seq_dir, "--sensor-height", str(sc.SENSOR_HEIGHT), "--device", "cpu"]) == 2       # refused without --force
    boxes, _ = actors.discover_sequence(seq_dir, sc.SENSOR_HEIGHT, "cpu")
    with pytest.raises(FileExistsError):
        sequence.write_boxes(seq_dir, boxes)
    sequence.write_boxes(seq_dir, boxes, force=True)
    same_as_write_sequence = str(seq_dir) + "_ws"
    sequence.write_sequence(same_as_write_sequence, scenario_frames(), extent=20.0, boxes=boxes)
    z0, z1 = np.load(os.path.join(seq_dir, "boxes.npz")), np.load(os.path.join(same_as_write_sequence, "boxes.npz"))
    assert set(z0.files) == set(z1.files) and all(np.array_equal(z0[k], z1[k]) and z0[k].dtype == z1[k].dtype for k in z0.files)
    assert json.load(open(os.path.join(same_as_write_sequence, "meta.json"))) == meta


def test_ingest_discover_actors_writes_what_the_two_steps_write(tmp_path):
    s = sc.scenario()
    pts_dir, one, two = tmp_path / "points", str(tmp_path / "one"), str(tmp_path / "two")
    pts_dir.mkdir()
    for i in s.ids:
        p, _, m = s.frames[i]
        np.save(pts_dir / f"{i}.npy", np.concatenate([p[m].numpy(), np.full((int(m.sum()), 1), 0.5, np.float32)], 1))
    np.save(tmp_path / "poses.npy", np.stack([s.poses[i] for i in s.ids]))
    common = ["--points", str(pts_dir), "--poses", str(tmp_path / "poses.npy"), "--height", str(sc.SCENARIO["H"]), "--width", str(sc.SCENARIO["W"]),
              "--inclination", *[str(v) for v in s.kw["inclination"]], "--device", "cpu"]
    assert ingest.main(common + ["--out", one, "--discover-actors", "--sensor-height", str(sc.SENSOR_HEIGHT)]) == 0
    assert ingest.main(common + ["--out", two]) == 0
    assert not os.path.exists(os.path.join(two, "boxes.npz")) and not os.path.exists(os.path.join(two, "actors.json"))      # without the flags: as ever
    assert "actors" not in json.load(open(os.path.join(two, "ingest.json")))
    assert actors.main(["--data", two, "--sensor-height", str(sc.SENSOR_HEIGHT), "--device", "cpu"]) == 0
    z1, z2 = np.load(os.path.join(one, "boxes.npz")), np.load(os.path.join(two, "boxes.npz"))
    assert set(z1.files) == set(z2.files) and z1["translation"].shape[0] == 2
    for k in z1.files:
        assert np.array_equal(z1[k], z2[k]), k
    assert json.load(open(os.path.join(one, "meta.json"))) == json.load(open(os.path.join(two, "meta.json")))
    assert json.load(open(os.path.join(one, "actors.json"))) == json.load(open(os.path.join(two, "actors.json")))
    assert ingest.main(common + ["--out", str(tmp_path / "three"), "--discover-actors"]) == 2                             # the height is required
