"""``python -m lidar_rt_amd.simulate`` end to end on the GPU: a small synthetic sequence with actors, an untrained checkpoint, and the clouds
it writes against the renders they come from, under edits, in the sensor frame through ``ingest`` and back, and as a sequence directory."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lidar_rt_amd import evaluation, ingest, sequence, simulate, training, unproject as up
from tests import unproject_cases as uc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
RATIO = 1.1                                                                  # an untrained scene's ray-drop output masks nothing
MAX_DEPTH = 80.0
H, W = 8, 64


def load_scene(data, ckpt=None):
    seq = sequence.load_sequence(data, DEV)
    opt = training.default_options()
    scene = sequence.scene_from_sequence(seq, max_points=2_000_000, seed=0)
    scene.training_setup(opt)
    if ckpt is not None:
        scene.restore(torch.load(ckpt, map_location=DEV, weights_only=False)[0], opt)
    rargs = SimpleNamespace(dynamic=bool(seq.meta.get("dynamic")), opt=SimpleNamespace(use_rayhit=bool(getattr(opt, "use_rayhit", False))), pipe=SimpleNamespace())
    return seq, scene, rargs


def render(seq, assets, rargs, ids):
    r = evaluation.render_frames(assets, seq.frames, ids, torch.tensor([0.0, 0.0, 1.0], device=DEV), rargs)
    out = {}
    for f in ids:
        depth = r[f]["depth"].squeeze(-1)
        mask = (r[f]["raydrop"].squeeze(-1) < RATIO) & torch.isfinite(depth) & (depth > 0) & (depth <= MAX_DEPTH)
        out[f] = SimpleNamespace(depth=depth, mask=mask, intensity=r[f]["intensity"].squeeze(-1), points=seq.frames.inverse_projection_with_range(f, depth, mask))
    return out


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import make_sequence
    root = tmp_path_factory.mktemp("simulate")
    data, ckpt = str(root / "seq"), str(root / "chkpnt0.pth")
    meta = make_sequence.make("kitti360_dynamic", data, n_frames=3, scale=0.02, hw=(H, W))
    assert (meta["height"], meta["width"], meta["n_actors"]) == (H, W, 8)
    seq, scene, rargs = load_scene(data)
    scene.save(0, ckpt)
    before = os.path.getmtime(ckpt), os.path.getsize(ckpt)
    run = lambda name, **kw: simulate.simulate(data, ckpt, str(root / name), frames="all", raydrop_ratio=RATIO, max_depth=MAX_DEPTH, fmt="npy", **kw)
    reports = {"plain": run("plain"), "removed": run("removed", remove_actor=[1]), "moved0": run("moved0", move_actor=[[2, 0.0, 0.0, 0.0, 0.0]]),
               "moved": run("moved", move_actor=[[2, 0.0, 3.0, 0.0, 45.0]]),
               "sensor": run("sensor", frame="sensor", sequence_dir=str(root / "rendered"), backend=None)}
    assert (os.path.getmtime(ckpt), os.path.getsize(ckpt)) == before           # the checkpoint is read, not written
    return SimpleNamespace(root=root, data=data, ckpt=ckpt, reports=reports, ids=[0, 1, 2])


def cloud(w, name, f):
    return np.load(str(w.root / name / f"{f:06d}.npy"))


def test_world_clouds_are_the_boolean_mask_expression_of_the_renders(world):
    seq, scene, rargs = load_scene(world.data, world.ckpt)
    want = render(seq, scene.gaussians_assets, rargs, world.ids)
    rep = world.reports["plain"]
    assert rep["frame"] == "world" and [f["id"] for f in rep["frames"]] == world.ids and (rep["height"], rep["width"]) == (H, W)
    total = 0
    for k, f in enumerate(world.ids):
        got = cloud(world, "plain", f)
        assert got.dtype == np.float32 and got.shape == (int(want[f].mask.sum()), 4)
        assert got[:, :3].tobytes() == want[f].points.cpu().numpy().tobytes()
        assert np.array_equal(got[:, 3], want[f].intensity[want[f].mask].cpu().numpy())
        c = rep["frames"][k]
        assert c["pixels"] == H * W == c["invalid"] + c["masked"] + c["out_of_range"] + c["points"] and c["points"] == got.shape[0] and c["masked"] == 0
        total += got.shape[0]
    assert total > 100                                                        # the untrained scene does return something
    assert json.load(open(world.root / "plain" / "simulate.json")) == json.loads(json.dumps(rep))
    poses = ingest.read_poses(str(world.root / "plain" / "poses.txt"), world.ids)
    for f in world.ids:
        assert np.array_equal(poses[f], seq.frames.pose_meta[f][1].double().cpu().numpy())
    # the torch backend writes the same bytes
    out = str(world.root / "torch")
    simulate.simulate(world.data, world.ckpt, out, frames="all", raydrop_ratio=RATIO, max_depth=MAX_DEPTH, fmt="npy", backend="torch")
    for f in world.ids:
        assert np.load(os.path.join(out, f"{f:06d}.npy")).tobytes() == cloud(world, "plain", f).tobytes()


def test_a_removed_actor_is_the_render_without_it_and_the_identity_move_changes_nothing(world):
    seq, scene, rargs = load_scene(world.data, world.ckpt)
    assets = scene.gaussians_assets
    want = render(seq, assets[:2] + assets[3:], rargs, world.ids)
    differs = 0
    for f in world.ids:
        got = cloud(world, "removed", f)
        assert got[:, :3].tobytes() == want[f].points.cpu().numpy().tobytes()
        differs += got.tobytes() != cloud(world, "plain", f).tobytes()
        assert cloud(world, "moved0", f).tobytes() == cloud(world, "plain", f).tobytes()
    assert world.reports["removed"]["edits"]["removed"] == [1] and world.reports["moved0"]["edits"]["moved"][0]["actor"] == 2
    moved = sum(cloud(world, "moved", f).tobytes() != cloud(world, "plain", f).tobytes() for f in world.ids)
    assert differs > 0 and moved > 0                                          # the edits are seen by the sensor
    with pytest.raises(simulate.SimulateError, match=r"0 \.\. 7"):
        simulate.simulate(world.data, world.ckpt, str(world.root / "bad"), remove_actor=[8])


def test_sensor_frame_clouds_come_back_through_ingest_as_the_renders(world, tmp_path):
    seq, scene, rargs = load_scene(world.data, world.ckpt)
    want = render(seq, scene.gaussians_assets, rargs, world.ids)
    inc = seq.frames.pose_meta[0][0]
    back = str(tmp_path / "back")
    rc = ingest.main(["--points", str(world.root / "sensor"), "--poses", str(world.root / "sensor" / "poses.txt"), "--out", back, "--height", str(H), "--width", str(W),
                      "--inclination", repr(float(inc[0])), repr(float(inc[1])), "--max-depth", "81", "--device", "cpu"])
    assert rc == 0
    worst = 0.0
    for f in world.ids:
        z = np.load(os.path.join(back, "frames", f"{f:06d}.npz"))
        mask = want[f].mask.cpu().numpy()
        assert np.array_equal(z["mask"], mask)
        a, b = z["depth"][mask].astype(np.float64), want[f].depth.cpu().numpy()[mask].astype(np.float64)
        e = float((np.abs(a - b) / (uc.UNIT * b)).max()) if mask.any() else 0.0
        print(f"frame {f}: round trip {e:.2f} x 2^-24 depth")
        worst = max(worst, e)
        assert np.array_equal(z["intensity"][mask], want[f].intensity.cpu().numpy()[mask])
    assert worst <= uc.BOUND, worst
    rep = json.load(open(os.path.join(back, "ingest.json")))
    assert rep["total"]["hidden"] == 0 and rep["total"]["out_of_view"] == 0 and rep["total"]["pixels"] == sum(int(want[f].mask.sum()) for f in world.ids)


def test_the_rendered_sequence_loads(world):
    seq, scene, rargs = load_scene(world.data, world.ckpt)
    want = render(seq, scene.gaussians_assets, rargs, world.ids)
    got = sequence.load_sequence(str(world.root / "rendered"), DEV)
    assert sorted(got.frames.rays) == world.ids and (got.meta["height"], got.meta["width"]) == (H, W)
    for f in world.ids:
        assert torch.equal(got.frames.get_mask(f), want[f].mask)
        assert torch.equal(got.frames.get_depth(f), want[f].depth * want[f].mask)
        assert torch.equal(got.frames.get_range_rays(f)[1], seq.frames.get_range_rays(f)[1])


def test_a_sensor_the_data_never_had(world, tmp_path):
    """Another grid, a mount and a moving sensor: the raw frame's points, six fields a row, lie at their rendered range from their own column."""
    out, rendered = str(tmp_path / "new"), str(tmp_path / "new_seq")
    table = str(tmp_path / "beams.txt")
    np.savetxt(table, np.linspace(-0.42, 0.03, 6))
    rc = simulate.main(["--data", world.data, "--ckpt", world.ckpt, "--out", out, "--frames", "all", "--raydrop-ratio", str(RATIO), "--max-depth", str(MAX_DEPTH),
                        "--height", "6", "--width", "48", "--inclination-table", table, "--mount", "0.2", "0", "0.3", "0", "0.01", "0.1", "--sweep", "poses", "--frame", "raw",
                        "--fields", "xyzirt", "--only", "background", "--sequence", rendered])
    assert rc == 0
    rep = json.load(open(os.path.join(out, "simulate.json")))
    assert (rep["height"], rep["width"], rep["frame"]) == (6, 48, "raw") and sorted(rep["twists"]) == ["0", "1", "2"] and len(rep["tau"]["0"]) == 48
    got = sequence.load_sequence(rendered, DEV, sweep="stored")
    for k, f in enumerate(world.ids):
        a = np.fromfile(os.path.join(out, f"{f:06d}.bin"), np.float32).reshape(-1, 6)
        assert a.shape[0] == rep["frames"][k]["points"] > 0 and rep["frames"][k]["pixels"] == 6 * 48
        ring, t = a[:, 4].astype(np.int64), a[:, 5]
        assert ring.min() >= 0 and ring.max() < 6 and set(np.unique(t)) <= set(np.float32(rep["tau"][str(f)]))
        depth = got.frames.get_depth(f).cpu().numpy()
        mask = got.frames.get_mask(f).cpu().numpy()
        assert int(mask.sum()) == a.shape[0]
        r = np.linalg.norm(a[:, :3].astype(np.float64), axis=1)
        assert np.abs(r - depth[mask]).max() <= 4 * uc.UNIT * MAX_DEPTH + 1e-7 * MAX_DEPTH       # in its column's frame a point's norm is its range (d is unit to 1e-7)
    assert rep["arguments"]["origin_shift"] is True
    # the plain inverses of pose, twist and tau: the same clouds up to the float32 rounding of the columns' origins (the sensor is within 2 m of the
    # world's origin here: half an ulp of 2 m is 1.2e-7 m per coordinate)
    plain = str(tmp_path / "plain")
    args = ["--data", world.data, "--ckpt", world.ckpt, "--frames", "all", "--raydrop-ratio", str(RATIO), "--max-depth", str(MAX_DEPTH), "--height", "6", "--width", "48",
            "--inclination-table", table, "--mount", "0.2", "0", "0.3", "0", "0.01", "0.1", "--sweep", "poses", "--frame", "raw", "--fields", "xyzirt", "--only", "background"]
    assert simulate.main(args + ["--out", plain, "--no-origin-shift"]) == 0
    assert json.load(open(os.path.join(plain, "simulate.json")))["arguments"]["origin_shift"] is False
    for f in world.ids:
        a = np.fromfile(os.path.join(out, f"{f:06d}.bin"), np.float32).reshape(-1, 6)
        b = np.fromfile(os.path.join(plain, f"{f:06d}.bin"), np.float32).reshape(-1, 6)
        assert a.shape == b.shape and np.array_equal(a[:, 3:], b[:, 3:]) and np.abs(a[:, :3].astype(np.float64) - b[:, :3]).max() <= 3 * 1.2e-7 + 2 * 80.0 * uc.UNIT
    assert simulate.main(["--data", world.data, "--ckpt", world.ckpt, "--out", str(tmp_path / "no"), "--frame", "raw"]) == 2
