"""lidar_rt_amd.actor_poses without a GPU: the stored box at the zero correction (bit for bit), the composition against a float64
restatement, the interpolation rule for frames without a learnt correction, the getter chain through an installed view, the state_dict
round trip, and the train entry's refusal of --refine-boxes on a sequence without boxes."""
import os
import subprocess
import sys

import numpy as np
import torch

from lidar_rt_amd import actor_poses, poses, training
from lidar_rt_amd.sequence import TrackingBox

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _boxes(n_actors=2, frames=range(10), seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for a in range(n_actors):
        tb = TrackingBox([4.4, 1.9, 1.6], "cpu")
        for f in frames:
            q = rng.normal(size=4).astype(np.float32) * np.float32(0.7 + 0.5 * a)        # not unit
            tb.frame[f] = (torch.tensor(rng.normal(size=3) * 10, dtype=torch.float32), torch.tensor(q).reshape(1, 4), None, None)
        out.append(tb)
    return out


def test_zero_correction_returns_the_stored_box_bit_for_bit():
    boxes = _boxes()
    ap = actor_poses.ActorPoses(boxes, [1, 4, 7])
    for a, bb in enumerate(boxes):
        for f in bb.frame:                                                   # learnt, interpolated and extrapolated frames alike
            t, q, _, _ = ap.views[a].frame[f]
            assert tuple(q.shape) == (1, 4) and tuple(t.shape) == (3,)
            assert torch.equal(t, bb.frame[f][0]) and torch.equal(q, bb.frame[f][1]), (a, f)


def _quat_of(R):
    w = 0.5 * np.sqrt(max(1.0 + np.trace(R), 0.0))
    return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])


def _qmul(a, b):
    aw, ax, ay, az = a; bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def _rot(q):
    return training._rotation_matrix(torch.tensor(np.asarray(q, np.float64)).reshape(1, 4)).squeeze(0).numpy()


def test_composition_matches_a_float64_restatement():
    boxes = _boxes(1, frames=[0])
    ap = actor_poses.ActorPoses(boxes, [0])
    rng = np.random.default_rng(3)
    for scale in (1e-6, 1e-3, 0.05, 0.4):
        xi = rng.normal(size=6) * scale
        with torch.no_grad():
            ap.xi[(0, 0)].copy_(torch.tensor(xi, dtype=torch.float32))
        t, q, _, _ = ap.views[0].frame[0]
        tb, qb = boxes[0].frame[0][0].double().numpy(), boxes[0].frame[0][1].double().numpy().reshape(4)
        xi64 = ap.xi[(0, 0)].detach().double()
        A = torch.zeros(4, 4, dtype=torch.float64); A[:3, :3] = poses._hat(xi64[3:]); A[:3, 3] = xi64[:3]
        E = torch.linalg.matrix_exp(A).numpy()
        want_t = _rot(qb) @ E[:3, 3] + tb
        want_q = _qmul(qb, _quat_of(E[:3, :3]))
        np.testing.assert_allclose(t.detach().double().numpy(), want_t, rtol=1e-6, atol=1e-6 * np.abs(want_t).max())
        np.testing.assert_allclose(q.detach().double().numpy().reshape(4), want_q, rtol=1e-6, atol=1e-6 * np.abs(want_q).max())
        # = T_box @ Exp(xi): a local point lands where the corrected box puts it
        x = rng.normal(size=3)
        T = np.eye(4); T[:3, :3] = _rot(qb); T[:3, 3] = tb
        np.testing.assert_allclose(_rot(q.detach().double().numpy().reshape(4)) @ x + t.detach().double().numpy(), (T @ E @ np.append(x, 1.0))[:3],
                                   rtol=1e-5, atol=1e-5)


def test_frames_without_a_learnt_correction_interpolate_between_the_nearest_training_frames():
    boxes = _boxes(2)
    del boxes[1].frame[5]                                                     # actor 1 has no box at training frame 5: nothing learnt there
    ap = actor_poses.ActorPoses(boxes, [2, 5, 8])
    assert sorted(ap.xi) == [(0, 2), (0, 5), (0, 8), (1, 2), (1, 8)]
    rng = np.random.default_rng(5)
    with torch.no_grad():
        for x in ap.xi.values():
            x.copy_(torch.tensor(rng.normal(size=6), dtype=torch.float32))
    X = lambda a, f: ap.xi[(a, f)].detach()
    for f in (0, 1, 2):
        assert torch.equal(ap.correction(0, f), X(0, 2))
    assert torch.equal(ap.correction(0, 9), X(0, 8)) and torch.equal(ap.correction(0, 5), X(0, 5))
    torch.testing.assert_close(ap.correction(0, 3), (2 / 3) * X(0, 2) + (1 / 3) * X(0, 5), rtol=0, atol=1e-7)
    torch.testing.assert_close(ap.correction(0, 7), (1 / 3) * X(0, 5) + (2 / 3) * X(0, 8), rtol=0, atol=1e-7)
    torch.testing.assert_close(ap.correction(1, 4), (2 / 3) * X(1, 2) + (1 / 3) * X(1, 8), rtol=0, atol=1e-7)
    # no training frame with a box at all: the stored box
    lone = _boxes(1, frames=[20, 21])
    ap2 = actor_poses.ActorPoses(lone, [2, 5])
    assert ap2.correction(0, 20) is None and torch.equal(ap2.views[0].frame[21][0], lone[0].frame[21][0])


def test_installed_view_feeds_the_getter_chain_and_carries_gradients():
    boxes = _boxes(1, frames=[0, 1])
    rng = np.random.default_rng(2)
    pts = torch.tensor(rng.normal(size=(50, 3)), dtype=torch.float32)
    asset = training.GaussianAsset.from_tensors(pts, torch.zeros(50, 1, 3), torch.zeros(50, 15, 3), torch.zeros(50, 2),
                                                torch.tensor(rng.normal(size=(50, 4)), dtype=torch.float32), torch.zeros(50, 1),
                                                bounding_box=boxes[0])
    before = asset.get_world_xyz(1).detach().clone()
    ap = actor_poses.ActorPoses(boxes, [0, 1])
    ap.install([asset])
    assert isinstance(asset.bounding_box, actor_poses.CorrectedBox)
    assert asset.bounding_box.min_xyz is boxes[0].min_xyz and 1 in asset.bounding_box.frame and 7 not in asset.bounding_box.frame
    assert torch.equal(asset.get_world_xyz(1), before)                      # zero correction: the same world positions
    obj, local = asset.get_rotation(1)
    (asset.get_world_xyz(1).sum() + obj.sum()).backward()
    g = ap.xi[(0, 1)].grad
    assert g is not None and torch.isfinite(g).all() and g.abs().sum() > 0 and ap.xi[(0, 0)].grad is None


def test_state_dict_round_trip_is_exact():
    boxes = _boxes(2)
    ap = actor_poses.ActorPoses(boxes, [1, 3, 6], lr_trans=0.02, lr_rot=0.003)
    for k in range(3):
        ap.zero_grad()
        loss = sum((ap.views[a].frame[f][0] ** 2).sum() + ap.views[a].frame[f][1].sum() for a in range(2) for f in (1, 3))
        loss.backward()
        ap.step()
    moved = ap.xi[(0, 1)].detach().clone()
    assert moved.abs().max() > 0 and torch.equal(ap.xi[(0, 6)].detach(), torch.zeros(6))      # only corrections with a gradient move
    sd = ap.state_dict()
    ap2 = actor_poses.ActorPoses(boxes, [1, 3, 6])
    ap2.load_state_dict(sd)
    assert (ap2.lr_trans, ap2.lr_rot) == (0.02, 0.003)
    for k in ap.xi:
        assert torch.equal(ap.xi[k].detach(), ap2.xi[k].detach()), k
    # the next step is the same on both: the Adam moments came along
    for p in (ap, ap2):
        p.zero_grad()
        (p.views[0].frame[1][0].sum() * 3.0).backward()
        p.step()
    for k in ap.xi:
        assert torch.equal(ap.xi[k].detach(), ap2.xi[k].detach()), k
    ap3 = actor_poses.ActorPoses.from_state_dict(boxes, ap.state_dict())
    assert all(torch.equal(ap3.xi[k].detach(), ap.xi[k].detach()) for k in ap.xi)


def test_train_refuses_refine_boxes_on_a_sequence_without_boxes(tmp_path):
    from lidar_rt_amd import sequence
    fr = {"id": 0, "depth": np.ones((4, 16), np.float32), "intensity": np.zeros((4, 16), np.float32), "mask": np.ones((4, 16), bool),
          "inclination": np.radians([-24.9, 2.0]), "sensor2world": np.eye(4)}
    sequence.write_sequence(str(tmp_path), [fr])
    r = subprocess.run([sys.executable, "-m", "lidar_rt_amd.train", "--data", str(tmp_path), "--iters", "1", "--refine-boxes"], cwd=REPO,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--refine-boxes" in r.stderr and "no tracking boxes" in r.stderr, r.stderr[-2000:]
