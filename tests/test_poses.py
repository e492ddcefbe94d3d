"""lidar_rt_amd.poses without a GPU: the SE(3) exponential, its gradient at the zero correction, the sensor duck-typing and the refusal
of frames that were added as plain rays."""
import math

import numpy as np
import pytest
import torch

from lidar_rt_amd import poses, training

KB = [math.radians(-24.9), math.radians(2.0)]


def test_se3_exp_matches_the_matrix_exponential():
    rng = np.random.default_rng(0)
    for scale in (1e-7, 1e-3, 0.3, 2.0):
        xi = torch.tensor(rng.normal(size=6) * scale, dtype=torch.float64)
        A = torch.zeros(4, 4, dtype=torch.float64)
        A[:3, :3] = poses._hat(xi[3:]); A[:3, 3] = xi[:3]
        np.testing.assert_allclose(poses.se3_exp(xi).numpy(), torch.linalg.matrix_exp(A).numpy(), rtol=1e-9, atol=1e-12)


def test_gradient_at_the_zero_correction_is_finite_and_exact():
    xi = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    w = torch.tensor(np.random.default_rng(1).normal(size=(4, 4)))
    (poses.se3_exp(xi) * w).sum().backward()
    assert torch.isfinite(xi.grad).all()
    # d Exp / d xi at 0 = the generators: rho -> translation column, phi -> hat(phi)
    want = torch.cat([w[:3, 3], torch.stack([w[2, 1] - w[1, 2], w[0, 2] - w[2, 0], w[1, 0] - w[0, 1]])])
    np.testing.assert_allclose(xi.grad.numpy(), want.numpy(), rtol=1e-12)


def _frames():
    fr = training.RangeFrames()
    s2w = torch.eye(4); s2w[:3, 3] = torch.tensor([1.0, 2.0, 0.5])
    fr.add_range_image(3, torch.ones(4, 16), torch.zeros(4, 16), torch.ones(4, 16), KB, s2w)
    o, d = training.RangeFrames.range_rays(4, 16, KB, torch.eye(4))
    fr.add_frame(5, o, d, torch.ones(4, 16), torch.zeros(4, 16), torch.ones(4, 16))
    return fr


def test_sensor_poses_start_at_the_recorded_pose_and_are_differentiable():
    fr = _frames()
    sp = poses.SensorPoses(fr, [3], lr_trans=0.01, lr_rot=0.001)
    o, d = sp.get_range_rays(3)
    o0, d0 = fr.get_range_rays(3)
    np.testing.assert_allclose(o.detach().numpy(), o0.numpy(), atol=1e-6); np.testing.assert_allclose(d.detach().numpy(), d0.numpy(), atol=1e-6)
    np.testing.assert_allclose(sp.sensor_center[3].detach().numpy(), [1.0, 2.0, 0.5], atol=1e-6)
    assert sp.get_depth(3) is fr.get_depth(3) and sp.train_frames == [3]
    (o.sum() + d[..., 0].sum()).backward()
    g = sp.xi[3].grad
    assert torch.isfinite(g).all() and g.abs().sum() > 0
    before = sp.xi[3].detach().clone()
    sp.step()
    step = (sp.xi[3].detach() - before).abs()
    # Adam's first step is lr * sign(g): the two learning rates
    np.testing.assert_allclose(step[:3][g[:3] != 0].numpy(), 0.01, rtol=1e-4)
    np.testing.assert_allclose(step[3:][g[3:] != 0].numpy(), 0.001, rtol=1e-4)
    sd = sp.state_dict()
    sp2 = poses.SensorPoses(fr, [3]); sp2.load_state_dict(sd)
    assert torch.equal(sp2.xi[3].detach(), sp.xi[3].detach()) and sp2.lr_trans == 0.01


def test_frames_added_as_plain_rays_cannot_be_refined():
    with pytest.raises(ValueError):
        poses.SensorPoses(_frames(), [3, 5])


def test_train_entry_refuses_pose_refinement_with_several_gpus():
    from lidar_rt_amd import train
    with pytest.raises(SystemExit) as e:
        train.main(["--data", "unused", "--refine-poses", "--gpus", "2"])
    assert e.value.code == 2
