"""Worker of tests/test_fused_loss_gpu.py: five `training.training_step`s with `opt.fused_loss` (incl. one densification) through `renderer.sharded`
on every rank (all on cuda:0, gloo); `opt.replica_check_interval = 1`, so every step runs `check_replicas` (it raises on every rank when the replicas'
parameters differ).  The parameters of each rank go to <out>.rank<r>.npz."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from lidar_rt_amd import scenes, training, renderer          # noqa: E402
from lidar_rt_amd.parallel import ShardedTracer               # noqa: E402


def main():
    out_path = sys.argv[1]
    dist.init_process_group(backend="gloo")
    rank = dist.get_rank()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    P, H, W = 20000, 16, 190
    sc = scenes.make_scene(P, seed=4, radius_scale=0.35)
    t = lambda a: torch.as_tensor(a, device=dev)
    asset = training.GaussianAsset.from_tensors(t(sc["means"]), t(sc["shs"][:, :1]).contiguous(), t(sc["shs"][:, 1:]).contiguous(),
                                                torch.log(t(sc["scales"])), t(sc["rotations"]), training.inverse_sigmoid(t(sc["opacities"])),
                                                max_sh_degree=3, extent=8.0)
    asset.active_sh_degree = 3
    scene = training.GaussianScene([asset])
    opt = training.default_options()
    opt.fused_loss = True
    opt.replica_check_interval = 1
    opt.densify_from_iter, opt.densification_interval, opt.densify_until_iter = 1, 3, 100
    opt.densify_grad_threshold, opt.densify_scale_threshold, opt.thresh_opa_prune = 2e-6, 0.0125, 0.03
    scene.training_setup(opt)
    frames = training.RangeFrames()
    rng = np.random.default_rng(7)
    for f in range(3):
        o, d = scenes.range_rays(H, W, (np.radians(-24.9), np.radians(2.0)), scenes.pose_matrix((0.1 * f, 0.05 * f, 0.0), yaw=0.03 * f), "KITTI")
        depth = (4.0 + 2.0 * np.sin(np.linspace(0, 6, W))[None, :] + 0.3 * rng.standard_normal((H, W))).astype(np.float32)
        inten = np.clip(0.5 + 0.2 * rng.standard_normal((H, W)), 0, 1).astype(np.float32)
        frames.add_frame(f, t(o), t(d), t(depth), t(inten), t(rng.uniform(size=(H, W)) < 0.8))
    bg = t(scenes.BG_DEFAULT)
    renderer.sharded = ShardedTracer(exchange="sparse")
    torch.manual_seed(1234)
    log = []
    for it in range(1, 6):
        r = training.training_step(scene, frames, it % 3, it, opt, bg)
        log.append([float(r["loss"]), float(r["points"])] + [float(x) for x in r["densify"]])
    renderer.sharded.check()
    pr = {n: p.detach().cpu().numpy() for n, p in asset._params().items()}
    st = asset.optimizer.state[asset._xyz]
    np.savez(out_path + f".rank{rank}.npz", log=np.asarray(log), m_xyz=st["exp_avg"].cpu().numpy(), v_xyz=st["exp_avg_sq"].cpu().numpy(), **pr)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
