"""Worker for tests/test_backward_outputs_gpu.py::test_sharded_deferred_weights_of_a_second_step_with_another_hit_set: ShardedTracer with
deferred weights on backend "nccl" (RCCL) with one rank and the collective code paths forced on.  Two steps per exchange, the second from
another sensor position; its weights are compared with a fresh single-rank step.  Option zero_in_prep from env LRT_ZERO_IN_PREP."""
import json
import os
import sys

import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from lidar_rt_amd import scenes                       # noqa: E402
from lidar_rt_amd.parallel import ShardedTracer       # noqa: E402


def main():
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group(backend="nccl", device_id=dev)
    zip_ = int(os.environ.get("LRT_ZERO_IN_PREP", "2"))
    sc, o, d = scenes.s10k()
    t = {k: torch.as_tensor(v, device=dev) for k, v in sc.items()}
    ro1, rd = torch.as_tensor(o, device=dev), torch.as_tensor(d, device=dev)
    ro2 = (ro1 + torch.tensor([1.5, -1.0, 0.3], device=dev)).contiguous()      # step 2: another sensor position, another hit set
    g_up = torch.as_tensor(scenes.upstream_grad(*o.shape[:2]), device=dev)
    bg = torch.as_tensor(scenes.BG_DEFAULT, device=dev)
    args = (t["means"], t["scales"], t["rotations"], t["opacities"], t["shs"], 3, bg)

    def fresh_accum(ro):
        tr = ShardedTracer()
        tr.forward(ro, rd, *args)
        return tr.backward(*args, g_up)["accum"].clone()

    acc1, acc2 = fresh_accum(ro1), fresh_accum(ro2)
    res = {"zero_in_prep": zip_, "lost_in_step2": int(((acc1 > 0) & (acc2 == 0)).sum()), "exchanges": {}}
    for ex in ("dense", "owner", "auto"):
        tr = ShardedTracer(exchange=ex, deferred_accum=True)
        tr.force_collectives = True
        tr.backend.state.set_option("zero_in_prep", zip_)
        tr.forward(ro1, rd, *args); tr.backward(*args, g_up)
        tr.forward(ro2, rd, *args); g = tr.backward(*args, g_up)
        tr.check()
        a = g["accum"].clone()
        torch.cuda.synchronize()
        res["exchanges"][ex] = {"last_exchange": tr.last_exchange, "mask_mismatch": int(((a > 0) != (acc2 > 0)).sum()),
                                "rel_l2": float((a.double() - acc2.double()).norm() / acc2.double().norm().clamp_min(1e-30))}
    print(json.dumps(res), flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
