"""``python -m lidar_rt_amd.train --data DIR --iters N [--gpus N]``: the training loop of zju3dv/LiDAR-RT's ``train.py`` (:67-447) on a
file-backed sequence (``lidar_rt_amd.sequence``: range images + poses + tracking boxes in a neutral on-disk layout).

Per iteration (train.py:125-220): pick a training frame, ``training_step`` (render through ``renderer.raytracing`` -> losses -> backward ->
``scene.optimize``: Adam, densification, pruning, opacity reset), log, and every ``--save-every`` iterations write a checkpoint in the
REFERENCE's layout -- ``torch.save(([12-tuple per asset], iteration), DIR_OUT/chkpnt<iteration>.pth)`` (gaussian_model.py:58-72,
train.py:229-232) -- which ``--resume`` reads back.  ``--gpus N`` starts one process per GPU (torch.distributed over RCCL); the frame is
sharded by azimuth sector and the gradients are exchanged (``lidar_rt_amd.parallel.ShardedTracer`` behind ``renderer.sharded``): every rank
holds the full gradient and runs the same optimizer step.

What a resumed run reproduces: the parameters, the Adam moments, the densification statistics and the iteration come from the checkpoint
bit for bit; the frame order and the random draws of the densification are functions of (seed, iteration), not of process state.  The
step's float sums themselves depend on the arrival order of integer atomics inside the backward (like the reference's float atomics), so
two runs of the same iterations agree to rounding, not bit for bit.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import subprocess
import sys
import time

import torch


def frame_of(seed: int, iteration: int, frames):
    """The training frame of an iteration: a function of (seed, iteration) only, so that a resumed run sees the same sequence."""
    return frames[random.Random(seed * 1_000_003 + iteration).randrange(len(frames))]


def refine_stage(args, scene, seq, bg, dev, opt, iteration: int):
    """train.py:386-447: the ray-drop refinement network trained on detached renders of the finished Gaussians (lidar_rt_amd.raydrop_refine);
    writes unet<iteration>.pth, a plain state_dict in the reference's names, next to the checkpoint.  One process renders whole frames, with
    the recorded sensor poses (also under --refine-poses): evaluate cannot load pose corrections, so these are the renders it will refine."""
    from types import SimpleNamespace
    from . import evaluation, raydrop_refine, renderer
    rargs = SimpleNamespace(dynamic=bool(seq.meta.get("dynamic")), opt=SimpleNamespace(use_rayhit=bool(getattr(opt, "use_rayhit", False))), pipe=SimpleNamespace())
    sharded, renderer.sharded = renderer.sharded, None
    log = []
    try:
        def render_fn(frame):
            return evaluation.render_frames(scene.gaussians_assets, seq.frames, [frame], bg, rargs)[frame]
        net = raydrop_refine.train_refiner(render_fn, seq.frames, seq.train_frames, in_spatial=not args.refine_no_spatial, rot=bool(args.refine_rot),
                                           epochs=args.refine_epochs, batch=args.refine_batch, seed=args.seed, channels=args.refine_channels, device=dev, log=log)
    finally:
        renderer.sharded = sharded
    path = os.path.join(args.out, f"unet{iteration}.pth")
    torch.save({k: v.detach().cpu() for k, v in net.state_dict().items()}, path)
    print(json.dumps({"refine_raydrop": {"epochs": args.refine_epochs, "batch": args.refine_batch, "channels": args.refine_channels,
                                         "in_channels": net.in_channels, "loss_first": log[0]["loss"] if log else None,
                                         "loss_last": log[-1]["loss"] if log else None, "path": path}}), flush=True)
    return net


def run(args) -> dict:
    from . import renderer, sequence, training
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("lidar_rt_amd.train needs a HIP device (there is no CPU path)")
    single_dev = os.environ.get("LRT_SINGLE_DEVICE", "0") == "1"            # developer switch: all ranks on cuda:0 (tests on a one-GPU box)
    dev = torch.device("cuda", 0 if single_dev else local_rank)
    torch.cuda.set_device(dev)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("LRT_DIST_BACKEND", "nccl")
        # --refine-raydrop: ranks > 0 wait at the final barrier while rank 0 trains the network, for longer than the default 10 minutes
        import datetime
        slow = {"timeout": datetime.timedelta(hours=24)} if getattr(args, "refine_raydrop", False) else {}
        dist.init_process_group(backend=backend, **slow, **({"device_id": dev} if backend == "nccl" else {}))
        from .parallel import ShardedTracer
        renderer.sharded = ShardedTracer(exchange="sparse", deferred_accum=not args.exact_accum, deterministic=args.deterministic)
    renderer.deferred_accum = not args.exact_accum       # the loop reads the hit weights after loss.backward() only (train.py:156,219)
    renderer.deterministic = bool(args.deterministic)    # gradient sums in a fixed order, a forward without learnt state: a resumed run repeats the uninterrupted one bit for bit

    # --sweep: one pose per column (lidar_rt_amd.sweep); callers that build `args` themselves need not know the switches
    seq = sequence.load_sequence(args.data, dev, sweep=getattr(args, "sweep", "off"), sweep_fraction=getattr(args, "sweep_fraction", 1.0),
                                 sweep_ref=getattr(args, "sweep_ref", 0.5), sweep_direction=getattr(args, "sweep_direction", "cw"),
                                 actor_sweep=getattr(args, "actor_sweep", "off"))
    # --actor-sweep: every Gaussian of a moving actor at the instant the sweep passes over it (lidar_rt_amd.actor_sweep), in front of the fused pre-processing
    renderer.actor_sweep = getattr(args, "actor_sweep", "off") != "off"
    opt = training.default_options()
    for kv in args.opt:
        k, v = kv.split("=", 1)
        if not hasattr(opt, k):
            raise SystemExit(f"--opt {k}: not an option of lidar_rt_amd.training.default_options()")
        setattr(opt, k, type(getattr(opt, k))(float(v)) if not isinstance(getattr(opt, k), bool) else v.lower() in ("1", "true"))
    opt.fused_loss = bool(opt.fused_loss or args.fused_loss)
    opt.grid_chamfer = bool(opt.grid_chamfer or args.grid_chamfer)
    opt.sparse_adam = bool(opt.sparse_adam or args.sparse_adam)
    opt.fused_adam = bool(opt.fused_adam or args.fused_adam or opt.sparse_adam)
    opt.fused_densify = bool(getattr(opt, "fused_densify", False) or args.fused_densify)
    opt.iterations = max(opt.iterations, args.iters)
    torch.manual_seed(args.seed)
    scene = sequence.scene_from_sequence(seq, max_points=args.max_points, seed=args.seed, init_from_frames=bool(args.init_from_frames),
                                         voxel_size=args.voxel_size, k=args.init_knn)
    if args.init_from_frames and rank == 0:
        print(json.dumps({"init_from_frames": {"voxel_size": args.voxel_size, "knn": args.init_knn,
                                               "clouds": getattr(seq, "init_report", {})}}), flush=True)
    scene.training_setup(opt)
    first = 1
    sensor_poses = None
    beam_cal = None
    beam_table = None
    if getattr(args, "refine_beams", False) or getattr(args, "beams", None):
        # the sensor's beam table (lidar_rt_amd.beams): learnt through the ray gradients (--refine-beams), or read from a file and held fixed (--beams alone)
        from . import beams as beams_mod
        rows = int(seq.frames.depth[seq.train_frames[0]].shape[0])
        init = beams_mod.load_table(args.beams, rows, dev) if getattr(args, "beams", None) else None
        if getattr(args, "refine_beams", False):
            # a uniform azimuth offset is a yaw of the sensor: beside --refine-poses the table's azimuth column is kept at zero mean
            beam_cal = beams_mod.BeamCalibration(rows, init=init, lr=getattr(args, "beam_lr", 1e-4), zero_mean_azimuth=bool(args.refine_poses), device=dev)
        else:
            beam_table = init
        if not args.refine_poses:
            from .poses import SensorPoses
            sensor_poses = SensorPoses(seq.frames, seq.train_frames, beams=beam_cal if beam_cal is not None else beam_table, fixed_poses=True)
    if args.refine_poses:
        # one se(3) correction per training frame, learnt through the tracer's ray gradients (lidar_rt_amd.poses); saved beside each checkpoint
        from .poses import SensorPoses
        # --refine-twist: a moving sensor's twists are parameters too (frames loaded with --sweep carry them)
        sensor_poses = SensorPoses(seq.frames, seq.train_frames, lr_trans=args.pose_lr_trans, lr_rot=args.pose_lr_rot,
                                   refine_twist=bool(getattr(args, "refine_twist", False)), lr_twist_trans=getattr(args, "twist_lr_trans", None),
                                   lr_twist_rot=getattr(args, "twist_lr_rot", None), beams=beam_cal if beam_cal is not None else beam_table)
    box_poses = None
    if args.refine_boxes:
        # one se(3) correction per (actor, training frame) with a box, learnt through the pose-table gradient of the fused pre-processing
        # (lidar_rt_amd.actor_poses); saved beside each checkpoint.  Identical on every rank: so are the gradients it comes from
        if not seq.boxes:
            raise SystemExit(f"--refine-boxes: {args.data} has no tracking boxes (boxes.npz)")
        from .actor_poses import ActorPoses
        box_poses = ActorPoses(seq.boxes, seq.train_frames, lr_trans=args.box_lr_trans, lr_rot=args.box_lr_rot)
        box_poses.install(scene.gaussians_assets)
    actor_twists = None
    if getattr(args, "refine_actor_twist", False):
        # one twist per (actor, training frame), learnt through the gradient of the actor-sweep stage; saved beside each checkpoint
        from .actor_sweep import ActorTwists
        actor_twists = ActorTwists(seq.boxes, seq.train_frames, lr_trans=args.actor_twist_lr_trans, lr_rot=args.actor_twist_lr_rot)
    if args.resume:
        model_params, it0 = torch.load(args.resume, map_location=dev, weights_only=False)
        scene.restore(model_params, opt)
        first = int(it0) + 1
        pp = os.path.join(os.path.dirname(os.path.abspath(args.resume)), f"poses{int(it0)}.pth")
        if sensor_poses is not None and os.path.exists(pp):
            sensor_poses.load_state_dict(torch.load(pp, map_location=dev, weights_only=False))
        mp = os.path.join(os.path.dirname(os.path.abspath(args.resume)), f"beams{int(it0)}.pth")
        if beam_cal is not None and os.path.exists(mp):
            beam_cal.load(mp)
            if rank == 0:
                import hashlib
                print(json.dumps({"beams_resumed": mp, "sha256": hashlib.sha256(beam_cal.table.detach().cpu().numpy().tobytes()).hexdigest()}), flush=True)
        elif beam_cal is not None and rank == 0:                      # a checkpoint written without the switch, or copied without its sibling file
            print(f"[train] warning: --refine-beams resumes from {args.resume} but {mp} is missing: the table starts from "
                  f"{'--beams ' + args.beams if getattr(args, 'beams', None) else 'zero'} again", file=sys.stderr, flush=True)
        bp = os.path.join(os.path.dirname(os.path.abspath(args.resume)), f"boxes{int(it0)}.pth")
        if box_poses is not None and os.path.exists(bp):
            box_poses.load_state_dict(torch.load(bp, map_location=dev, weights_only=False))
        tp = os.path.join(os.path.dirname(os.path.abspath(args.resume)), f"actor_twists{int(it0)}.pth")
        if actor_twists is not None and os.path.exists(tp):
            actor_twists.load_state_dict(torch.load(tp, map_location=dev, weights_only=False))
        elif actor_twists is not None and rank == 0:                  # a checkpoint written without the switch, or copied without its sibling file
            print(f"[train] warning: --refine-actor-twist resumes from {args.resume} but {tp} is missing: the twists start from the boxes again", file=sys.stderr, flush=True)
    os.makedirs(args.out, exist_ok=True)
    bg = torch.tensor([0.0, 0.0, 1.0], device=dev)       # the reference's background for (intensity, ray-hit, ray-drop): train.py:106
    log, t0 = [], time.perf_counter()
    res = {}
    only_refine = bool(getattr(args, "only_refine", False))
    if only_refine and not args.resume:
        raise SystemExit("--only-refine needs --resume (the Gaussians it renders)")
    for it in range(first, (first - 1 if only_refine else args.iters) + 1):
        torch.manual_seed(args.seed * 1_000_003 + it)      # the densification's random draws: a function of (seed, iteration) on every rank
        frame = frame_of(args.seed, it, seq.train_frames)
        if actor_twists is not None:
            actor_twists.zero_grad()
        res = training.training_step(scene, seq.frames, frame, it, opt, bg, dynamic=bool(seq.meta.get("dynamic")), poses=sensor_poses,
                                      box_poses=box_poses, chamfer_points_detached=not args.chamfer_grad)
        if actor_twists is not None:
            actor_twists.step()
        if it % args.log_every == 0 or it == args.iters:
            row = {"iteration": it, "frame": int(frame), "loss": float(res["loss"]), "depth": float(res["depth"]), "intensity": float(res["intensity"]),
                   "raydrop": float(res["raydrop"]), "points": int(res["points"]), "seconds": round(time.perf_counter() - t0, 3)}
            log.append(row)
            if rank == 0:
                print(json.dumps(row), flush=True)
        if rank == 0 and (it % args.save_every == 0 or it == args.iters):
            scene.save(it, os.path.join(args.out, f"chkpnt{it}.pth"))
            if sensor_poses is not None and args.refine_poses:
                torch.save(sensor_poses.state_dict(), os.path.join(args.out, f"poses{it}.pth"))
            if beam_cal is not None:
                beam_cal.save(os.path.join(args.out, f"beams{it}.pth"))
            if box_poses is not None:
                torch.save(box_poses.state_dict(), os.path.join(args.out, f"boxes{it}.pth"))
            if actor_twists is not None:
                torch.save(actor_twists.state_dict(), os.path.join(args.out, f"actor_twists{it}.pth"))
    if renderer.sharded is not None:
        renderer.sharded.check(wait=True)
    elif renderer.tracer_2dgs is not None:
        renderer.tracer_2dgs.check(dev)
    torch.cuda.synchronize()
    unet = None
    if getattr(args, "refine_raydrop", False) and rank == 0:
        # after the last iteration; with --gpus N rank 0 alone runs it on whole frames while the others wait at the barrier below
        unet = refine_stage(args, scene, seq, bg, dev, opt, first - 1 if only_refine else max(args.iters, first - 1))
    if world > 1:
        import torch.distributed as dist
        dist.barrier(); dist.destroy_process_group()
    return {"log": log, "scene": scene, "sequence": seq, "last": res, "poses": sensor_poses, "boxes": box_poses, "unet": unet, "actor_twists": actor_twists, "beams": beam_cal}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m lidar_rt_amd.train", description=__doc__.split("\n\n")[0])
    ap.add_argument("--data", required=True, help="sequence directory (lidar_rt_amd.sequence layout; tools/make_sequence.py writes synthetic ones)")
    ap.add_argument("--iters", type=int, default=30_000)
    ap.add_argument("--out", default=None, help="checkpoint / log directory (default: DATA/output)")
    ap.add_argument("--gpus", type=int, default=1, help="N > 1: one process per GPU, azimuth-sharded frames, replicated optimizer")
    ap.add_argument("--resume", default=None, help="checkpoint to continue from (the reference's (model_params, iteration) tuple)")
    ap.add_argument("--save-every", type=int, default=1000)
    ap.add_argument("--log-every", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-points", type=int, default=2_000_000, help="cap of the background's initial point cloud")
    ap.add_argument("--init-from-frames", action="store_true", help="build the initial clouds DATA/init lacks from the training frames (lidar_rt_amd.scene_init: "
                    "normals from each return's k nearest returns, the returns inside a tracking box moved to that actor, the background averaged per voxel) "
                    "instead of un-oriented back-projected returns and random points in the boxes; --max-points still caps the background")
    ap.add_argument("--voxel-size", type=float, default=0.15, help="--init-from-frames: edge of the background's averaging voxels (m)")
    ap.add_argument("--init-knn", type=int, default=6, help="--init-from-frames: neighbours per normal, the return itself included (3..8)")
    ap.add_argument("--opt", action="append", default=[], help="training option name=value (lidar_rt_amd.training.default_options)")
    ap.add_argument("--exact-accum", action="store_true", help="hit weights complete at the forward (the reference's contract) instead of written by "
                    "the backward (renderer.deferred_accum, the default here: the loop reads them after the backward only)")
    ap.add_argument("--deterministic", action="store_true", help="bit-reproducible steps (Tracer(deterministic=True): the backward adds a Gaussian's records up by ray and "
                    "the pieces of long runs in order, the forward keeps no learnt tables): ~1.4 x the tracer time; a run resumed from a checkpoint then equals the "
                    "uninterrupted one bit for bit (with lambda_cd = 0, or with --grid-chamfer for lambda_cd != 0: chamfer_3DDist's backward adds with float atomics, "
                    "the grid operator's does not).  SH tables of at most 17 coefficients per "
                    "channel (sh_degree <= 3 with a table sized for it): the backward raises otherwise")
    ap.add_argument("--fused-loss", action="store_true", help="the depth / intensity / ray-drop losses and their gradient through the fused HIP operator "
                    "(lidar_rt_amd.losses.range_image_loss: three launches, no float atomics) instead of the PyTorch expression")
    ap.add_argument("--grid-chamfer", action="store_true", help="the Chamfer term (lambda_cd != 0) through the operator on the range-image grid "
                    "(lidar_rt_amd.grid_chamfer.grid_chamfer: an exact tiled search, no sort, no tree, no float atomics) instead of chamfer_3DDist on the masked points; "
                    "works with --fused-loss, --refine-poses, --refine-boxes and --gpus N (every rank computes the identical term on the gathered image)")
    ap.add_argument("--fused-adam", action="store_true", help="the optimizer step of every asset through the fused HIP operator (lidar_rt_amd.optim.GaussianAdam: "
                    "one launch for the six parameter groups, no atomics) instead of torch.optim.Adam(fused=True); same rule, same state, checkpoints move "
                    "between the two")
    ap.add_argument("--sparse-adam", action="store_true", help="implies --fused-adam: step only the Gaussians the frame hit; an unseen Gaussian keeps its parameter and "
                    "both Adam moments bit for bit (its moments do not decay, it does not coast).  An actor with a tracking box is stepped densely while "
                    "lambda_reg != 0 (the box regulariser gives every row a gradient).  Works with --gpus N (the hit mask is identical on every rank) and "
                    "keeps --deterministic's promise (no atomics, no history)")
    ap.add_argument("--fused-densify", action="store_true", help="the densification statistics and densify-and-prune of every asset through the fused HIP "
                    "operator (lidar_rt_amd.densify: one launch per asset and iteration for the statistics; an event is one decision per row and one "
                    "compaction of the asset -- four launches and one host wait) instead of the PyTorch bookkeeping; the same rule and row order, the normal "
                    "draws made up front from the iteration's seed.  Works with --fused-adam, --sparse-adam, --deterministic and --gpus N")
    ap.add_argument("--chamfer-grad", action="store_true", help="keep the predicted points of the Chamfer term differentiable (chamfer_points_detached=False); "
                    "the reference's term, and the default here, is a logged constant")
    ap.add_argument("--refine-poses", action="store_true", help="also learn a per-frame se(3) correction of the recorded sensor poses through the tracer's "
                    "ray gradients (lidar_rt_amd.poses); written as poses<it>.pth beside each checkpoint and read back by --resume")
    ap.add_argument("--pose-lr-trans", type=float, default=1e-3, help="--refine-poses: Adam learning rate of the translation part (m)")
    ap.add_argument("--pose-lr-rot", type=float, default=1e-4, help="--refine-poses: Adam learning rate of the rotation part (rad)")
    ap.add_argument("--sweep", choices=("off", "stored", "poses"), default="off", help="the sensor moves while it turns: every column of a range image gets its own "
                    "pose (lidar_rt_amd.sweep).  stored: each frame's twist (and column times) from its file; poses: twists derived from consecutive "
                    "sensor poses; off (the default): one pose per frame")
    ap.add_argument("--sweep-ref", type=float, default=0.5, help="--sweep: the part of the sweep at which a frame's pose holds (0 = its first column, 0.5 = its middle)")
    ap.add_argument("--sweep-direction", choices=("cw", "ccw"), default="cw", help="--sweep: cw = time rises with the column index (a clockwise-spinning sensor)")
    ap.add_argument("--sweep-fraction", type=float, default=1.0, help="--sweep poses: the part of the time between two consecutive frame ids that one sweep takes")
    ap.add_argument("--refine-twist", action="store_true", help="also learn every frame's twist; needs --refine-poses and a --sweep")
    ap.add_argument("--twist-lr-trans", type=float, default=1e-3, help="--refine-twist: Adam learning rate of the twists' translation part (m per sweep)")
    ap.add_argument("--twist-lr-rot", type=float, default=1e-4, help="--refine-twist: Adam learning rate of the twists' rotation part (rad per sweep)")
    ap.add_argument("--refine-beams", action="store_true", help="also learn the sensor's beam table -- an elevation and an azimuth offset per image row "
                    "(lidar_rt_amd.beams) -- through the tracer's ray gradients; alone (the recorded poses held fixed) or beside --refine-poses (the azimuth column "
                    "then keeps a zero mean: a uniform azimuth offset is a yaw); written as beams<it>.pth beside each checkpoint and read back by --resume")
    ap.add_argument("--beam-lr", type=float, default=1e-4, help="--refine-beams: Adam learning rate of the offsets (rad)")
    ap.add_argument("--beams", default=None, help="a beam table to start from (--refine-beams) or to render through as it is: a beams<it>.pth, or a text table with "
                    "one `eps delta` pair per image row (rad)")
    ap.add_argument("--actor-sweep", choices=("off", "stored", "boxes"), default="off", help="the actors move within a sweep too: every Gaussian of an actor is placed where "
                    "it is when the sweep passes over it (lidar_rt_amd.actor_sweep); needs a --sweep.  stored: the twists of the box file; boxes: twists derived from "
                    "consecutive tracking boxes (with --sweep-fraction); off (the default): every actor at its box pose of the reference instant")
    ap.add_argument("--refine-actor-twist", action="store_true", help="also learn every (actor, frame) twist; needs --actor-sweep; written as actor_twists<it>.pth beside "
                    "each checkpoint and read back by --resume")
    ap.add_argument("--actor-twist-lr-trans", type=float, default=1e-3, help="--refine-actor-twist: Adam learning rate of the translation part (m per sweep)")
    ap.add_argument("--actor-twist-lr-rot", type=float, default=1e-4, help="--refine-actor-twist: Adam learning rate of the rotation part (rad per sweep)")
    ap.add_argument("--refine-boxes", action="store_true", help="also learn a per-frame se(3) correction of every actor's tracking box through the "
                    "pose-table gradient of the fused pre-processing (lidar_rt_amd.actor_poses); written as boxes<it>.pth beside each checkpoint and "
                    "read back by --resume; works with --gpus N")
    ap.add_argument("--box-lr-trans", type=float, default=1e-3, help="--refine-boxes: Adam learning rate of the translation part (m)")
    ap.add_argument("--box-lr-rot", type=float, default=1e-4, help="--refine-boxes: Adam learning rate of the rotation part (rad)")
    ap.add_argument("--refine-raydrop", action="store_true", help="after the last iteration, train the ray-drop refinement U-Net on detached renders "
                    "(lidar_rt_amd.raydrop_refine.train_refiner, the stage of the reference's train.py:386-447) and write unet<it>.pth, a plain state_dict in the "
                    "reference's names, next to the checkpoint; python -m lidar_rt_amd.evaluate --unet reads it.  With --gpus N rank 0 alone runs it")
    ap.add_argument("--refine-epochs", type=int, default=400, help="--refine-raydrop: Adam steps")
    ap.add_argument("--refine-batch", type=int, default=16, help="--refine-raydrop: frames whose gradients are accumulated per Adam step")
    ap.add_argument("--refine-rot", action="store_true", help="--refine-raydrop: roll every frame by a random number of columns, input and labels alike")
    ap.add_argument("--refine-no-spatial", action="store_true", help="--refine-raydrop: 3 input channels (no ray origins and directions) instead of 9")
    ap.add_argument("--refine-channels", type=int, default=32, help="--refine-raydrop: width of the network (the reference's is 32; a multiple of 8 for the HIP operator)")
    ap.add_argument("--only-refine", action="store_true", help="with --resume and --refine-raydrop: skip the Gaussian loop and train the network on the checkpoint's renders")
    args = ap.parse_args(argv)
    if args.only_refine and not (args.resume and args.refine_raydrop):
        ap.error("--only-refine needs --resume and --refine-raydrop")
    if args.refine_epochs < 1 or args.refine_batch < 1:
        ap.error("--refine-epochs and --refine-batch must be positive")
    if args.refine_boxes and not os.path.exists(os.path.join(args.data, "boxes.npz")):
        ap.error(f"--refine-boxes: {args.data} has no tracking boxes (boxes.npz)")
    if not 3 <= args.init_knn <= 8:
        ap.error("--init-knn: 3 <= K <= 8")
    if not args.voxel_size > 0:
        ap.error("--voxel-size must be positive")
    if args.refine_poses and args.gpus > 1:
        ap.error("--refine-poses needs ray gradients, which azimuth sharding (--gpus > 1) does not provide")
    if (args.refine_beams or args.beams) and args.gpus > 1:
        ap.error("--refine-beams / --beams are refused with --gpus > 1, as --refine-poses is: the rays of a beam table come from the sensor model, "
                 "which azimuth sharding (--gpus > 1) does not provide")
    if not args.beam_lr > 0:
        ap.error("--beam-lr must be positive")
    if args.refine_twist and not args.refine_poses:               # so --refine-twist is refused with --gpus > 1 too: --refine-poses is, above
        ap.error("--refine-twist needs --refine-poses (the twists are learnt beside the pose corrections)")
    if args.refine_twist and args.sweep == "off":
        ap.error("--refine-twist needs a sweep (--sweep stored or --sweep poses): without one a frame has no twist")
    if args.actor_sweep != "off" and args.sweep == "off":
        ap.error("--actor-sweep needs a sweep (--sweep stored or --sweep poses): the instants are those of the sensor's columns")
    if args.refine_actor_twist and args.actor_sweep == "off":
        ap.error("--refine-actor-twist needs --actor-sweep stored or boxes: without one an actor has no twist")
    if args.refine_actor_twist and args.gpus > 1:
        ap.error("--refine-actor-twist is refused with --gpus > 1, as --refine-twist is")
    if args.exact_accum and args.deterministic:
        ap.error("--deterministic takes the hit weights from the backward (the forward's are float atomics): not with --exact-accum")
    if args.out is None:
        args.out = os.path.join(args.data, "output")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # one rank per GPU under torch.distributed.run, like bench.py --gpus N
        import socket
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        if torch.cuda.device_count() < args.gpus and os.environ.get("LRT_SINGLE_DEVICE", "0") != "1":
            print(f"[train] refusing: --gpus {args.gpus} but {torch.cuda.device_count()} visible devices", file=sys.stderr)
            return 2
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), "-m", "lidar_rt_amd.train"] + (argv if argv is not None else sys.argv[1:])
        return subprocess.call(cmd)
    run(args)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
