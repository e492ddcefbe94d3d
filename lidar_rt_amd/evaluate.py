"""``python -m lidar_rt_amd.evaluate --data DIR --ckpt CKPT [--frames test|train|all]``: the evaluation loop of zju3dv/LiDAR-RT's ``eval.py``
(:370-470) on a file-backed sequence (``lidar_rt_amd.sequence``) and a checkpoint in the reference's layout (what ``python -m lidar_rt_amd.train``
writes: ``torch.save(([12-tuple per asset], iteration), path)``, gaussian_model.py:58-72).

Renders the chosen frames forward-only through ``renderer.raytracing`` (no host synchronisation between frames: ``evaluation.render_frames``),
computes the metric set of eval.py:282-365 (depth / intensity: rmse, mae, medae, ssim, psnr; ray-drop: rmse, accuracy, F1; points: Chamfer distance
and F-score through the package's own Chamfer operator) and prints ONE JSON object ``{"iteration", "frames", "mean", "per_frame"}``; ``--out`` also
writes it to a file.  ``--unet PATH`` puts the ray-drop refinement network (``lidar_rt_amd.raydrop_refine``; a ``unet<it>.pth`` of ``python -m
lidar_rt_amd.train --refine-raydrop`` or the reference's ``unet.pth``) behind every render, as eval.py:129-144 does -- with the stored batch-norm
statistics and without dropout.  Not reproduced (``evaluation.py``): LPIPS, image dumps; the renders' point clouds are written by ``python -m lidar_rt_amd.simulate``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch


def run(args) -> dict:
    from . import evaluation, sequence, training
    if not torch.cuda.is_available():
        raise SystemExit("lidar_rt_amd.evaluate needs a HIP device (there is no CPU path)")
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    seq = sequence.load_sequence(args.data, dev, sweep=getattr(args, "sweep", "off"), sweep_fraction=getattr(args, "sweep_fraction", 1.0),
                                 sweep_ref=getattr(args, "sweep_ref", 0.5), sweep_direction=getattr(args, "sweep_direction", "cw"),
                                 actor_sweep=getattr(args, "actor_sweep", "off"))
    if getattr(args, "actor_sweep", "off") != "off":
        # the actors move within a sweep too (lidar_rt_amd.actor_sweep); --actor-twists: the twists python -m lidar_rt_amd.train --refine-actor-twist learnt
        from . import renderer
        renderer.actor_sweep = True
        sibling = os.path.join(os.path.dirname(os.path.abspath(args.ckpt)), os.path.basename(args.ckpt).replace("chkpnt", "actor_twists"))
        if not getattr(args, "actor_twists", None) and sibling != os.path.abspath(args.ckpt) and os.path.exists(sibling):
            print(f"[evaluate] note: learnt actor twists lie beside {args.ckpt}; they are used only when given with --actor-twists", file=sys.stderr, flush=True)
        if getattr(args, "actor_twists", None):
            for (a, f), v in torch.load(args.actor_twists, map_location=dev, weights_only=False)["eta"].items():
                seq.boxes[a].twist[f] = v.to(dev)
    if getattr(args, "beams", None):
        # the sensor's beam table (lidar_rt_amd.beams): what python -m lidar_rt_amd.train --refine-beams learnt, or a text table; every frame renders through it
        from . import beams as beams_mod
        rows = int(next(iter(seq.frames.depth.values())).shape[0])
        beams_mod.apply_table(seq.frames, beams_mod.load_table(args.beams, rows, dev))
    opt = training.default_options()
    scene = sequence.scene_from_sequence(seq, max_points=args.max_points, seed=args.seed)
    scene.training_setup(opt)
    model_params, iteration = torch.load(args.ckpt, map_location=dev, weights_only=False)
    scene.restore(model_params, opt)
    if args.boxes:
        # the actors' refined tracking boxes (python -m lidar_rt_amd.train --refine-boxes writes them); test frames interpolate the corrections
        from .actor_poses import ActorPoses
        if not seq.boxes:
            raise SystemExit(f"--boxes: {args.data} has no tracking boxes (boxes.npz)")
        ActorPoses.from_state_dict(seq.boxes, torch.load(args.boxes, map_location=dev, weights_only=False)).install(scene.gaussians_assets)
    refiner = None
    if getattr(args, "unet", None):
        refiner = load_refiner(args.unet, dev, spatial=not getattr(args, "unet_no_spatial", False), backend=getattr(args, "unet_backend", None))
    frames = {"test": seq.test_frames or seq.train_frames, "train": seq.train_frames, "all": sorted(set(seq.train_frames) | set(seq.test_frames))}[args.frames]
    if args.max_frames > 0:
        frames = frames[:args.max_frames]
    bg = torch.tensor([0.0, 0.0, 1.0], device=dev)          # the reference's background for (intensity, ray-hit, ray-drop): eval.py:104
    rargs = SimpleNamespace(dynamic=bool(seq.meta.get("dynamic")), opt=SimpleNamespace(use_rayhit=bool(getattr(opt, "use_rayhit", False))), pipe=SimpleNamespace())
    res = evaluation.evaluate(scene.gaussians_assets, seq.frames, frames, bg, rargs, raydrop_ratio=args.raydrop_ratio, use_gt_mask=args.use_gt_mask,
                              max_depth=args.max_depth, fused=bool(args.fused_metrics), refiner=refiner)
    return {"iteration": int(iteration), "frames": [int(f) for f in frames], "mean": res["mean"], "per_frame": {str(k): v for k, v in res["frames"].items()}}


def load_refiner(path: str, dev, spatial: bool = True, backend=None):
    """The network of a ``unet*.pth`` (a plain state_dict in the reference's names) on `dev`, packed for the HIP operator; a width that is no
    multiple of 8 is served by the module itself."""
    from . import raydrop_refine
    sd = torch.load(path, map_location="cpu", weights_only=False)
    if not isinstance(sd, dict) or "inc.conv.weight" not in sd:
        raise SystemExit(f"--unet: {path} is not a state_dict of the ray-drop refinement network")
    channels, in_channels = int(sd["inc.conv.weight"].shape[0]), int(sd["inc.conv.weight"].shape[1])
    if in_channels != (9 if spatial else 3):
        raise SystemExit(f"--unet: {path} takes {in_channels} input channels ({'without' if spatial else 'with'} --unet-no-spatial: {9 if spatial else 3})")
    net = raydrop_refine.RaydropUNet(in_channels, channels, 1)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    if channels % 8 != 0:
        if backend == "hip":
            raise SystemExit(f"--unet-backend hip: a network of {channels} channels (the operator needs a multiple of 8)")
        return net
    return raydrop_refine.pack(net, backend=backend)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m lidar_rt_amd.evaluate", description=__doc__.split("\n\n")[0])
    ap.add_argument("--data", required=True, help="sequence directory (lidar_rt_amd.sequence layout)")
    ap.add_argument("--ckpt", required=True, help="checkpoint in the reference's (model_params, iteration) layout (python -m lidar_rt_amd.train writes them)")
    ap.add_argument("--frames", choices=("test", "train", "all"), default="test", help="which frames (test falls back to train when the sequence names no test frames)")
    ap.add_argument("--max-frames", type=int, default=0)
    ap.add_argument("--raydrop-ratio", type=float, default=0.4, help="eval.py:72")
    ap.add_argument("--use-gt-mask", action="store_true", help="mask the renders with the ground-truth ray-hit mask instead of the predicted one (eval.py:184)")
    ap.add_argument("--max-depth", type=float, default=80.0)
    ap.add_argument("--max-points", type=int, default=2_000_000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--boxes", default=None, help="refined actor boxes (boxes<it>.pth of python -m lidar_rt_amd.train --refine-boxes) to render with")
    ap.add_argument("--fused-metrics", action="store_true", help="every frame's figures from the fused HIP operator (lidar_rt_amd.metrics) instead of the PyTorch expressions")
    ap.add_argument("--unet", default=None, help="state_dict of the ray-drop refinement network (unet<it>.pth of python -m lidar_rt_amd.train --refine-raydrop, or the "
                    "reference's unet.pth): every frame's ray-drop probability is replaced by the network's output before the mask is formed (eval.py:129-144)")
    ap.add_argument("--unet-backend", choices=("hip", "torch"), default=None, help="--unet: the HIP operator (liblrt_refine.so) or the module through torch; "
                    "default: lidar_rt_amd.raydrop_refine.DEFAULT_CUDA_BACKEND (torch: the faster one at 64x2048, profiles/raydrop_refine.md)")
    ap.add_argument("--unet-no-spatial", action="store_true", help="--unet: a network of 3 input channels (no ray origins and directions)")
    ap.add_argument("--sweep", choices=("off", "stored", "poses"), default="off", help="render with one pose per column (lidar_rt_amd.sweep), as python -m lidar_rt_amd.train "
                    "--sweep: stored = each frame's twist from its file, poses = twists derived from consecutive sensor poses")
    ap.add_argument("--sweep-ref", type=float, default=0.5, help="--sweep: the part of the sweep at which a frame's pose holds")
    ap.add_argument("--sweep-direction", choices=("cw", "ccw"), default="cw", help="--sweep: cw = time rises with the column index")
    ap.add_argument("--sweep-fraction", type=float, default=1.0, help="--sweep poses: the part of the time between two consecutive frame ids that one sweep takes")
    ap.add_argument("--actor-sweep", choices=("off", "stored", "boxes"), default="off", help="the actors move within a sweep too (lidar_rt_amd.actor_sweep), as "
                    "python -m lidar_rt_amd.train --actor-sweep; needs a --sweep")
    ap.add_argument("--actor-twists", default=None, help="--actor-sweep: learnt twists (actor_twists<it>.pth of python -m lidar_rt_amd.train --refine-actor-twist)")
    ap.add_argument("--beams", default=None, metavar="FILE", help="render through a beam table (lidar_rt_amd.beams): a beams<it>.pth of python -m lidar_rt_amd.train "
                    "--refine-beams, or a text table with one `eps delta` pair per image row (rad)")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args(argv)
    if args.actor_sweep != "off" and args.sweep == "off":
        ap.error("--actor-sweep needs a sweep (--sweep stored or --sweep poses)")
    if args.actor_twists and args.actor_sweep == "off":
        ap.error("--actor-twists needs --actor-sweep")
    res = run(args)
    txt = json.dumps(res)
    print(txt, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
