"""Actor box refinement: one se(3) correction per (actor, training frame), learnt through the gradient of the fused pre-processing's pose
table (``lrt_preprocess_backward_poses``).

``ActorPoses(boxes, frame_ids)`` holds xi = (rho, phi) for every (actor, training frame) that has a box, zero-initialised.  The correction is
applied in the actor frame, ``T_box(f) @ Exp(xi)``:

    t' = R(q_box / |q_box|) t_c + t_box        (t_c = the translation column of poses.se3_exp(xi))
    q' = q_box (x) quat(Exp(phi))              (the stored, possibly non-unit, q_box: the composition the reference applies to it)

so that at xi = 0 the corrected pose is the stored one bit for bit.  ``install(assets)`` replaces each actor's ``bounding_box`` by a view
with the ``TrackingBox`` surface (``frame[ts] -> (t (3,), q (1,4), None, None)``, ``min_xyz``, ``max_xyz``): the fused path of
``renderer.raytracing`` and the getter chain (``GaussianAsset.get_world_xyz`` / ``get_rotation``) both read the corrected poses from it,
and box pruning / ``box_reg_loss`` (actor coordinates) are unchanged.  A frame without a learnt correction (a test frame) takes xi
interpolated linearly between the actor's nearest earlier and later training frames, or the nearest one at either end.
Adam with separate translation / rotation rates, ``step()`` / ``zero_grad()`` / ``state_dict()`` / ``load_state_dict()`` as
``poses.SensorPoses``.
"""
from __future__ import annotations

import bisect
import copy
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import torch

from .poses import se3_exp


def so3_quat(phi: torch.Tensor) -> torch.Tensor:
    """(3,) rotation vector -> (4,) unit quaternion (w, x, y, z) of Exp(phi); exactly (1, 0, 0, 0) at phi = 0, with the small-angle series
    below 1e-4 rad (autograd of |phi| at 0 is NaN)."""
    th2 = (phi * phi).sum()
    small = th2 < 1e-8
    th2s = torch.where(small, torch.ones_like(th2), th2)
    th = torch.sqrt(th2s)
    w = torch.where(small, 1.0 - th2 / 8.0, torch.cos(0.5 * th))
    s = torch.where(small, 0.5 - th2 / 48.0, torch.sin(0.5 * th) / th)                    # sin(t/2) / t
    return torch.cat([w.reshape(1), s * phi])


def quat_mul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """(4,) x (4,) Hamilton product, (w, x, y, z) -- quaternion_raw_multiply of the reference for one pair."""
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def _rotation(q: torch.Tensor) -> torch.Tensor:
    from .training import _rotation_matrix
    return _rotation_matrix(q.reshape(1, 4)).squeeze(0)


class ActorPoses:
    def __init__(self, boxes: Sequence, frame_ids: Iterable[int], lr_trans: float = 1e-3, lr_rot: float = 1e-4):
        self.boxes = list(boxes)
        self.frame_ids = sorted(int(f) for f in frame_ids)
        self.xi: Dict[Tuple[int, int], torch.nn.Parameter] = {}
        self._learnt: List[List[int]] = []                   # per actor: its training frames with a box, ascending
        for a, bb in enumerate(self.boxes):
            fs = [f for f in self.frame_ids if f in bb.frame]
            self._learnt.append(fs)
            for f in fs:
                self.xi[(a, f)] = torch.nn.Parameter(torch.zeros(6, dtype=torch.float32, device=bb.frame[f][0].device))
        params = list(self.xi.values())
        self.optimizer = torch.optim.Adam([{"params": params, "lr": 1.0, "name": "xi"}], betas=(0.9, 0.999), eps=1e-15) if params else None
        self.lr_trans, self.lr_rot = float(lr_trans), float(lr_rot)
        self.views = [CorrectedBox(self, a) for a in range(len(self.boxes))]

    # ---- the corrected poses ---------------------------------------------------------------------------------------------------
    def correction(self, a: int, f) -> Optional[torch.Tensor]:
        """xi of actor a at frame f: the learnt one, else interpolated between the nearest learnt frames; None without any."""
        x = self.xi.get((a, f))
        if x is not None:
            return x
        fs = self._learnt[a]
        if not fs:
            return None
        i = bisect.bisect_left(fs, f)
        if i == 0:
            return self.xi[(a, fs[0])]
        if i == len(fs):
            return self.xi[(a, fs[-1])]
        f0, f1 = fs[i - 1], fs[i]
        w = (f - f0) / (f1 - f0)
        return (1.0 - w) * self.xi[(a, f0)] + w * self.xi[(a, f1)]

    def pose(self, a: int, f) -> tuple:
        """(t (3,), q (1,4), None, None): the box of actor a at frame f composed with its correction (differentiable in xi)."""
        t, q = self.boxes[a].frame[f][:2]
        xi = self.correction(a, f)
        if xi is None:
            return (t, q, None, None)
        tc = se3_exp(xi)[:3, 3]
        t_new = t + _rotation(q.detach()) @ tc
        q_new = quat_mul(q.reshape(4), so3_quat(xi[3:])).reshape(1, 4)
        return (t_new, q_new, None, None)

    def install(self, assets) -> None:
        """Give every asset whose ``bounding_box`` is one of ``boxes`` the corrected view of it."""
        for pc in assets:
            for a, bb in enumerate(self.boxes):
                if getattr(pc, "bounding_box", None) is bb:
                    pc.bounding_box = self.views[a]

    # ---- optimisation ------------------------------------------------------------------------------------------------------------
    def zero_grad(self):
        if self.optimizer is not None:
            self.optimizer.zero_grad(set_to_none=True)

    @torch.no_grad()
    def step(self):
        """One Adam step; translation (rho) and rotation (phi) have their own learning rates (Adam's update is elementwise: a unit-rate step
        scaled per component).  Corrections without a gradient this step (actors outside the frame) stay where they are."""
        if self.optimizer is None:
            return
        live = [x for x in self.xi.values() if x.grad is not None]
        if not live:
            return
        before = [x.detach().clone() for x in live]
        self.optimizer.step()
        scale = torch.tensor([self.lr_trans] * 3 + [self.lr_rot] * 3, device=live[0].device)
        for x, b in zip(live, before):
            x.copy_(b + (x - b) * scale)

    def check_replicas(self, group=None):
        """Multi-GPU: every rank must hold the same corrections, bit for bit (the gradients they come from are identical on every rank).
        Elementwise MIN and MAX over the ranks; raises alike on every rank when they differ."""
        import torch.distributed as dist
        if not self.xi:
            return
        v = torch.stack([x.detach() for x in self.xi.values()])
        lo, hi = v.clone(), v.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=group); dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=group)
        if not bool(torch.equal(lo, hi)):
            raise RuntimeError("actor box corrections differ between ranks")

    def state_dict(self):
        return {"xi": {k: x.detach().cpu().clone() for k, x in self.xi.items()}, "frame_ids": list(self.frame_ids),
                # a copy: Adam's state_dict shares its step counters with the live optimiser
                "optimizer": None if self.optimizer is None else copy.deepcopy(self.optimizer.state_dict()), "lr_trans": self.lr_trans,
                "lr_rot": self.lr_rot}

    def load_state_dict(self, sd):
        if set(sd["xi"]) != set(self.xi):
            raise ValueError(f"ActorPoses.load_state_dict: the file holds corrections for {len(sd['xi'])} (actor, frame) pairs, this object "
                             f"{len(self.xi)}; they must be the same pairs (same boxes and training frames)")
        with torch.no_grad():
            for k, x in sd["xi"].items():
                self.xi[k].copy_(x.to(self.xi[k].device))
        if self.optimizer is not None and sd.get("optimizer") is not None:
            self.optimizer.load_state_dict(sd["optimizer"])
        self.lr_trans, self.lr_rot = float(sd["lr_trans"]), float(sd["lr_rot"])

    @classmethod
    def from_state_dict(cls, boxes: Sequence, sd) -> "ActorPoses":
        self = cls(boxes, sd["frame_ids"], sd["lr_trans"], sd["lr_rot"])
        self.load_state_dict(sd)
        return self


class CorrectedBox:
    """The ``TrackingBox`` surface of one actor with its corrections applied: ``frame[ts]``, ``min_xyz``, ``max_xyz``."""

    def __init__(self, poses: ActorPoses, a: int):
        self.poses, self.a, self.box = poses, a, poses.boxes[a]
        self.min_xyz, self.max_xyz = self.box.min_xyz, self.box.max_xyz
        self.twist = getattr(self.box, "twist", {})                # the actor's motion within a sweep (lidar_rt_amd.actor_sweep): the box's own dict
        self.frame = _CorrectedFrames(self)


class _CorrectedFrames:
    def __init__(self, view: CorrectedBox):
        self.v = view

    def __contains__(self, ts):
        return ts in self.v.box.frame

    def __getitem__(self, ts):
        return self.v.poses.pose(self.v.a, ts)

    def __iter__(self):
        return iter(self.v.box.frame)

    def __len__(self):
        return len(self.v.box.frame)

    def keys(self):
        return self.v.box.frame.keys()
