"""Sensor pose refinement: one se(3) correction per frame, learnt through the tracer's ray gradients (lrt_backward_rays).

``SensorPoses(frames, frame_ids)`` holds xi = (rho, phi) per frame, zero-initialised; the corrected pose is ``sensor2world @ Exp(xi)``
(a correction in the sensor frame).  The rays are rebuilt from it by ``RangeFrames.range_rays`` -- differentiable torch -- so that
``loss.backward()`` carries dL/dray_o and dL/dray_d from the tracer back to xi.  The object is duck-typed as a sensor for
``renderer.raytracing`` (``get_range_rays``, ``sensor_center``, ``inverse_projection_with_range``, the ground-truth accessors of
``frames``) and brings its own Adam optimiser with separate translation / rotation learning rates (``step()`` / ``zero_grad()``).

A frame with sweep rays (``RangeFrames.sweep_meta``: a moving sensor, one pose per column) gets its rays from
``sweep.sweep_rays(sensor2world @ Exp(xi), twist, ...)`` -- the fused operator, four launches forward and backward instead of the torch
expression's dozens.  ``refine_twist=True`` makes those frames' twists parameters too, with learning rates of their own.

``beams=`` (a ``beams.BeamCalibration``, or a fixed ``(H, 2)`` tensor that is read detached) puts the sensor's beam table into the rays: every
frame's rays then come from ``beams.beam_rays`` -- with the frame's twist, or ``None`` for a static frame -- and a ``BeamCalibration`` is zeroed
and stepped with the poses.  ``fixed_poses=True`` holds the recorded poses as they are (no ``xi`` parameters), so that a table can be learnt
alone.  Without ``beams`` and ``fixed_poses`` nothing here changes.
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional

import torch


def _hat(v: torch.Tensor) -> torch.Tensor:
    z = torch.zeros((), dtype=v.dtype, device=v.device)
    return torch.stack([torch.stack([z, -v[2], v[1]]), torch.stack([v[2], z, -v[0]]), torch.stack([-v[1], v[0], z])])


def se3_exp(xi: torch.Tensor) -> torch.Tensor:
    """(6,) xi = (rho, phi) -> (4, 4) SE(3) matrix.  Rodrigues with the small-angle series below 1e-4 rad: autograd of |phi| at exactly
    phi = 0 is NaN, and the zero-initialised corrections start there."""
    rho, phi = xi[:3], xi[3:]
    th2 = (phi * phi).sum()
    small = th2 < 1e-8
    th2s = torch.where(small, torch.ones_like(th2), th2)                  # keeps the unused branch finite (and its gradient)
    th = torch.sqrt(th2s)
    A = torch.where(small, 1.0 - th2 / 6.0, torch.sin(th) / th)                             # sin t / t
    B = torch.where(small, 0.5 - th2 / 24.0, (1.0 - torch.cos(th)) / th2s)                  # (1 - cos t) / t^2
    C = torch.where(small, 1.0 / 6.0 - th2 / 120.0, (th - torch.sin(th)) / (th2s * th))     # (t - sin t) / t^3
    K = _hat(phi)
    I = torch.eye(3, dtype=xi.dtype, device=xi.device)
    K2 = K @ K
    R = I + A * K + B * K2
    V = I + B * K + C * K2
    top = torch.cat([R, (V @ rho).unsqueeze(1)], 1)
    bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=xi.dtype, device=xi.device)
    return torch.cat([top, bottom], 0)


class SensorPoses:
    def __init__(self, frames, frame_ids: Optional[Iterable[int]] = None, lr_trans: float = 1e-3, lr_rot: float = 1e-3, refine_twist: bool = False,
                 lr_twist_trans: Optional[float] = None, lr_twist_rot: Optional[float] = None, beams=None, fixed_poses: bool = False):
        meta = getattr(frames, "pose_meta", {})
        ids = list(frame_ids) if frame_ids is not None else list(frames.train_frames)
        for f in ids:
            if f not in meta:
                raise ValueError(f"SensorPoses: frame {f} was added as plain rays (RangeFrames.add_frame); only frames added with "
                                 "add_range_image (inclination + sensor2world) can be refined")
        self.frames = frames
        self.frame_ids = ids
        dev = frames.depth[ids[0]].device if ids else torch.device("cpu")
        self.fixed_poses = bool(fixed_poses)
        self.xi: Dict[int, torch.nn.Parameter] = {} if self.fixed_poses else {f: torch.nn.Parameter(torch.zeros(6, dtype=torch.float32, device=dev)) for f in ids}
        groups = [] if self.fixed_poses else [{"params": list(self.xi.values()), "lr": 1.0, "name": "xi"}]
        # frames with sweep rays (RangeFrames.sweep_meta): their motion over the sweep, a parameter too under refine_twist
        sweep_meta = getattr(frames, "sweep_meta", {})
        self.refine_twist = bool(refine_twist)
        self.twist: Dict[int, torch.Tensor] = {}
        self._sweep_args: Dict[int, tuple] = {}               # per sweep frame: what sweep_rays needs besides pose and twist, made once
        for f in ids:
            if f in sweep_meta:
                tw, tau = sweep_meta[f]
                tw = tw.detach().to(device=dev, dtype=torch.float32).clone()
                self.twist[f] = torch.nn.Parameter(tw) if self.refine_twist else tw
        if self.refine_twist:
            if not self.twist:
                raise ValueError("SensorPoses: refine_twist needs frames with sweep rays (add_range_image(..., twist=...)); none of the frames has a twist")
            groups.append({"params": list(self.twist.values()), "lr": 1.0, "name": "twist"})
        self.optimizer = torch.optim.Adam(groups, betas=(0.9, 0.999), eps=1e-15) if groups else None      # fixed poses, fixed twists: nothing of its own to step
        # the sensor's beam table (lidar_rt_amd.beams): a BeamCalibration that learns with the poses, or a fixed (H, 2) tensor
        self.beams = beams
        if beams is not None:
            from .beams import BeamCalibration, BeamError
            table = beams.table if isinstance(beams, BeamCalibration) else beams
            for f in ids:
                H = frames.depth[f].shape[0]
                if not torch.is_tensor(table) or tuple(table.shape) != (H, 2) or table.dtype != torch.float32 or table.device != dev:
                    raise BeamError(f"SensorPoses: beams must be a BeamCalibration or an ({H}, 2) float32 tensor on {dev} (frame {f} has {H} rows; it is "
                                    f"{(tuple(table.shape), table.dtype, str(table.device)) if torch.is_tensor(table) else type(table).__name__})")
        self.lr_trans, self.lr_rot = float(lr_trans), float(lr_rot)
        self.lr_twist_trans = float(lr_trans if lr_twist_trans is None else lr_twist_trans)
        self.lr_twist_rot = float(lr_rot if lr_twist_rot is None else lr_twist_rot)

    # ---- the corrected poses ---------------------------------------------------------------------------------------------------
    def sensor2world(self, frame) -> torch.Tensor:
        """(4, 4) corrected pose, differentiable in xi[frame]."""
        inc, s2w, _, _ = self.frames.pose_meta[frame]
        if self.fixed_poses:
            return s2w.to(torch.float32)
        return s2w.to(torch.float32) @ se3_exp(self.xi[frame])

    def _sweep(self, frame):
        a = self._sweep_args.get(frame)
        if a is None:
            inc, s2w, data_type, s2e = self.frames.pose_meta[frame]
            H, W = self.frames.depth[frame].shape[:2]
            dev = s2w.device
            s2e_host = None
            if data_type == "Waymo" and s2e is not None:
                s2e_host = torch.as_tensor(s2e).detach().to("cpu", torch.float32)       # read back once, not per iteration
            inc = [-float(inc), float(inc)] if isinstance(inc, (int, float)) else inc
            inc_t = torch.as_tensor(inc, dtype=torch.float32).reshape(-1).to(dev)
            tau = self.frames.sweep_meta[frame][1].to(device=dev, dtype=torch.float32) if frame in self.twist else None    # a static frame (beams only)
            a = (H, W, inc_t, data_type, s2e_host, tau)
            self._sweep_args[frame] = a
        return a

    def get_range_rays(self, frame):
        inc, s2w, data_type, s2e = self.frames.pose_meta[frame]
        H, W = self.frames.depth[frame].shape[:2]
        if self.beams is not None:                                # the sensor's own beam table: the fused operator, moving or not
            from . import beams as bm
            table = self.beams.table if isinstance(self.beams, bm.BeamCalibration) else self.beams.detach()
            H, W, inc_t, data_type, s2e_host, tau = self._sweep(frame)
            return bm.beam_rays(self.sensor2world(frame), self.twist.get(frame), H, W, inc_t, table, data_type, s2e_host, tau=tau)
        if frame in self.twist:                                   # a moving sensor: one pose per column, through the fused operator
            from . import sweep
            H, W, inc_t, data_type, s2e_host, tau = self._sweep(frame)
            return sweep.sweep_rays(self.sensor2world(frame), self.twist[frame], H, W, inc_t, data_type, s2e_host, tau=tau)
        return self.frames.range_rays(H, W, inc, self.sensor2world(frame), data_type, s2e)

    @property
    def sensor_center(self):
        return _Centers(self)

    def inverse_projection_with_range(self, frame, range_map, mask=None):
        o, d = self.get_range_rays(frame)
        pts = (o + d * range_map.reshape(*d.shape[:2], 1)).reshape(-1, 3)
        if mask is None:
            return pts.index_select(0, self.frames.mask_index[frame])
        return pts[mask.reshape(-1).bool()]

    # the ground truth: the frames' own
    train_frames = property(lambda s: s.frame_ids)
    get_depth = lambda s, f: s.frames.get_depth(f)
    get_intensity = lambda s, f: s.frames.get_intensity(f)
    get_mask = lambda s, f: s.frames.get_mask(f)
    mask_index = property(lambda s: s.frames.mask_index)

    # ---- optimisation ------------------------------------------------------------------------------------------------------------
    def _calibration(self):
        return self.beams if self.beams is not None and hasattr(self.beams, "step") else None

    def zero_grad(self):
        if self.optimizer is not None:
            self.optimizer.zero_grad(set_to_none=True)
        if self._calibration() is not None:
            self.beams.zero_grad()

    @torch.no_grad()
    def step(self):
        """One Adam step; the translation (rho) and rotation (phi) parts of xi have their own learning rates (Adam's update is
        elementwise, so scaling a unit-rate step per component is exactly two learning rates), and so have the twists' under refine_twist."""
        if self._calibration() is not None:
            self.beams.step()
        if self.optimizer is None:
            return
        params = dict(self.xi)
        twists = {f: x for f, x in self.twist.items()} if self.refine_twist else {}
        before = {f: x.detach().clone() for f, x in params.items()}
        before_tw = {f: x.detach().clone() for f, x in twists.items()}
        self.optimizer.step()
        dev = next(iter(list(self.xi.values()) + list(twists.values()))).device
        scale = torch.tensor([self.lr_trans] * 3 + [self.lr_rot] * 3, device=dev)
        for f, x in params.items():
            x.copy_(before[f] + (x - before[f]) * scale)
        if twists:
            scale_tw = torch.tensor([self.lr_twist_trans] * 3 + [self.lr_twist_rot] * 3, device=dev)
            for f, x in twists.items():
                x.copy_(before_tw[f] + (x - before_tw[f]) * scale_tw)

    def state_dict(self):
        sd = {"xi": {f: x.detach().cpu() for f, x in self.xi.items()}, "optimizer": None if self.optimizer is None else self.optimizer.state_dict(),
              "lr_trans": self.lr_trans, "lr_rot": self.lr_rot}
        if self.twist:
            sd.update(twist={f: x.detach().cpu() for f, x in self.twist.items()}, refine_twist=self.refine_twist,
                      lr_twist_trans=self.lr_twist_trans, lr_twist_rot=self.lr_twist_rot)
        return sd

    def load_state_dict(self, sd):
        with torch.no_grad():
            for f, x in sd["xi"].items():
                if not self.fixed_poses:                                # held fixed here: saved corrections are not applied
                    self.xi[f].copy_(x.to(self.xi[f].device))
            for f, x in sd.get("twist", {}).items():                    # a state dict from before the twists (or of static frames) has none
                if f in self.twist:
                    self.twist[f].copy_(x.to(self.twist[f].device))
        self.lr_trans, self.lr_rot = float(sd["lr_trans"]), float(sd["lr_rot"])
        self.lr_twist_trans = float(sd.get("lr_twist_trans", self.lr_twist_trans))
        self.lr_twist_rot = float(sd.get("lr_twist_rot", self.lr_twist_rot))
        if self.optimizer is None or sd["optimizer"] is None:       # nothing stepped on one side: there are no moments to carry over
            return
        groups = len(sd["optimizer"]["param_groups"])
        if groups == len(self.optimizer.param_groups):
            self.optimizer.load_state_dict(sd["optimizer"])
        elif groups == 1 and self.refine_twist:
            # saved without twists: the xi group's moments are restored, the twists start fresh
            xi_only = torch.optim.Adam([self.optimizer.param_groups[0]], betas=(0.9, 0.999), eps=1e-15)
            xi_only.load_state_dict(sd["optimizer"])
            for p in self.optimizer.param_groups[0]["params"]:
                if p in xi_only.state:
                    self.optimizer.state[p] = xi_only.state[p]
        else:
            raise ValueError(f"SensorPoses: the state dict's optimizer has {groups} parameter groups, this one {len(self.optimizer.param_groups)}")


class _Centers:
    """``sensor_center[frame]``: the corrected sensor position."""

    def __init__(self, poses: SensorPoses):
        self.p = poses

    def __getitem__(self, frame):
        return self.p.sensor2world(frame)[:3, 3]
