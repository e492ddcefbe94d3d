"""Seeded cases of the actor-sweep operator, shared by tests/test_actor_sweep.py and tests/test_actor_sweep_gpu.py.

A case is the arguments of ``actor_sweep`` as CPU tensors, upstream gradients, and the twin's forward and backward, computed once on the CPU and
left unchanged.  Every builder asserts its conditions on the TWIN: ``margin >= MARGIN`` (every evaluated column coordinate stays off its rounding
boundary, the condition under which two evaluations of the rule that differ in the last float64 bits agree on every column) and at most
``UNCONVERGED_CAP`` of the moved Gaussians unconverged.  They are conditions on the inputs, not filters: a seeded case that misses one gets
another seed (SEEDS).

The bounds (``excess``): a float32 output is within 2^-24 |twin64| + 2^-40 A of the un-rounded float64 twin, A the sum of the absolute terms of
the last sums that form it (half a float32 ulp plus float64 contraction noise); ``d_actor_twist`` within 2^-23 |twin| + 2^-34 A, A the sum of the
absolute per-Gaussian contributions (the form of tests/sweep_cases.py)."""
from types import SimpleNamespace

import numpy as np
import torch

from lidar_rt_amd import actor_sweep as asw, sweep

MARGIN = 1e-9
UNCONVERGED_CAP = 0.05
SENSOR_TWIST = (4.0, 0.3, 0.0, 0.0, 0.01, 0.05)
ACTOR_TWIST = (-3.0, 0.2, 0.0, 0.0, 0.0, 0.15)
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
COLUMNS = [64, 1030]
SEEDS = {(255, "three", 64, "waymo_yaw", "ccw"): 4, (257, "mixed", 64, "kitti", "ccw"): 4, (256, "three", 1030, "kitti", "ccw"): 4}      # seed 3 puts an
# asset where its relative motion outruns the columns (more than UNCONVERGED_CAP unconverged); every other case uses 3
WAYMO_S2E = [[0.8, -0.6, 0.0, 1.4], [0.6, 0.8, 0.0, 0.0], [0.0, 0.0, 1.0, 2.1], [0.0, 0.0, 0.0, 1.0]]      # a yaw of atan2(0.6, 0.8)
CONVENTIONS = {"kitti": dict(data_type="KITTI", sensor2ego=None), "waymo_yaw": dict(data_type="Waymo", sensor2ego=WAYMO_S2E)}


def layout(name, P):
    """(seg_start, posed (A,), moving (A,)).  "mixed": an asset boundary inside a wave, an unposed asset in the middle, an empty asset;
    "three": three moving assets (one workgroup spans them for P <= 256); "one": one asset (it spans four workgroups at P = 1000);
    "still": a posed asset with a zero twist row next to a moving one."""
    if name == "one":
        return [0, P], [True], [True]
    if name == "mixed":
        n0, n1 = (2 * P) // 5, (7 * P) // 10
        return [0, n0, n1, n1, P], [True, False, True, True], [True, True, True, True]
    if name == "three":
        return [0, P // 3, (2 * P) // 3 + 1 if P > 2 else P, P], [True, True, True], [True, True, True]
    if name == "still":
        return [0, P // 2, P], [True, True], [False, True]
    raise KeyError(name)


def random_pose(rng, centre, spread):
    q = rng.normal(size=4)
    q = q / np.linalg.norm(q) * rng.uniform(0.5, 2.0)                          # not normalised: the rule normalises
    return np.concatenate([centre + rng.uniform(-spread, spread, 3), q, [1.0]])


def sensor_pose(rng):
    yaw = rng.uniform(-np.pi, np.pi)
    c, s = np.cos(yaw), np.sin(yaw)
    T = np.eye(4)
    T[:3, :3] = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.02], [0.0, 1.0, -0.01], [-0.02, 0.01, 1.0]])
    u, _, vt = np.linalg.svd(T[:3, :3])
    T[:3, :3] = u @ vt
    T[:3, 3] = rng.uniform(-5.0, 5.0, 3) * [1.0, 1.0, 0.1]
    return T


_CACHE = {}


def case(P, lay="mixed", W=64, conv="kitti", direction="cw", seed=None, sensor_twist=SENSOR_TWIST, actor_scale=1.0, check=True):
    key = (P, lay, W, conv, direction, seed, tuple(sensor_twist) if sensor_twist is not None else None, actor_scale)
    if key in _CACHE:
        return _CACHE[key]
    sd = SEEDS.get((P, lay, W, conv, direction), 3) if seed is None else seed
    rng = np.random.default_rng([sd, P, W])
    seg, posed, moving = layout(lay, P)
    A = len(posed)
    s2w = sensor_pose(rng)
    poses, twists = [], []
    for a in range(A):
        az, r = rng.uniform(-np.pi, np.pi), rng.uniform(3.0, 60.0)
        centre = s2w[:3, 3] + np.array([r * np.cos(az), r * np.sin(az), rng.uniform(-1.0, 1.0)])
        row = random_pose(rng, centre, 0.5)
        row[7] = 1.0 if posed[a] else 0.0
        poses.append(row)
        twists.append(np.array(ACTOR_TWIST) * rng.uniform(0.3, 1.0) * rng.choice([-1.0, 1.0]) * actor_scale + rng.normal(size=6) * [0.1, 0.1, 0.02, 0.002, 0.002, 0.01] * actor_scale
                      if moving[a] else np.zeros(6))
    xyz = (rng.uniform(-1.0, 1.0, (P, 3)) * [2.2, 0.9, 0.8]).astype(np.float32)
    rot = rng.normal(size=(P, 4)).astype(np.float32)
    if P >= 64:
        rot[5] = [1e-20, -2e-20, 0.0, 1e-20]                                    # below F.normalize's eps: the clamped denominator
    xi = None if sensor_twist is None else np.array(sensor_twist) * rng.uniform(0.5, 1.0)
    c = SimpleNamespace(key=key, P=P, A=A, W=W, layout=lay, xyz=torch.tensor(xyz), rot=torch.tensor(rot), seg=torch.tensor(seg, dtype=torch.int32),
                        poses=torch.tensor(np.array(poses), dtype=torch.float32), twist=torch.tensor(np.array(twists), dtype=torch.float32),
                        sensor_pose=torch.tensor(s2w), sensor_twist=None if xi is None else torch.tensor(xi), tau=sweep.column_times(W, 0.5, direction),
                        conv=CONVENTIONS[conv], g_xyz=torch.tensor(rng.normal(size=(P, 3)), dtype=torch.float32),
                        g_rot=torch.tensor(rng.normal(size=(P, 4)), dtype=torch.float32), posed=posed, moving=moving)
    c.ref = reference(c)
    if check:
        moved, unconverged = int(c.ref.counts[0]), int(c.ref.counts[2])
        assert c.ref.margin >= MARGIN, (key, c.ref.margin)
        assert unconverged <= UNCONVERGED_CAP * moved, (key, unconverged, moved)
        assert int(c.ref.counts[0] + c.ref.counts[1]) == P
    _CACHE[key] = c
    return c


def arguments(c, dev="cpu", **over):
    """The positional and keyword arguments of actor_sweep for a case on a device (the steering arguments stay host data)."""
    d = dict(xyz=c.xyz.to(dev), rot_raw=c.rot.to(dev), seg_start=c.seg.to(dev), poses=c.poses.to(dev), actor_twist=c.twist.to(dev), sensor_pose=c.sensor_pose,
             sensor_twist=c.sensor_twist, tau=c.tau, W=c.W, **c.conv)
    d.update(over)
    return d


def _abs_hamilton(a, b):
    aw, ax, ay, az = a.abs().unbind(-1)
    bw, bx, by, bz = b.abs().unbind(-1)
    return torch.stack([aw * bw + ax * bx + ay * by + az * bz, aw * bx + ax * bw + ay * bz + az * by,
                        aw * by + ax * bz + ay * bw + az * bx, aw * bz + ax * by + ay * bx + az * bw], -1)


def reference(c):
    """The twin's forward, its float64 gradients for the case's upstream gradients, and the absolute terms of the bounds."""
    x = c.xyz.double().requires_grad_(True)
    r = c.rot.double().requires_grad_(True)
    eta = c.twist.double().requires_grad_(True)
    kw = arguments(c)
    kw.update(xyz=x, rot_raw=r, actor_twist=eta)
    t = asw.actor_sweep_reference(**kw, g_xyz=c.g_xyz, g_rot=c.g_rot)
    ((t.xyz_s * c.g_xyz.double()).sum() + (t.rot_s * c.g_rot.double()).sum()).backward()
    p, m = t.parts, t.moved
    g, h = c.g_xyz.double(), c.g_rot.double()
    zero3, zero4 = torch.zeros_like(g), torch.zeros_like(h)
    A_xyz = torch.where(m[:, None], (p.Re.abs() @ c.xyz.double().abs()[:, :, None])[:, :, 0] + p.te.abs(), zero3)
    A_rot = torch.where(m[:, None], _abs_hamilton(p.qe, p.b), zero4)
    A_dx = torch.where(m[:, None], (p.Re.abs().transpose(1, 2) @ g.abs()[:, :, None])[:, :, 0], zero3)
    db = _abs_hamilton(p.qe, h)
    clamped = p.n <= asw.NORM_EPS
    A_dr = torch.where(clamped[:, None], db / asw.NORM_EPS, (db + p.b.abs() * (p.b.abs() * db).sum(1, keepdim=True)) / p.n.clamp(min=asw.NORM_EPS)[:, None])
    A_dr = torch.where(m[:, None], A_dr, zero4)
    A_tw = torch.zeros(c.A, 6, dtype=torch.float64).index_add_(0, t.asset, t.contrib.abs())
    return SimpleNamespace(xyz_s=t.xyz_s.detach(), rot_s=t.rot_s.detach(), column=t.column, counts=t.counts, state=t.state, evals=t.evals, margin=t.margin,
                           moved=m, asset=t.asset, d_xyz=x.grad, d_rot=r.grad, d_twist=eta.grad, contrib=t.contrib, A_xyz=A_xyz, A_rot=A_rot, A_dx=A_dx,
                           A_dr=A_dr, A_tw=A_tw)


def excess(got32, ref64, A):
    """max of |got - ref| - (2^-24 |ref| + 2^-40 A): not positive when the bound of a float32 output holds (0 for an empty array)."""
    if ref64.numel() == 0:
        return 0.0
    err = (got32.detach().cpu().double() - ref64).abs()
    return float((err - (2.0 ** -24 * ref64.abs() + 2.0 ** -40 * A)).max())


def twist_excess(got32, ref64, A):
    """max of |got - ref| - (2^-23 |ref| + 2^-34 A)."""
    err = (got32.detach().cpu().double() - ref64).abs()
    return float((err - (2.0 ** -23 * ref64.abs() + 2.0 ** -34 * A)).max())


def all_cases_small():
    """The cases the host program is compared on: every size in the mixed layout, the other layouts, both column counts, conventions and directions,
    a static sensor."""
    out = [case(P, "mixed", 64) for P in SIZES]
    out += [case(255, "three", 64), case(257, "three", 1030, "waymo_yaw", "ccw"), case(1000, "one", 1030), case(256, "still", 64, "waymo_yaw"),
            case(1000, "mixed", 1030, "waymo_yaw", "ccw"), case(257, "mixed", 64, "kitti", "ccw"), case(65, "mixed", 64, sensor_twist=None)]
    return out
