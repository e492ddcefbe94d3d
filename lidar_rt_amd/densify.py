"""Adaptive density control of one Gaussian asset as one decision per row and one compaction (``opt.fused_densify``): what
``GaussianAsset.add_densification_stats`` and ``GaussianAsset.densify_and_prune`` do with PyTorch bookkeeping, through ``csrc/liblrt_densify.so``.

    densify_stats(accum, denom, mean_grads, weights)            # in place: accum += |mean_grad|, denom += (weight > 0); one launch
    res = densify(groups, moments, accum, denom, rule, split_noise, box_noise)      # a DensifyResult: the new tensors, moments and counts
    twin = densify_reference(groups, moments, accum, denom, rule, split_noise, box_noise)   # the float64 twin, any device

``groups``: the six tensors of an asset by name (``xyz (P, 3)``, ``f_dc (P, 1, 3)``, ``f_rest (P, K, 3)`` with K >= 0, ``opacity (P, 1)``,
``scaling (P, S)`` with S in {2, 3}, ``rotation (P, 4)``).  ``moments``: ``{name: (exp_avg, exp_avg_sq)}`` for every group, or None for an asset
that has not stepped yet.  ``rule``: a ``DensifyRule`` (``rule_of`` builds it from the training options).  The noise is explicit:
``split_noise (P, 2, 3)`` standard normal draws, ``box_noise (P, 2, 2, 3)`` for an asset with a tracking box.  ``include/lrt_densify.h`` states
the rule and the order of the result.

* ``densify_reference`` / ``densify_stats_reference``: the float64 twins.  They are the yardstick.  Step 1 of the rule (``accum / denom`` and
  its comparison with the gradient threshold) is float32 on purpose: it IS a float32 decision, rows sit exactly on it.
* ``densify`` / ``densify_stats``: HIP float32 contiguous tensors go through the library -- an event is two launches of the plan, ONE read of
  the totals (the only host wait: the outputs have to be allocated) and one launch that moves all groups and moments.  A missing library is an
  error, and so is any other tensor on a HIP device: there is no quiet fall-back to PyTorch there.  CPU tensors run the same rule in torch
  ops, so the switch means the same thing without a GPU.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from types import SimpleNamespace
from typing import Dict, Optional, Tuple

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LRT_DENSIFY_LIB") or os.path.join(HERE, "csrc", "liblrt_densify.so")
EXPORTS = ("lrt_densify_abi_version", "lrt_densify_last_error", "lrt_densify_stats", "lrt_densify_workspace_bytes", "lrt_densify_plan",
           "lrt_densify_apply")                                              # include/lrt_densify.h
ABI_VERSION = 1
MAX_GROUPS = 8                                                               # LRT_DENSIFY_MAX_GROUPS
BLOCK_ROWS = 256                                                             # LRT_DENSIFY_BLOCK_ROWS
SCAN_BLOCKS = 1024                                                           # LRT_DENSIFY_SCAN_BLOCKS: blocks per pass of the scan
N_TOTALS = 8
GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
ROLE = {"xyz": 1, "scaling": 2}
LOG_1_6 = math.log(1.6)
SLOT_NAMES = ("original", "clone", "child 0", "child 1")

_lib = None


class DensifyError(RuntimeError):
    pass


class _Group(C.Structure):                                                   # lrt_densify_group
    _fields_ = [("src", C.c_void_p), ("src_exp_avg", C.c_void_p), ("src_exp_avg_sq", C.c_void_p), ("dst", C.c_void_p), ("dst_exp_avg", C.c_void_p),
                ("dst_exp_avg_sq", C.c_void_p), ("width", C.c_int), ("role", C.c_int)]


class _Rule(C.Structure):                                                    # lrt_densify_rule
    _fields_ = [("grad_thr", C.c_float), ("big_thr", C.c_float), ("huge_thr", C.c_float), ("opa_thr", C.c_float), ("size_limit", C.c_int),
                ("has_box", C.c_int), ("box_min", C.c_float * 3), ("box_max", C.c_float * 3)]


def load():
    """Load liblrt_densify.so (after torch, so that both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DensifyError(f"{LIB_PATH} is missing: build it with `python -m lidar_rt_amd.build` (hipcc --offload-arch=gfx950). "
                           "fused_densify has no fall-back on a HIP device.")
    lib = C.CDLL(LIB_PATH)
    lib.lrt_densify_abi_version.restype = C.c_int
    lib.lrt_densify_last_error.restype = C.c_char_p
    lib.lrt_densify_stats.restype = C.c_int
    lib.lrt_densify_stats.argtypes = [C.c_int, C.c_longlong] + [C.c_void_p] * 5
    lib.lrt_densify_workspace_bytes.restype = C.c_longlong
    lib.lrt_densify_workspace_bytes.argtypes = [C.c_longlong]
    lib.lrt_densify_plan.restype = C.c_int
    lib.lrt_densify_plan.argtypes = [C.c_int, C.c_longlong, C.c_int] + [C.c_void_p] * 8 + [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
    lib.lrt_densify_apply.restype = C.c_int
    lib.lrt_densify_apply.argtypes = [C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
    if lib.lrt_densify_abi_version() != ABI_VERSION:
        raise DensifyError("liblrt_densify.so ABI version mismatch; rebuild with `python -m lidar_rt_amd.build --force`")
    _lib = lib
    return lib


# ---- the rule's scalars ----------------------------------------------------------------------------------------------------------------------------

def _f32(x: float) -> float:
    """The float32 nearest to x, as a Python float."""
    return float(torch.tensor(x, dtype=torch.float64).to(torch.float32))


class DensifyRule(SimpleNamespace):
    """grad_thr, big_thr, huge_thr, opa_thr: float32 values (held as Python floats); size_limit: bool; box_min / box_max: three floats each, or None."""

    @property
    def has_box(self) -> bool:
        return self.box_min is not None


def make_rule(grad_thr, big_thr, huge_thr, opa_thr, size_limit, box_min=None, box_max=None) -> DensifyRule:
    if (box_min is None) != (box_max is None):
        raise DensifyError("densify: box_min and box_max come together")
    box = lambda b: None if b is None else tuple(_f32(float(v)) for v in torch.as_tensor(b).reshape(-1).tolist())
    r = DensifyRule(grad_thr=_f32(grad_thr), big_thr=_f32(big_thr), huge_thr=_f32(huge_thr), opa_thr=_f32(opa_thr), size_limit=bool(size_limit),
                    box_min=box(box_min), box_max=box(box_max))
    if r.box_min is not None and (len(r.box_min) != 3 or len(r.box_max) != 3):
        raise DensifyError("densify: box_min and box_max have three components")
    return r


def rule_of(opt, extent: float, scale_threshold: float, size_limit, bounding_box=None) -> DensifyRule:
    """The scalars of an event from the training options, formed as ``densify_and_prune`` forms them (Python floats, then float32)."""
    bb = bounding_box
    return make_rule(opt.densify_grad_threshold, scale_threshold * extent, 0.1 * extent * opt.prune_size_threshold, opt.thresh_opa_prune, bool(size_limit),
                     None if bb is None else bb.min_xyz, None if bb is None else bb.max_xyz)


# ---- the rule in torch ops: the twin and the CPU path --------------------------------------------------------------------------------------------------

class DensifyResult(SimpleNamespace):
    """groups {name: tensor of P_new rows}, moments {name: (exp_avg, exp_avg_sq)} or None, P_new, n_clone, n_split, n_scale, n_opa, n_outside,
    prune_applied.  The twin and the CPU path add src (the source row of every output row), slot (0 original, 1 clone, 2 child 0, 3 child 1) and
    offset (|R (exp(scaling) * noise)| per output row and component, 0 for copies: the scale of the children's accuracy gate), and per SOURCE row
    kind (0 keep, 1 clone, 2 split), mark (P, 2: the outputs marked for pruning), child_xyz (P, 2, 3) and child_scaling (P, S)."""

    @property
    def info(self) -> Tuple[int, int, int, int]:
        return self.n_clone, self.n_split, self.n_scale, self.n_opa


def _rotation(q: torch.Tensor) -> torch.Tensor:
    """(P, 4) quaternions (w, x, y, z), normalised here -> (P, 3, 3), in q's type."""
    q = q / q.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).view(-1, 3, 3)


def _offsets(R: torch.Tensor, sd: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
    """R (P, 3, 3), sd (P, ..., S) = exp(scaling), noise (P, ..., 3) -> R (sd * noise[..., :S]) with the third component 0 for S == 2: (P, ..., 3)."""
    S = sd.shape[-1]
    v = sd * noise[..., :S].to(sd.dtype)
    if S == 2:
        v = torch.cat([v, torch.zeros_like(v[..., :1])], -1)
    shape = v.shape
    return torch.bmm(v.reshape(shape[0], v[0].numel() // 3 if shape[0] else 1, 3), R.transpose(1, 2)).reshape(shape)


def _check_inputs(groups, moments, accum, denom, rule, split_noise, box_noise):
    if set(groups) != set(GROUPS):
        raise DensifyError(f"densify: the groups are {GROUPS} (got {tuple(groups)})")
    P = groups["xyz"].shape[0]
    S = groups["scaling"].shape[1] if groups["scaling"].dim() == 2 else -1
    if S not in (2, 3):
        raise DensifyError(f"densify: scaling must be (P, 2) or (P, 3) (it is {tuple(groups['scaling'].shape)})")
    want = {"xyz": (P, 3), "opacity": (P, 1), "scaling": (P, S), "rotation": (P, 4)}
    for n in GROUPS:
        t = groups[n]
        if t.shape[0] != P or (n in want and tuple(t.shape) != want[n]):
            raise DensifyError(f"densify: group {n} has shape {tuple(t.shape)} for an asset of {P} rows" + (f" (expected {want[n]})" if n in want else ""))
        if moments is not None:
            if n not in moments or len(moments[n]) != 2 or any(m.shape != t.shape for m in moments[n]):
                raise DensifyError(f"densify: group {n} needs two moments of shape {tuple(t.shape)}")
    for name, t in (("accum", accum), ("denom", denom)):
        if t.numel() != P:
            raise DensifyError(f"densify: {name} has {t.numel()} elements for an asset of {P} rows")
    if tuple(split_noise.shape) != (P, 2, 3):
        raise DensifyError(f"densify: split_noise must be ({P}, 2, 3) (it is {tuple(split_noise.shape)})")
    if rule.size_limit and rule.has_box:
        if box_noise is None or tuple(box_noise.shape) != (P, 2, 2, 3):
            raise DensifyError(f"densify: an asset with a box needs box_noise of shape ({P}, 2, 2, 3)")
    return P, S


def _rule_torch(groups, moments, accum, denom, rule, split_noise, box_noise, twin: bool) -> DensifyResult:
    """The rule in torch ops.  twin: every decision but step 1 and all geometry in float64, float64 children.  Otherwise the operator's arithmetic:
    float32 decisions, the children's geometry in float64 rounded to float32 once."""
    P, S = _check_inputs(groups, moments, accum, denom, rule, split_noise, box_noise)
    dev = groups["xyz"].device
    dec = torch.float64 if twin else torch.float32
    thr = lambda x: torch.tensor(x, dtype=torch.float32, device=dev).to(dec)
    xyz, scaling, rotation, opacity = (groups[n].detach() for n in ("xyz", "scaling", "rotation", "opacity"))
    # 1. float32 on purpose
    g = (accum.detach().reshape(-1).float() / denom.detach().reshape(-1).float()).nan_to_num(0.0)
    hot = g >= torch.tensor(rule.grad_thr, dtype=torch.float32, device=dev)
    big = torch.exp(scaling.to(dec)).max(dim=1).values > thr(rule.big_thr) if P else torch.zeros(0, dtype=torch.bool, device=dev)
    clone, split = hot & ~big, hot & big
    # 3. the children
    R = _rotation(rotation.double())
    sd = torch.exp(scaling.double())
    child_off = _offsets(R, sd[:, None, :], split_noise.double())                                  # (P, 2, 3)
    child_xyz = xyz.double()[:, None, :] + child_off
    child_scaling = torch.log(sd / 1.6) if twin else scaling.double() - LOG_1_6
    if not twin:
        child_xyz, child_scaling = child_xyz.float().double(), child_scaling.float().double()
    # 4. marks per output (slot 0, slot 1)
    has1 = clone | split
    low = (torch.sigmoid(opacity.to(dec)).reshape(-1) < thr(rule.opa_thr))
    out_scaling = torch.where(split[:, None], child_scaling, scaling.double())                      # both outputs of a row have one scaling
    zeros = torch.zeros(P, dtype=torch.bool, device=dev)
    huge, outside = zeros, torch.stack([zeros, zeros], 1)
    if rule.size_limit:
        huge = torch.exp(out_scaling.to(dec)).max(dim=1).values > thr(rule.huge_thr) if P else zeros
        if rule.has_box and P:
            out_xyz = torch.where(split[:, None, None], child_xyz, xyz.double()[:, None, :].expand(-1, 2, -1))      # (P, slot, 3)
            smp = out_xyz[:, :, None, :] + _offsets(R, torch.exp(out_scaling)[:, None, None, :], box_noise.double())   # (P, slot, sample, 3)
            lo = torch.tensor(rule.box_min, dtype=torch.float64, device=dev); hi = torch.tensor(rule.box_max, dtype=torch.float64, device=dev)
            outside = ~((smp >= lo) & (smp <= hi)).reshape(P, 2, 6).all(-1)
    exists = torch.stack([torch.ones(P, dtype=torch.bool, device=dev), has1], 1)
    outside = outside & exists
    low2, huge2 = low[:, None] & exists, huge[:, None] & exists
    mark = low2 | huge2 | outside
    n_out, n_mark = int(exists.sum()), int(mark.sum())
    applied = n_mark < n_out
    survive = exists & ~mark if applied else exists
    seg = [survive[:, 0] & ~split, survive[:, 1] & clone, survive[:, 0] & split, survive[:, 1] & split]
    idx = [torch.nonzero(s).reshape(-1) for s in seg]
    src = torch.cat(idx)
    slot = torch.cat([torch.full_like(ix, k) for k, ix in enumerate(idx)])
    P_new = int(src.numel())
    is_child = slot >= 2
    ch = (slot - 2).clamp_min(0)
    out, out_m = {}, (None if moments is None else {})
    for n in GROUPS:
        t = groups[n].detach()
        o = t[src]
        if n == "xyz":
            o = torch.where(is_child[:, None], child_xyz[src, ch], o.double())
        elif n == "scaling":
            o = torch.where(is_child[:, None], child_scaling[src], o.double())
        if n in ("xyz", "scaling") and not twin:
            o = o.to(t.dtype)
        out[n] = o
        if moments is not None:
            keep = (slot == 0).reshape((-1,) + (1,) * (t.dim() - 1))
            out_m[n] = tuple(torch.where(keep, m.detach()[src], torch.zeros((), dtype=m.dtype, device=dev)) for m in moments[n])
    offset = torch.where(is_child[:, None], child_off[src, ch].abs(), torch.zeros((), dtype=torch.float64, device=dev))
    return DensifyResult(groups=out, moments=out_m, P_new=P_new, n_clone=int(clone.sum()), n_split=int(split.sum()), n_scale=int(huge2.sum()),
                         n_opa=int(low2.sum()), n_outside=int(outside.sum()), prune_applied=int(applied), src=src, slot=slot, offset=offset,
                         kind=clone.to(torch.int64) + 2 * split.to(torch.int64), mark=mark, child_xyz=child_xyz, child_scaling=child_scaling)


@torch.no_grad()
def densify_reference(groups, moments, accum, denom, rule, split_noise, box_noise=None) -> DensifyResult:
    """The float64 twin of an event.  Copied tensors keep their type and bits; the children's xyz and scaling make those two tensors float64."""
    return _rule_torch(groups, moments, accum, denom, rule, split_noise, box_noise, twin=True)


@torch.no_grad()
def densify_stats_reference(accum, denom, mean_grads, weights):
    """(accum + |mean_grad|, denom + (weight > 0)) in float64, shaped like accum and denom."""
    a = accum.detach().double() + mean_grads.detach().double().reshape(-1, 3).pow(2).sum(-1).sqrt().reshape(accum.shape)
    d = denom.detach().double() + (weights.detach().reshape(denom.shape) > 0).double()
    return a, d


# ---- the operator ---------------------------------------------------------------------------------------------------------------------------------------

def _hip_tensor(name, t, dev, shape=None):
    if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.is_contiguous() and t.device == dev and (shape is None or tuple(t.shape) == tuple(shape))):
        what = f"{t.dtype}, {'contiguous' if t.is_contiguous() else 'not contiguous'}, {tuple(t.shape)}, on {t.device}" if torch.is_tensor(t) else type(t).__name__
        raise DensifyError(f"lrt_densify: {name} must be a contiguous float32 tensor" + (f" of shape {tuple(shape)}" if shape is not None else "") + f" on {dev} "
                           f"(it is {what}); there is no fall-back to PyTorch on a HIP device")
    return t


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


@torch.no_grad()
def densify_stats(accum, denom, mean_grads, weights):
    """In place: accum += |mean_grads row|, denom += (weights > 0).  accum, denom: P elements each; mean_grads (P, 3); weights: P elements
    (float32 hit weights, or a bool / uint8 filter on the CPU path)."""
    P = accum.numel()
    if denom.numel() != P or mean_grads.numel() != 3 * P or weights.numel() != P:
        raise DensifyError(f"densify_stats: accum {tuple(accum.shape)}, denom {tuple(denom.shape)}, mean_grads {tuple(mean_grads.shape)}, weights {tuple(weights.shape)} "
                           "do not describe one asset")
    dev = accum.device
    if dev.type == "cuda":
        lib = load()
        if weights.dtype != torch.float32:
            weights = weights.to(torch.float32)
        for name, t in (("accum", accum), ("denom", denom), ("mean_grads", mean_grads), ("weights", weights)):
            _hip_tensor(name, t, dev)
        if P == 0:
            return
        with torch.cuda.device(dev):
            rc = lib.lrt_densify_stats(dev.index, P, mean_grads.data_ptr(), weights.data_ptr(), accum.data_ptr(), denom.data_ptr(), _stream(dev))
        if rc != 0:
            raise DensifyError(f"lrt_densify_stats failed ({rc}): {lib.lrt_densify_last_error().decode()}")
        return
    if any(t.device != dev for t in (denom, mean_grads, weights)):
        raise DensifyError("densify_stats: the tensors of one asset live on one device")
    a, d = densify_stats_reference(accum, denom, mean_grads, weights)         # float64, rounded once: the kernel's arithmetic
    accum.copy_(a.to(accum.dtype)); denom.copy_(d.to(denom.dtype))


def _rule_struct(rule: DensifyRule) -> _Rule:
    r = _Rule(rule.grad_thr, rule.big_thr, rule.huge_thr, rule.opa_thr, int(rule.size_limit), int(rule.has_box))
    for k in range(3):
        r.box_min[k] = rule.box_min[k] if rule.has_box else 0.0
        r.box_max[k] = rule.box_max[k] if rule.has_box else 0.0
    return r


class Plan(SimpleNamespace):
    """What ``plan`` hands to ``apply``: the inputs, the workspace and the totals on the device."""


def plan(groups, moments, accum, denom, rule, split_noise, box_noise=None) -> Plan:
    """The two launches of lrt_densify_plan on HIP tensors.  No host wait: the totals stay on the device (``Plan.totals``, 8 x int64)."""
    P, S = _check_inputs(groups, moments, accum, denom, rule, split_noise, box_noise)
    dev = groups["xyz"].device
    lib = load()
    for n in GROUPS:
        _hip_tensor(f"group {n}", groups[n], dev)
        if moments is not None:
            _hip_tensor(f"exp_avg of group {n}", moments[n][0], dev); _hip_tensor(f"exp_avg_sq of group {n}", moments[n][1], dev)
    _hip_tensor("accum", accum, dev); _hip_tensor("denom", denom, dev); _hip_tensor("split_noise", split_noise, dev)
    box = rule.size_limit and rule.has_box
    if box:
        _hip_tensor("box_noise", box_noise, dev)
    nbytes = int(lib.lrt_densify_workspace_bytes(P))
    if nbytes < 0:
        raise DensifyError(f"lrt_densify_plan: {P} rows")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)                   # the caching allocator's blocks are 512-byte aligned
    totals = torch.empty(N_TOTALS, dtype=torch.int64, device=dev)
    crule = _rule_struct(rule)
    with torch.cuda.device(dev):
        rc = lib.lrt_densify_plan(dev.index, P, S, groups["xyz"].data_ptr(), groups["scaling"].data_ptr(), groups["rotation"].data_ptr(), groups["opacity"].data_ptr(),
                                  accum.data_ptr(), denom.data_ptr(), split_noise.data_ptr(), box_noise.data_ptr() if box else None, C.byref(crule),
                                  ws.data_ptr(), nbytes, totals.data_ptr(), _stream(dev))
    if rc != 0:
        raise DensifyError(f"lrt_densify_plan failed ({rc}): {lib.lrt_densify_last_error().decode()}")
    return Plan(P=P, S=S, dev=dev, groups=groups, moments=moments, split_noise=split_noise, workspace=ws, nbytes=nbytes, totals=totals)


def apply(pl: Plan, totals) -> DensifyResult:
    """The one launch of lrt_densify_apply.  ``totals``: ``pl.totals`` as the caller read it on the host (a list of 8 ints).  Allocates the outputs
    (torch.empty: no launch) and fills them."""
    P_new, n_clone, n_split, n_scale, n_opa, n_outside, applied = (int(v) for v in totals[:7])
    lib, dev = load(), pl.dev
    out, out_m = {}, (None if pl.moments is None else {})
    arr = (_Group * len(GROUPS))()
    for k, n in enumerate(GROUPS):
        t = pl.groups[n]
        out[n] = torch.empty((P_new,) + tuple(t.shape[1:]), dtype=torch.float32, device=dev)
        m = v = dm = dv = None
        if pl.moments is not None:
            m, v = pl.moments[n]
            dm, dv = torch.empty_like(out[n]), torch.empty_like(out[n])
            out_m[n] = (dm, dv)
        width = int(math.prod(t.shape[1:]))
        if width == 0:                                                       # f_rest of SH degree 0: nothing to move
            continue
        ptr = lambda x: None if x is None or x.numel() == 0 else x.data_ptr()
        arr[k] = _Group(ptr(t), ptr(m), ptr(v), ptr(out[n]), ptr(dm), ptr(dv), width, ROLE.get(n, 0))
    table = [arr[k] for k in range(len(GROUPS)) if arr[k].width > 0]
    carr = (_Group * len(table))(*table)
    if pl.P > 0:
        with torch.cuda.device(dev):
            rc = lib.lrt_densify_apply(dev.index, pl.P, P_new, pl.S, pl.groups["rotation"].data_ptr(), pl.split_noise.data_ptr(), len(table), C.cast(carr, C.c_void_p),
                                       pl.workspace.data_ptr(), pl.nbytes, _stream(dev))
        if rc != 0:
            raise DensifyError(f"lrt_densify_apply failed ({rc}): {lib.lrt_densify_last_error().decode()}")
    return DensifyResult(groups=out, moments=out_m, P_new=P_new, n_clone=n_clone, n_split=n_split, n_scale=n_scale, n_opa=n_opa, n_outside=n_outside,
                         prune_applied=applied)


@torch.no_grad()
def densify(groups: Dict[str, torch.Tensor], moments: Optional[Dict[str, Tuple[torch.Tensor, torch.Tensor]]], accum, denom, rule: DensifyRule, split_noise,
            box_noise=None) -> DensifyResult:
    """One event on one asset (see the module text).  The inputs are not changed."""
    groups = {n: groups[n].detach() for n in GROUPS} if set(groups) == set(GROUPS) else groups
    dev = groups["xyz"].device
    if dev.type == "cuda":
        pl = plan(groups, moments, accum, denom, rule, split_noise, box_noise)
        return apply(pl, pl.totals.tolist())                                  # the one host wait of the event
    if any(t.device != dev for t in groups.values()):
        raise DensifyError("densify: the tensors of one asset live on one device")
    return _rule_torch(groups, moments, accum, denom, rule, split_noise, box_noise, twin=False)
