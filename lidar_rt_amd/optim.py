"""The optimizer step of one Gaussian asset in one operator (``training_setup`` with ``opt.fused_adam``), optionally on the rows a frame hit only
(``opt.sparse_adam``).

    opt = GaussianAdam([{"params": [xyz], "lr": ..., "name": "xyz"}, ...], lr=0.0, eps=1e-15)
    opt.step()                     # every row of every group whose parameter has a gradient
    opt.step(rows=touched)         # only the rows whose flag is set; the others keep parameter and both moments bit for bit
    p, m, v = adam_reference(param, grad, exp_avg, exp_avg_sq, step=t, lr=lr, rows=None)

The rule is ``torch.optim.Adam``'s without weight decay, amsgrad or maximize (``include/lrt_adam.h`` states it).  ``state`` has torch's keys --
``step`` (a float32 tensor on the parameter's device, as torch's fused Adam keeps it), ``exp_avg``, ``exp_avg_sq`` -- and the param groups carry
torch's defaults, so ``GaussianAsset._rewrite``, ``capture()`` / ``restore()`` work unchanged and a checkpoint written under either optimizer
loads under the other.

* ``adam_reference``: the float64 twin, any device.  Returns float64 tensors.  It is the yardstick.
* ``GaussianAdam.step``: HIP float32 contiguous tensors go through ``csrc/liblrt_adam.so`` -- ONE launch for all groups of the asset, no
  allocation, no host wait, no atomics.  A missing library is an error, and so is any other tensor on a HIP device: there is no quiet fall-back
  to PyTorch there.  CPU tensors (float32 or float64) run the same rule with the same mask semantics in torch ops: sparse mode means the same
  thing without a GPU.

What sparse mode changes in the optimisation: Adam's moments normally decay on every step, and a row whose gradient is zero still moves along
its first moment.  A row outside ``rows`` does neither -- its moments do not decay and its parameter does not coast; when a later frame hits it
again it continues from the moments it had.  The bias corrections are those of the group's step count, which advances on every call.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LRT_ADAM_LIB") or os.path.join(HERE, "csrc", "liblrt_adam.so")
EXPORTS = ("lrt_adam_abi_version", "lrt_adam_last_error", "lrt_adam_step")   # include/lrt_adam.h
ABI_VERSION = 1
MAX_GROUPS = 8                                                               # LRT_ADAM_MAX_GROUPS

_lib = None


class AdamError(RuntimeError):
    pass


class _Group(C.Structure):                                                   # lrt_adam_group
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("rows", C.c_longlong),
                ("width", C.c_int), ("lr", C.c_double), ("bias_correction1", C.c_double), ("bias_correction2_sqrt", C.c_double)]


def load():
    """Load liblrt_adam.so (after torch, so that both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AdamError(f"{LIB_PATH} is missing: build it with `python -m lidar_rt_amd.build` (hipcc --offload-arch=gfx950). "
                        "GaussianAdam has no fall-back on a HIP device.")
    lib = C.CDLL(LIB_PATH)
    lib.lrt_adam_abi_version.restype = C.c_int
    lib.lrt_adam_last_error.restype = C.c_char_p
    lib.lrt_adam_step.restype = C.c_int
    lib.lrt_adam_step.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_double, C.c_double, C.c_double, C.c_void_p]
    if lib.lrt_adam_abi_version() != ABI_VERSION:
        raise AdamError("liblrt_adam.so ABI version mismatch; rebuild with `python -m lidar_rt_amd.build --force`")
    _lib = lib
    return lib


def bias_corrections(step: float, beta1: float, beta2: float):
    """(1 - beta1^step, sqrt(1 - beta2^step)) in float64, as torch forms them."""
    return 1.0 - beta1 ** step, math.sqrt(1.0 - beta2 ** step)


def _row_flags(rows: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    return (rows != 0).reshape((-1,) + (1,) * (like.dim() - 1))


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------------------

@torch.no_grad()
def adam_reference(param, grad, exp_avg, exp_avg_sq, *, step: float, lr: float, betas=(0.9, 0.999), eps: float = 1e-15, rows=None):
    """One Adam step in float64: the (parameter, exp_avg, exp_avg_sq) after step number ``step`` (1 for the first), float64 tensors.
    ``rows``: a flag per row of the first dimension; a row whose flag is 0 keeps all three."""
    b1, b2 = betas
    dev = param.device if torch.is_tensor(param) else None
    p, g, m, v = (torch.as_tensor(t).detach().to(device=dev, dtype=torch.float64) for t in (param, grad, exp_avg, exp_avg_sq))   # tensors or numpy arrays
    bc1, bc2s = bias_corrections(float(step), b1, b2)
    m2 = m + (1.0 - b1) * (g - m)
    v2 = b2 * v + (1.0 - b2) * g * g
    p2 = p - (lr / bc1) * m2 / (v2.sqrt() / bc2s + eps)
    if rows is not None:
        if rows.numel() != p.shape[0]:
            raise AdamError(f"adam_reference: a row mask of {rows.numel()} rows for a tensor of {p.shape[0]}")
        on = _row_flags(rows.to(p.device), p)
        p2, m2, v2 = torch.where(on, p2, p), torch.where(on, m2, m), torch.where(on, v2, v)
    return p2, m2, v2


# ---- the optimizer ------------------------------------------------------------------------------------------------------------------------------

def _step_torch(p, g, m, v, on, lr, bc1, bc2s, b1, b2, eps):
    """lrt_adam_math.h in torch ops, in place: the moment lines in float64 rounded to the tensors' type once each, lr / bias_correction1 one
    float64 division rounded once, the parameter line in the tensors' type."""
    dt = p.dtype
    g64, m64, v64 = g.double(), m.double(), v.double()
    m2 = (m64 + (1.0 - b1) * (g64 - m64)).to(dt)
    v2 = (b2 * v64 + (1.0 - b2) * g64 * g64).to(dt)
    sc = lambda x: torch.tensor(x, dtype=dt, device=p.device)
    step_size = sc(lr / bc1)
    denom = ((v2.sqrt() / sc(bc2s)).double() + eps).to(dt)
    p2 = p - step_size * m2 / denom
    if on is None:
        p.copy_(p2); m.copy_(m2); v.copy_(v2)
    else:
        p.copy_(torch.where(on, p2, p)); m.copy_(torch.where(on, m2, m)); v.copy_(torch.where(on, v2, v))


class GaussianAdam(torch.optim.Optimizer):
    """Adam over the parameter groups of one asset (one parameter per group, all sharing the first dimension), see the module text."""

    def __init__(self, params, lr: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-15):
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0 and eps >= 0.0):
            raise ValueError(f"GaussianAdam: betas {betas} (0 <= beta < 1), eps {eps} (>= 0)")
        # torch.optim.Adam's own defaults, whatever keys this torch version has: a state_dict of this optimizer then loads under Adam
        defaults = dict(torch.optim.Adam([torch.zeros(1)], lr=lr, betas=betas, eps=eps).defaults)
        super().__init__(params, defaults)
        first = self.param_groups[0]["params"][0]
        for g in self.param_groups:
            g["fused"] = bool(first.is_cuda)                 # what training_setup passes to Adam: load_state_dict then keeps `step` on the device
        self._mirror = {}                                    # parameter -> (its `step` tensor, the same count on the host)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._mirror = {}
        for p, st in self.state.items():
            if not torch.is_tensor(st["step"]):
                st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32, device=p.device)
            self._mirror[p] = (st["step"], float(st["step"]))

    def _host_step(self, p, st) -> float:
        """The step count of a state entry on the host.  Read from the tensor (a host wait) only when the entry is new to this optimizer:
        after load_state_dict or when the training loop moved a state to a replaced parameter."""
        ent = self._mirror.get(p)
        if ent is None or ent[0] is not st["step"]:
            if len(self._mirror) > 4 * max(1, len(self.state)):
                self._mirror = {q: e for q, e in self._mirror.items() if q in self.state}     # parameters that were replaced
            ent = (st["step"], float(st["step"]))
            self._mirror[p] = ent
        return ent[1]

    @torch.no_grad()
    def step(self, rows: Optional[torch.Tensor] = None, closure=None):
        """One step of every group whose parameter has a gradient; a parameter without one is skipped and its ``step`` does not advance.
        ``rows`` (bool or uint8, one flag per row, on the parameters' device): only the flagged rows are updated."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = []
        for g in self.param_groups:
            for p in g["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    self._mirror[p] = (st["step"], 0.0)
                work.append((g, p, st))
        if not work:
            return loss
        dev = work[0][1].device
        if any(p.device != dev for _, p, _ in work):
            raise AdamError("GaussianAdam.step: the parameters of one optimizer live on one device")
        if rows is not None:
            if not (torch.is_tensor(rows) and rows.dtype in (torch.bool, torch.uint8) and rows.dim() == 1):
                raise AdamError("GaussianAdam.step: rows must be a one-dimensional bool or uint8 tensor")
            if rows.device != dev:
                raise AdamError(f"GaussianAdam.step: rows must be on {dev} (it is on {rows.device})")
        table = []
        for g, p, st in work:
            t = self._host_step(p, st) + 1.0
            b1, b2 = g["betas"]
            table.append((g, p, st, t) + bias_corrections(t, b1, b2))
        if dev.type == "cuda":
            self._step_hip(dev, table, rows)
        else:
            for g, p, st, t, bc1, bc2s in table:
                if rows is not None and rows.numel() != p.shape[0]:
                    raise AdamError(f"GaussianAdam.step: group {g.get('name', '?')} has {p.shape[0]} rows, the row mask {rows.numel()}")
            for g, p, st, t, bc1, bc2s in table:
                b1, b2 = g["betas"]
                _step_torch(p, p.grad, st["exp_avg"], st["exp_avg_sq"], None if rows is None else _row_flags(rows, p), g["lr"], bc1, bc2s, b1, b2, g["eps"])
        # the call was accepted: the counts advance, on the device (one launch) and in the mirror
        torch._foreach_add_([st["step"] for _, _, st, *_ in table], 1.0)
        for _, p, st, t, *_ in table:
            self._mirror[p] = (st["step"], t)
        return loss

    def _step_hip(self, dev, table, rows):
        lib = load()
        g0 = table[0][0]
        for g, p, st, *_ in table:
            if g["betas"] != g0["betas"] or g["eps"] != g0["eps"]:
                raise AdamError("GaussianAdam.step: one call has one beta1, beta2 and eps; the groups differ")
            for name, x in (("parameter", p), ("gradient", p.grad), ("exp_avg", st["exp_avg"]), ("exp_avg_sq", st["exp_avg_sq"])):
                if x.dtype != torch.float32 or not x.is_contiguous() or x.device != dev or x.shape != p.shape:
                    raise AdamError(f"lrt_adam_step: group {g.get('name', '?')}: the {name} must be a contiguous float32 tensor of shape {tuple(p.shape)} on {dev} "
                                    f"(it is {x.dtype}, {'contiguous' if x.is_contiguous() else 'not contiguous'}, {tuple(x.shape)}, on {x.device}); "
                                    "there is no fall-back to PyTorch on a HIP device")
            if p.dim() < 1:
                raise AdamError(f"lrt_adam_step: group {g.get('name', '?')}: a parameter without a first dimension")
        for g, p, *_ in table:                               # an empty asset: nothing to update, and no pointer to pass
            if p.numel() == 0 and rows is not None and rows.numel() != p.shape[0]:
                raise AdamError(f"lrt_adam_step: group {g.get('name', '?')} has {p.shape[0]} rows, the row mask {rows.numel()}")
        table = [e for e in table if e[1].numel() > 0]
        if not table:
            return
        arr = (_Group * len(table))()
        for k, (g, p, st, t, bc1, bc2s) in enumerate(table):
            n_rows = p.shape[0]
            arr[k] = _Group(p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), n_rows,
                            p.numel() // n_rows if n_rows else 1, float(g["lr"]), bc1, bc2s)
        mask = None
        if rows is not None:
            mask = rows.contiguous()
            mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
        b1, b2 = g0["betas"]
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            rc = lib.lrt_adam_step(dev.index, len(table), C.cast(arr, C.c_void_p), None if mask is None else mask.data_ptr(),
                                   0 if mask is None else mask.numel(), float(b1), float(b2), float(g0["eps"]), stream)
        if rc != 0:
            raise AdamError(f"lrt_adam_step failed ({rc}): {lib.lrt_adam_last_error().decode()}")
