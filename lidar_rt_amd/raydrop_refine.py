"""Ray-drop refinement: the U-Net that the reference trains after its Gaussians (train.py:386-447) and puts in front of every metric
(eval.py:129-144), its training stage, and its inference through ``csrc/liblrt_refine.so``.

    net = RaydropUNet(in_channels=9, channels=32)         # the reference's architecture and state_dict names: its unet.pth loads with strict=True
    packed = pack(net.cuda())                              # folded batch norms and K-major weights, on the device, once
    prob = refine_raydrop(render, rays, packed, backend="hip")   # (H, W, 1) float32; "hip": the operator, "torch": the module (the default, see below)
    net = train_refiner(render_fn, sensor, frames)         # the stage of train.py:386-447 through torch autograd

The network: a 1x1 convolution into ``channels`` planes; four stages of (2x2 max pooling, two 3x3 convolutions) to 2, 4, 8 and 8 times the
width; an attention block at the bottom; four stages of (bilinear x2 upsampling with aligned corners, padding to the skip's size,
concatenation ``[skip, upsampled]``, two 3x3 convolutions); batch norm, ReLU, a 1x1 convolution and a sigmoid.  Every 3x3 convolution has no
bias and is preceded by batch norm, ReLU and (in training) channel dropout.  The attention block normalises without a ReLU, projects to q, k, v
with one 1x1 convolution, attends with 8 heads over channel chunks, and then READS THE PRODUCT ``(heads, T, d)`` AS ``(H, W, C)`` without moving
the head axis behind the tokens -- trained weights depend on that, so it is reproduced here, in the module and in the kernels.

Inference here ALWAYS uses the stored running statistics and no dropout.  The reference's eval.py never takes its network out of training
mode: it normalises each frame with that frame's own statistics and draws dropout noise while evaluating, so its figures are not repeatable
even by itself.  ``RaydropUNet(...).double().eval()`` on the CPU is the float64 twin of the operator.
"""
from __future__ import annotations

import ctypes as C
import os
import random
from typing import Callable, Dict, List, Optional, Sequence

import torch
from torch import nn
from torch.nn import functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LRT_REFINE_LIB") or os.path.join(HERE, "csrc", "liblrt_refine.so")
EXPORTS = ("lrt_refine_abi_version", "lrt_refine_last_error", "lrt_refine_param_count", "lrt_refine_work_bytes", "lrt_refine_forward")   # include/lrt_refine.h
ABI_VERSION = 1
HEADS = 8                                                                    # LRT_REFINE_HEADS
MAX_TOKENS = 2048                                                            # LRT_REFINE_MAX_TOKENS
MAX_PIXELS = 1 << 24                                                         # LRT_REFINE_MAX_PIXELS
DROPOUT = 0.1
# "hip" or "torch": what refine_raydrop runs for CUDA tensors when neither the caller nor the packed network says.  It is "torch" because the
# operator is the slower one at the shape that matters (64 x 2048, channels 32: 1.80 ms against 1.28 ms, profiles/raydrop_refine.md); the
# operator stays selectable with backend="hip", pack(net, backend="hip") and evaluate --unet-backend hip.
DEFAULT_CUDA_BACKEND = "torch"

_lib = None


class RefineError(RuntimeError):
    pass


# ---- the module -------------------------------------------------------------------------------------------------------------------------------------------

class _Group(nn.Module):
    """Named children and nothing else: it gives the parameters the reference's dotted names; RaydropUNet holds the arithmetic."""

    def __init__(self, **children):
        super().__init__()
        for name, child in children.items():
            self.add_module(name, child)


def _conv_pair(c_in: int, c_out: int, c_mid: Optional[int] = None) -> nn.Sequential:
    """(batch norm, ReLU, channel dropout, 3x3 convolution without bias) twice: entries 0, 3, 4 and 7 carry the parameters."""
    c_mid = c_mid or c_out
    layers: List[nn.Module] = []
    for a, b in ((c_in, c_mid), (c_mid, c_out)):
        layers += [nn.BatchNorm2d(a), nn.ReLU(), nn.Dropout2d(DROPOUT), nn.Conv2d(a, b, 3, padding=1, bias=False)]
    return nn.Sequential(*layers)


def _stage(c_in: int, c_out: int, c_mid: Optional[int] = None) -> _Group:
    return _Group(conv=_Group(double_conv=_conv_pair(c_in, c_out, c_mid)))


class RaydropUNet(nn.Module):
    DOWN = ("down1", "down2", "down3", "down4")
    UP = ("up1", "up2", "up3", "up4")

    def __init__(self, in_channels: int = 9, channels: int = 32, out_channels: int = 1):
        super().__init__()
        c = int(channels)
        self.in_channels, self.channels, self.out_channels = int(in_channels), c, int(out_channels)
        self.inc = _Group(conv=nn.Conv2d(in_channels, c, 1))
        for name, (a, b) in zip(self.DOWN, ((c, 2 * c), (2 * c, 4 * c), (4 * c, 8 * c), (8 * c, 8 * c))):
            self.add_module(name, _stage(a, b))
        self.attn = _Group(proj_qkv=nn.Conv2d(8 * c, 24 * c, 1, bias=False), proj=nn.Conv2d(8 * c, 8 * c, 1, bias=False), norm=nn.BatchNorm2d(8 * c))
        for name, (a, b) in zip(self.UP, ((16 * c, 4 * c), (8 * c, 2 * c), (4 * c, c), (2 * c, c))):
            self.add_module(name, _stage(a, b, a))
        self.outc = _Group(conv=nn.Sequential(nn.BatchNorm2d(c), nn.ReLU(), nn.Conv2d(c, out_channels, 1)))

    def _attend(self, x: torch.Tensor) -> torch.Tensor:
        a = self.attn
        B, Cc, H, W = x.shape
        d = Cc // HEADS
        qkv = a.proj_qkv(a.norm(x)).reshape(B, 3, HEADS, d, H * W)
        q, k, v = qkv[:, 0], qkv[:, 1], qkv[:, 2]                            # (B, heads, d, T): head h owns channels h d .. h d + d - 1
        w = (q.transpose(-1, -2) @ k) * (int(d) ** -0.5)                     # (B, heads, T queries, T keys)
        if self.training:
            w = w + torch.bernoulli(torch.full_like(w, DROPOUT)) * -1e12
        h = (torch.softmax(w, dim=-1) @ v.transpose(-1, -2)).contiguous()    # (B, heads, T, d)
        h = h.reshape(B, H, W, Cc).permute(0, 3, 1, 2)                       # the memory re-read as (H, W, C): heads and tokens are NOT swapped
        return x + a.proj(h)

    def logits(self, x: torch.Tensor) -> torch.Tensor:
        skips = [self.inc.conv(x)]
        for name in self.DOWN:
            skips.append(getattr(self, name).conv.double_conv(F.max_pool2d(skips[-1], 2)))
        y = self._attend(skips.pop())
        for name in self.UP:
            skip = skips.pop()
            y = F.interpolate(y, scale_factor=2, mode="bilinear", align_corners=True)
            dy, dx = skip.shape[2] - y.shape[2], skip.shape[3] - y.shape[3]
            y = F.pad(y, [dx // 2, dx - dx // 2, dy // 2, dy - dy // 2])
            y = getattr(self, name).conv.double_conv(torch.cat([skip, y], dim=1))
        return self.outc.conv(y)

    def forward(self, x: torch.Tensor, return_logits: bool = False):
        z = self.logits(x)
        return (torch.sigmoid(z), z) if return_logits else torch.sigmoid(z)


# ---- inputs and weights -------------------------------------------------------------------------------------------------------------------------------------

def _planes(render):
    if isinstance(render, dict):
        return render["raydrop"], render["intensity"], render["depth"]
    return tuple(render)


def refine_inputs(render, rays=None) -> torch.Tensor:
    """(1, 3 | 9, H, W): ray-drop probability, intensity, depth, then ray_o xyz and ray_d xyz when ``rays`` is given (eval.py:131-143)."""
    p, i, d = _planes(render)
    H, W = d.shape[0], d.shape[1]
    x = [p.reshape(1, H, W), i.reshape(1, H, W), d.reshape(1, H, W)]
    if rays is not None:
        x += [rays[0].reshape(H, W, 3).permute(2, 0, 1), rays[1].reshape(H, W, 3).permute(2, 0, 1)]
    return torch.cat(x, dim=0).unsqueeze(0)


def fold_bn(bn: nn.BatchNorm2d):
    """(a, b) float32 with bn(x) = a x + b for the stored statistics: a = gamma / sqrt(var + eps), b = beta - mean a, in float64, rounded once."""
    a = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    b = bn.bias.detach().double() - bn.running_mean.detach().double() * a
    return a.float(), b.float()


def _k_major3(conv: nn.Conv2d) -> torch.Tensor:
    """(9 Cin, Cout): row k = (3 ky + kx) Cin + ci."""
    w = conv.weight.detach()
    return w.permute(2, 3, 1, 0).reshape(9 * w.shape[1], w.shape[0])


def _k_major1(conv: nn.Conv2d) -> torch.Tensor:
    w = conv.weight.detach()
    return w.reshape(w.shape[0], w.shape[1]).t()


class PackedRefiner:
    """What the operator reads: ``params``, one float32 tensor on the device in the order of include/lrt_refine.h, and the module in eval()
    for the torch path."""

    def __init__(self, net: RaydropUNet, params: torch.Tensor, backend: Optional[str] = None):
        self.net, self.params, self.backend = net, params, backend
        self.in_channels, self.channels = net.in_channels, net.channels
        self.device = params.device


def param_count(in_channels: int, channels: int) -> int:
    c, n = channels, in_channels * channels + channels
    for a, m, b in ((c, 2 * c, 2 * c), (2 * c, 4 * c, 4 * c), (4 * c, 8 * c, 8 * c), (8 * c, 8 * c, 8 * c),
                    (16 * c, 16 * c, 4 * c), (8 * c, 8 * c, 2 * c), (4 * c, 4 * c, c), (2 * c, 2 * c, c)):
        n += 2 * a + 9 * a * m + 2 * m + 9 * m * b
    return n + 2 * 8 * c + 8 * c * 24 * c + 8 * c * 8 * c + 2 * c + c + 1


def pack(net: RaydropUNet, device=None, backend: Optional[str] = None) -> PackedRefiner:
    """Fold every batch norm, lay the convolution weights out K-major and put all of it on the device in one tensor; reused for every frame.
    ``backend``: what refine_raydrop runs with this network on CUDA tensors when its caller does not say ("hip" or "torch"; None: the module default)."""
    if backend not in (None, "hip", "torch"):
        raise ValueError(f"pack: backend {backend!r} (hip, torch or None)")
    if not isinstance(net, RaydropUNet):
        raise TypeError("pack: a RaydropUNet")
    if net.channels < 8 or net.channels % 8 != 0:
        raise ValueError(f"pack: channels must be a multiple of 8 (it is {net.channels}): the kernels read eight input channels at a time")
    if net.in_channels not in (3, 9) or net.out_channels != 1:
        raise ValueError(f"pack: {net.in_channels} input and {net.out_channels} output channels (3 or 9, and 1)")
    dev = torch.device(device) if device is not None else next(net.parameters()).device
    parts = [_k_major1(net.inc.conv), net.inc.conv.bias.detach()]
    pairs = [getattr(net, n).conv.double_conv for n in net.DOWN] + [getattr(net, n).conv.double_conv for n in net.UP]
    for i, seq in enumerate(pairs):
        if i == 4:                                                           # the attention block sits between down4 and up1
            parts += [*fold_bn(net.attn.norm), _k_major1(net.attn.proj_qkv), _k_major1(net.attn.proj)]
        parts += [*fold_bn(seq[0]), _k_major3(seq[3]), *fold_bn(seq[4]), _k_major3(seq[7])]
    parts += [*fold_bn(net.outc.conv[0]), net.outc.conv[2].weight.detach().reshape(-1), net.outc.conv[2].bias.detach().reshape(-1)]
    flat = torch.cat([p.reshape(-1).to(torch.float32).cpu() for p in parts]).contiguous()
    assert flat.numel() == param_count(net.in_channels, net.channels)
    twin = net if dev == next(net.parameters()).device and not net.training and next(net.parameters()).dtype == torch.float32 else None
    if twin is None:
        twin = RaydropUNet(net.in_channels, net.channels, net.out_channels)
        twin.load_state_dict(net.state_dict())
        twin = twin.to(device=dev, dtype=torch.float32).eval()
    return PackedRefiner(twin, flat.to(dev), backend)


# ---- the operator -------------------------------------------------------------------------------------------------------------------------------------------

def load():
    """Load liblrt_refine.so (after torch, so that both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RefineError(f"{LIB_PATH} is missing: build it with `python -m lidar_rt_amd.build` (hipcc --offload-arch=gfx950). "
                          "refine_raydrop(backend='hip') has no fall-back.")
    lib = C.CDLL(LIB_PATH)
    lib.lrt_refine_abi_version.restype = C.c_int
    lib.lrt_refine_last_error.restype = C.c_char_p
    lib.lrt_refine_param_count.restype = C.c_longlong
    lib.lrt_refine_param_count.argtypes = [C.c_int, C.c_int]
    lib.lrt_refine_work_bytes.restype = C.c_longlong
    lib.lrt_refine_work_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    lib.lrt_refine_forward.restype = C.c_int
    lib.lrt_refine_forward.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_longlong] + [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p] * 4 \
        + [C.c_void_p, C.c_longlong, C.c_void_p]
    if lib.lrt_refine_abi_version() != ABI_VERSION:
        raise RefineError("liblrt_refine.so ABI version mismatch; rebuild with `python -m lidar_rt_amd.build --force`")
    _lib = lib
    return lib


def work_bytes(H: int, W: int, in_channels: int = 9, channels: int = 32) -> int:
    """Bytes of the workspace of one call; RefineError for a shape the operator refuses (the message says which limit)."""
    lib = load()
    n = int(lib.lrt_refine_work_bytes(int(H), int(W), int(in_channels), int(channels)))
    if n < 0:
        raise RefineError(f"refine_raydrop: refused ({n}): {lib.lrt_refine_last_error().decode()}")
    return n


def _workspace(workspace, nbytes, dev):
    if workspace is None:
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if not (torch.is_tensor(workspace) and workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.device == dev
            and workspace.numel() >= nbytes and workspace.data_ptr() % 256 == 0):
        raise RefineError(f"lrt_refine: the workspace must be a contiguous uint8 tensor of at least {nbytes} bytes on {dev}, 256-byte aligned")
    return workspace


def _plane(name, t, shape, dev):
    if not (torch.is_tensor(t) and t.device == dev and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == shape[0] * shape[1] * shape[2]):
        raise RefineError(f"lrt_refine: {name} must be a contiguous float32 tensor of {shape} on {dev}; there is no fall-back to PyTorch on a HIP device")
    return t


def _strided_plane(name, t, H, W, dev):
    """(tensor, pixel stride): a float32 plane of H x W pixels at a constant stride, read where it lies -- the renderer's planes are slices of
    one (H, W, channels) tensor.  Any other layout is copied once."""
    if not (torch.is_tensor(t) and t.device == dev and t.dtype == torch.float32 and t.numel() == H * W):
        raise RefineError(f"lrt_refine: {name} must be a float32 tensor of {H} x {W} pixels on {dev}; there is no fall-back to PyTorch on a HIP device")
    if tuple(t.shape) not in ((H, W), (H, W, 1)):
        raise RefineError(f"lrt_refine: {name} must be ({H}, {W}, 1) or ({H}, {W}) (it is {tuple(t.shape)})")
    t = t.detach()[..., 0] if t.dim() == 3 else t.detach()
    s = t.stride(1) if W > 1 else 1
    if s >= 1 and t.stride(0) == W * s and s * H * W < 2 ** 31:
        return t, s
    return t.contiguous(), 1


def _refine_hip(planes, rays, packed: PackedRefiner, return_logits, out, workspace):
    lib = load()
    p, i, d = planes
    dev = d.device
    H, W = int(d.shape[0]), int(d.shape[1])
    if packed.device != dev:
        raise RefineError(f"lrt_refine: the packed weights are on {packed.device}, the render on {dev}")
    if (rays is not None) != (packed.in_channels == 9):
        raise RefineError(f"lrt_refine: a network of {packed.in_channels} input channels {'needs' if rays is None else 'takes no'} rays")
    (p, sp), (i, si), (d, sd) = _strided_plane("raydrop", p, H, W, dev), _strided_plane("intensity", i, H, W, dev), _strided_plane("depth", d, H, W, dev)
    ro = rd = None
    if rays is not None:
        ro, rd = _plane("ray_o", rays[0].detach().contiguous(), (H, W, 3), dev), _plane("ray_d", rays[1].detach().contiguous(), (H, W, 3), dev)
    ws = _workspace(workspace, work_bytes(H, W, packed.in_channels, packed.channels), dev)
    if out is None:
        out = torch.empty((H, W, 1), dtype=torch.float32, device=dev)
    else:
        _plane("out", out, (H, W, 1), dev)
    logits = torch.empty((H, W, 1), dtype=torch.float32, device=dev) if return_logits else None
    with torch.cuda.device(dev):
        rc = lib.lrt_refine_forward(dev.index, H, W, packed.in_channels, packed.channels, packed.params.data_ptr(), packed.params.numel(),
                                    p.data_ptr(), i.data_ptr(), d.data_ptr(), sp, si, sd, None if ro is None else ro.data_ptr(), None if rd is None else rd.data_ptr(),
                                    out.data_ptr(), None if logits is None else logits.data_ptr(), ws.data_ptr(), ws.numel(),
                                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise RefineError(f"lrt_refine_forward failed ({rc}): {lib.lrt_refine_last_error().decode()}")
    return (out, logits) if return_logits else out


def refine_raydrop(render, rays, packed, *, return_logits: bool = False, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                   backend: Optional[str] = None):
    """The refined ray-drop probability (H, W, 1) float32 of one frame (and the logits with ``return_logits``).  ``render``: the renderer's
    dictionary (or the triple raydrop, intensity, depth), each (H, W, 1); ``rays``: (ray_o, ray_d), each (H, W, 3), or None for a 3-input network.
    ``packed``: what ``pack`` returned (a bare RaydropUNet serves the torch path only).  backend "hip": the operator, which reads the tensors as
    they are (no cat / permute copy); "torch": the module in eval() on refine_inputs.  None: for CUDA tensors what the packed network names, else
    DEFAULT_CUDA_BACKEND; the module for CPU tensors.  Stored running statistics, no dropout, whatever mode the module is in."""
    planes = _planes(render)
    dev = planes[2].device
    if backend is None:
        backend = (packed.backend or DEFAULT_CUDA_BACKEND) if dev.type == "cuda" and isinstance(packed, PackedRefiner) else "torch"
    if backend not in ("hip", "torch"):
        raise RefineError(f"refine_raydrop: backend {backend!r} (hip or torch)")
    if backend == "hip":
        if dev.type != "cuda" or not isinstance(packed, PackedRefiner):
            raise RefineError("refine_raydrop: backend 'hip' needs CUDA tensors and packed weights (pack(net))")
        return _refine_hip(planes, rays, packed, return_logits, out, workspace)
    if workspace is not None:
        raise RefineError("refine_raydrop: a workspace with the torch backend")
    net = packed.net if isinstance(packed, PackedRefiner) else packed
    H, W = planes[2].shape[0], planes[2].shape[1]
    was_training = net.training
    net.eval()
    try:
        with torch.no_grad():
            par = next(net.parameters())
            prob, z = net(refine_inputs(planes, rays).to(device=par.device, dtype=par.dtype), return_logits=True)
    finally:
        net.train(was_training)
    prob, z = prob.reshape(H, W, 1).to(device=dev, dtype=torch.float32), z.reshape(H, W, 1).to(device=dev, dtype=torch.float32)
    if out is not None:
        out.copy_(prob); prob = out
    return (prob, z) if return_logits else prob


# ---- the training stage ---------------------------------------------------------------------------------------------------------------------------------------

def refine_sample(render, rays, mask: torch.Tensor, rot: int = 0):
    """One frame's (input (1, C, H, W), labels (H W, 1) float): detached renders, labels 1 where the ray was dropped (~mask); both rolled to start
    at column ``rot`` (train.py:419-436)."""
    x = refine_inputs({k: render[k].detach() for k in ("raydrop", "intensity", "depth")}, rays)
    lab = ~mask.bool().reshape(x.shape[2], x.shape[3])
    if rot:
        x = torch.cat([x[..., rot:], x[..., :rot]], dim=-1)
        lab = torch.cat([lab[:, rot:], lab[:, :rot]], dim=-1)
    return x, lab.reshape(-1, 1).to(x.dtype)


def train_refiner(render_fn: Callable, sensor, frames: Sequence, *, in_spatial: bool = True, rot: bool = False, epochs: int = 400, batch: int = 16,
                  lr: float = 1e-3, lambda_bce: float = 0.01, seed: int = 0, net: Optional[RaydropUNet] = None, channels: int = 32, device=None,
                  log: Optional[list] = None) -> RaydropUNet:
    """The stage of train.py:386-447: the network in train() mode on detached renders, BCE against ~mask scaled by ``lambda_bce``, gradients
    accumulated over ``batch`` frames per Adam step, ``epochs`` steps; frames are popped from a shuffled stack that is refilled when empty.
    ``render_fn(frame)`` returns the render dictionary; ``sensor`` offers get_mask(frame) and (in_spatial) get_range_rays(frame).  The draws (initial
    weights, shuffles, dropout, rolls) are functions of ``seed``.  ``log``: a list that receives one {"epoch", "frames", "loss"} per step."""
    frames = list(frames)
    if not frames:
        raise RefineError("train_refiner: no frames")
    rng = random.Random(seed)
    devices = [torch.cuda.current_device()] if torch.cuda.is_available() else []
    with torch.random.fork_rng(devices=devices):
        torch.manual_seed(seed)
        if net is None:
            net = RaydropUNet(9 if in_spatial else 3, channels, 1)
        if device is not None:
            net = net.to(device)
        net.train()
        optimizer = torch.optim.Adam(net.parameters(), lr=lr)
        optimizer.zero_grad()
        par = next(net.parameters())
        stack: list = []
        for epoch in range(epochs):
            seen, total = [], 0.0
            for _ in range(batch):
                if not stack:
                    stack = list(frames)
                    rng.shuffle(stack)
                frame = stack.pop()
                render = render_fn(frame)
                rays = sensor.get_range_rays(frame) if in_spatial else None
                W = render["depth"].shape[1]
                x, labels = refine_sample(render, rays, sensor.get_mask(frame), rng.randrange(W) if rot else 0)
                prob = net(x.to(device=par.device, dtype=par.dtype)).reshape(-1, 1)
                loss = lambda_bce * F.binary_cross_entropy(prob, labels.to(device=par.device, dtype=par.dtype))
                loss.backward()
                seen.append(frame); total = total + loss.detach()
            optimizer.step()
            optimizer.zero_grad()
            if log is not None:
                log.append({"epoch": epoch, "frames": seen, "loss": float(total) / batch})       # one host wait per Adam step, none per frame
    return net
