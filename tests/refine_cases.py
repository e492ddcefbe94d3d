"""Shared cases of the ray-drop refinement tests: the golden fixture, seeded networks with randomised batch-norm statistics, frames as the
renderer produces them, the case tables and gates of the GPU tests, a twin of the operator's workspace plan, and the references (float64 twin and
float32 CPU module: logits and every layer), computed once per case and handed out unchanged."""
import functools
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refine_unet.npz")
LOGIT_04 = math.log(0.4 / 0.6)                                               # sigmoid(z) < 0.4  <=>  z < logit(0.4)
GOLDEN_SHAPES = ((9, 18, 38), (9, 33, 75), (3, 16, 32))

# The cases (inputs, channels, H, W) of the GPU tests.  CASES are the first ones: channels 8 and 32 over four frames, and the shape the project
# is built for.  64 x 2048 at channels 32 is the only one of them at which the launcher leaves the K-split kernel: up4.1 has 8192 tiles and
# takes two column tiles per wave (NT = 2), up3.1 and up4.2 have 4096 and run one chain over all of K in four-group steps (KS = 1)
FRAMES = ((16, 32), (18, 38), (33, 75), (64, 256))
FULL = (9, 32, 64, 2048)
CASES = [(9, 32, H, W) for H, W in FRAMES] + [(9, 8, H, W) for H, W in FRAMES] + [(3, 32, 18, 38), (3, 8, 33, 75), (3, 8, 64, 256), FULL]
# What CASES never run (tests/test_raydrop_refine.py restates the launcher and asserts that these reach it):
#   1  a four-group loop FOLLOWED by a one-group remainder in one fma chain (a per-wave channel range above 32 that is no multiple of 32)
#   2  a column tile from output channel 32 on that is only partly inside C_out, in the plain and in the K-split kernel
#   3  two column tiles per wave with a ragged last pixel tile and idle waves in the last workgroup
#   4  attention over more than 64 tokens that are no multiple of 64, and over one token
#   5  the smallest legal frame: a 1 x 1 bottom level, up-sampling from a single pixel, levels under 32 pixels in the plain kernel
#   6  the widths between 8 and 64 (at 64 up1's first convolution sums over K = 9 x 1024)
NEW_CASES = [(9, 16, 33, 75), (9, 24, 33, 75), (9, 40, 18, 38), (9, 48, 33, 75), (9, 56, 18, 38), (9, 64, 33, 75),      # every width; 1, 2, 6
             (3, 40, 64, 256),                                                                                      # 3 inputs at a ragged width
             (9, 8, 16, 16), (3, 24, 16, 16), (9, 64, 16, 16),                                                      # 5, and 4 with T = 1
             (9, 24, 80, 210), (9, 8, 17, 1100),                                                                    # 4 with T = 65 and 68
             (9, 32, 65, 2017),                                                                                     # 3, T = 504
             (9, 24, 65, 2017)]                                                                                     # 1, 2 and 3 at NT = 2: up4.1 with 48 channels in and out
# The gates.  Logits: e_op = max |logit_op - logit_f64| <= K e_f32, e_f32 the same figure of the float32 CPU module; one K for all cases, at most
# K_CAP.  Layers: e_op[b] <= K_L max(e_f32[b], 2^-24 max |b_f64|) for each of the 20 buffers b; profiles/raydrop_refine.md has the measured ratios.
# K was fixed at 4 over a first measured 1.66.  K_L by the same rule, the smallest of 2, 4, 8 that is at least twice the largest ratio of the first
# run with the layers: that was 3.56 (X1 at channels 56, 18 x 38; no buffer of any case above 4), so K_L = 8, which is also the cap.
K = 4.0
K_L = 8.0
K_CAP = 8.0
MASK_CAP = 0.005                                                             # at most 0.5 % of a case's pixels may sit that close to logit(0.4)
WIDTHS = (8, 16, 24, 32, 40, 48, 56, 64)                                    # what check_shape of lrt_refine.hip accepts

# The workspace's buffers in rf_plan's order, the level each lives on and its channels in units of the width
BUFFERS = ("X0", "M1", "X1", "M2", "X2", "M3", "X3", "M4", "X4", "QKV", "HB", "X4A", "U3M", "Y3", "U2M", "Y2", "U1M", "Y1", "U0M", "Y0")
BUFFER_LEVEL = (0, 1, 1, 2, 2, 3, 3, 4, 4, 4, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0)
BUFFER_CHANNELS = (1, 2, 2, 4, 4, 8, 8, 8, 8, 24, 8, 8, 16, 4, 8, 2, 4, 1, 2, 1)


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def golden_state(C):
    g = golden()
    # the 3-input network is the 9-input one behind its own input convolution: the fixture holds that one array (p3_0) and shares the rest
    return {str(n): torch.as_tensor(g[f"p{C}_{i}"] if f"p{C}_{i}" in g else g[f"p9_{i}"]) for i, n in enumerate(g[f"names{C}"])}


def randomise(net, seed):
    """Seeded weights as they are, and every batch norm's statistics and affine drawn anew: the default ones make a batch norm the identity."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                m.running_mean.copy_(torch.randn(n, generator=g) * 0.5)
                m.running_var.copy_(torch.rand(n, generator=g) * 1.5 + 0.5)
                m.weight.copy_(torch.rand(n, generator=g) + 0.5)
                m.bias.copy_(torch.randn(n, generator=g) * 0.3)
    return net


@functools.lru_cache(maxsize=None)
def network(in_channels, channels, seed=0):
    from lidar_rt_amd.raydrop_refine import RaydropUNet
    from lidar_rt_amd.raydrop_refine import refine_inputs
    torch.manual_seed(1000 + 10 * channels + in_channels + seed)
    net = randomise(RaydropUNet(in_channels, channels), 2000 + channels + in_channels + seed).eval()
    # a freshly drawn network's logits lie in a narrow band on one side of logit(0.4): move the output bias so that the band's middle (on one
    # small frame) sits on the threshold and the masks of the cases hold hits and drops alike
    render, rays = frame(18, 38)
    with torch.no_grad():
        z = net.logits(refine_inputs(render, rays if in_channels == 9 else None))
        net.outc.conv[2].bias += LOGIT_04 - float(z.median())
    return net


@functools.lru_cache(maxsize=None)
def frame(H, W, seed=0):
    """(render dictionary, (ray_o, ray_d)) float32 on the CPU: probabilities, intensities, depth 0..80 m, one origin, unit directions."""
    g = torch.Generator().manual_seed(77 * H + W + seed)
    render = {"raydrop": torch.rand((H, W, 1), generator=g), "intensity": torch.rand((H, W, 1), generator=g),
              "depth": torch.rand((H, W, 1), generator=g) * 80.0}
    o = (torch.randn(3, generator=g) * 10.0).expand(H, W, 3).contiguous()
    d = torch.randn((H, W, 3), generator=g)
    return render, (o, (d / d.norm(dim=-1, keepdim=True)).contiguous())


def plan(channels, H, W):
    """The Python twin of rf_plan (csrc/lrt_refine_math.h): ({buffer: (float offset, level, channels)}, total floats).  Every buffer is
    channels-last (pixels of its level, channels), starts at a multiple of 64 floats and holds a RAW convolution output."""
    off, o = {}, 0
    for name, level, mult in zip(BUFFERS, BUFFER_LEVEL, BUFFER_CHANNELS):
        off[name] = (o, level, mult * channels)
        o += ((H >> level) * (W >> level) * mult * channels + 63) // 64 * 64
    return off, o


def collect(net, x):
    """One forward of `net` (any dtype, eval()) on x (1, C, H, W): (logits (H, W), {buffer: (pixels, channels) tensor laid out as the operator's
    workspace}).  Forward hooks on the convolutions and a wrapper round whatever `net._attend` is at the time; nothing of the arithmetic changes."""
    got, hooks = {}, []
    last = lambda t: t.detach()[0].permute(1, 2, 0).reshape(-1, t.shape[1]).contiguous()          # (1, ch, h, w) -> (h w, ch)

    def keep(module, name):
        hooks.append(module.register_forward_hook(lambda m, inp, out: got.__setitem__(name, last(out))))
    keep(net.inc.conv, "X0")
    stages = list(zip(net.DOWN, ("M1", "M2", "M3", "M4"), ("X1", "X2", "X3", "X4"))) + list(zip(net.UP, ("U3M", "U2M", "U1M", "U0M"), ("Y3", "Y2", "Y1", "Y0")))
    for stage, mid, out in stages:
        seq = getattr(net, stage).conv.double_conv
        keep(seq[3], mid)
        keep(seq[7], out)
    keep(net.attn.proj_qkv, "QKV")
    # proj reads the value product's memory (heads, T, d) as (H, W, C): channels-last of its input IS that memory, in order
    hooks.append(net.attn.proj.register_forward_hook(lambda m, inp, out: got.__setitem__("HB", last(inp[0]))))
    own, attend = vars(net).get("_attend"), net._attend                       # own: an override that the caller put on this instance

    def wrapped(t):
        y = attend(t)
        got["X4A"] = last(y)
        return y
    net._attend = wrapped
    try:
        with torch.no_grad():
            z = net.logits(x).reshape(x.shape[2], x.shape[3])
    finally:
        if own is None:
            del net._attend
        else:
            net._attend = own
        for h in hooks:
            h.remove()
    assert sorted(got) == sorted(BUFFERS)
    return z, got


def case_input(in_channels, H, W):
    from lidar_rt_amd.raydrop_refine import refine_inputs
    render, rays = frame(H, W)
    return refine_inputs(render, rays if in_channels == 9 else None)


@functools.lru_cache(maxsize=None)
def _both(in_channels, channels, H, W):
    """The float64 twin and the float32 CPU module on one case, each run ONCE: logits and the 20 buffers of either."""
    from lidar_rt_amd.raydrop_refine import RaydropUNet
    net = network(in_channels, channels)
    x = case_input(in_channels, H, W)
    twin = RaydropUNet(in_channels, channels)
    twin.load_state_dict(net.state_dict())
    twin = twin.double().eval()
    z64, b64 = collect(twin, x.double())
    z32, b32 = collect(net, x)
    return z64, z32, b64, b32


@functools.lru_cache(maxsize=None)
def references(in_channels, channels, H, W):
    """(logits of the float64 twin (H, W) float64, logits of the float32 CPU module (H, W) float32, e_f32 = their largest difference)."""
    z64, z32, _, _ = _both(in_channels, channels, H, W)
    return z64, z32, float((z32.double() - z64).abs().max())


@functools.lru_cache(maxsize=None)
def layer_references(in_channels, channels, H, W):
    """({buffer: float64 (pixels, channels)} of the twin, the same in float32 of the CPU module, {buffer: e_f32 = their largest difference})."""
    _, _, b64, b32 = _both(in_channels, channels, H, W)
    return b64, b32, {b: float((b32[b].double() - b64[b]).abs().max()) for b in BUFFERS}


def layer_ratios(got, b64, e_f32):
    """{buffer: (e_op, allowance, e_op / allowance)} of one set of buffers against the twin's: e_op = max |got - twin|, the allowance is the float32
    module's own error on that buffer or, where that is smaller, half an ulp of the buffer's largest value.  The per-layer gate is ratio <= K_L."""
    out = {}
    for b in BUFFERS:
        assert got[b].shape == b64[b].shape, (b, got[b].shape, b64[b].shape)
        e_op = float((got[b].double() - b64[b]).abs().max())
        if not bool(torch.isfinite(got[b]).all()):
            e_op = math.inf
        allow = max(e_f32[b], 2.0 ** -24 * float(b64[b].abs().max()))
        out[b] = (e_op, allow, e_op / allow)
    return out


def rejected_layers(ratios, k_l):
    return [b for b in BUFFERS if not ratios[b][2] <= k_l]
