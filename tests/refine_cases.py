"""Shared cases of the ray-drop refinement tests: the golden fixture, seeded networks with randomised batch-norm statistics, frames as the
renderer produces them, and the references (float64 twin and float32 CPU module), computed once per case and handed out unchanged."""
import functools
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refine_unet.npz")
LOGIT_04 = math.log(0.4 / 0.6)                                               # sigmoid(z) < 0.4  <=>  z < logit(0.4)
GOLDEN_SHAPES = ((9, 18, 38), (9, 33, 75), (3, 16, 32))


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


@functools.lru_cache(maxsize=None)
def references(in_channels, channels, H, W):
    """(logits of the float64 twin (H, W) float64, logits of the float32 CPU module (H, W) float32, e_f32 = their largest difference)."""
    from lidar_rt_amd.raydrop_refine import RaydropUNet, refine_inputs
    net = network(in_channels, channels)
    render, rays = frame(H, W)
    x = refine_inputs(render, rays if in_channels == 9 else None)
    twin = RaydropUNet(in_channels, channels)
    twin.load_state_dict(net.state_dict())
    twin = twin.double().eval()
    with torch.no_grad():
        z64 = twin.logits(x.double()).reshape(H, W)
        z32 = net.logits(x).reshape(H, W)
    return z64, z32, float((z32.double() - z64).abs().max())
