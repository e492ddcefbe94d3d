"""Write tests/golden/refine_unet.npz from the reference's own ray-drop U-Net.

    python tools/gen_refine_golden.py --reference /path/to/LiDAR-RT [--out tests/golden/refine_unet.npz]

Run by hand where a checkout of the reference exists; no test runs it.  It imports ``lib/scene/unet.py`` of that tree, builds the network at
``channels=4`` with 9 and with 3 inputs under a fixed seed, and RANDOMISES every batch norm's running mean, running variance, weight and bias:
with the default statistics a batch norm is the identity, which hides the relu(b_c) of padded pixels and every mistake in folding.  The
networks are put in eval() and run in float32 on the CPU.  The file holds data only:

    names9 / names3            the state_dict's names, in order
    p9_<i>                     the i-th array of the 9-input state_dict
    p3_0                       the 3-input network's first array (inc.conv.weight); its other 111 arrays are the 9-input network's
    x9_18x38, x9_33x75         inputs (1, 9, H, W) float32;  prob9_<H>x<W>, logit9_<H>x<W>: the outputs (1, 1, H, W) float32
    x3_16x32, prob3_16x32, logit3_16x32
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch


def randomise_bn(net, g):
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            n = m.num_features
            m.running_mean.copy_(torch.randn(n, generator=g) * 0.5)
            m.running_var.copy_(torch.rand(n, generator=g) * 1.5 + 0.5)
            with torch.no_grad():
                m.weight.copy_(torch.rand(n, generator=g) + 0.5)
                m.bias.copy_(torch.randn(n, generator=g) * 0.3)


def frame(C, H, W, g):
    """Inputs as the renderer produces them: probability, intensity, depth 0..80 m, origins, unit directions."""
    x = torch.rand((1, C, H, W), generator=g)
    x[:, 2] *= 80.0
    if C == 9:
        x[:, 3:6] = torch.randn((1, 3, 1, 1), generator=g).expand(1, 3, H, W) * 10.0
        d = torch.randn((1, 3, H, W), generator=g)
        x[:, 6:9] = d / d.norm(dim=1, keepdim=True)
    return x


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="root of a checkout of the reference")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "refine_unet.npz"))
    a = ap.parse_args(argv)
    spec = importlib.util.spec_from_file_location("reference_unet", os.path.join(a.reference, "lib", "scene", "unet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {}
    for C, shapes, seed in ((9, ((18, 38), (33, 75)), 1234), (3, ((16, 32),), 4321)):
        torch.manual_seed(seed)
        g = torch.Generator().manual_seed(seed + 1)
        net = mod.UNet(in_channels=C, channels=4, out_channels=1)
        if C == 9:
            randomise_bn(net, g)
            first = net.state_dict()
        else:                                                                # the same network behind another input convolution: one array more
            own = net.state_dict()
            net.load_state_dict({k: (own[k] if k == "inc.conv.weight" else v) for k, v in first.items()})
        net.eval()
        sd = net.state_dict()
        out[f"names{C}"] = np.array(list(sd.keys()))
        for i, (k, v) in enumerate(sd.items()):
            if C == 9 or k == "inc.conv.weight":
                out[f"p{C}_{i}"] = v.detach().numpy()
        for H, W in shapes:
            x = frame(C, H, W, g)
            grab = {}
            hook = net.outc.register_forward_hook(lambda m, i, o: grab.__setitem__("z", o.detach()))
            with torch.no_grad():
                p = net(x)
            hook.remove()
            out[f"x{C}_{H}x{W}"] = x.numpy()
            out[f"prob{C}_{H}x{W}"] = p.numpy()
            out[f"logit{C}_{H}x{W}"] = grab["z"].numpy()
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
