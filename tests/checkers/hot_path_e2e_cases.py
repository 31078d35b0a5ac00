"""Inputs of the end-to-end hot-path tests (GPU) and of the checker's CPU pin: synthetic scenes,
injected ratios, deterministic weights, random colour maps and upstream gradients."""
import torch

import golden_inputs as gi
from rgbd_amd import init as winit

CH = [96, 192, 384, 768]
# (synthetic config id, B, H, W): maps 13x18, 7x9, 4x5, 2x3 and 16x24, 8x12, 4x6, 2x3.  No case
# with fewer than three depth modes (Q6): oracle.edsam.decompose finds three in every synthetic
# scene at these sizes (config ids 0-399 scanned at both), so synthetic cannot supply one.
CASES = [(21, 2, 52, 72), (22, 3, 64, 96)]


def modules():
    from rgbd_amd.modules import DSAModule, DepthGradientInjectionResidual
    pre = "model.pixel_level_module."
    dsams = []
    for k in range(3):
        m = DSAModule(CH[k], CH[k + 1])
        winit.init_deterministic(m, prefix=f"{pre}dsam{k}.")
        dsams.append(m)
    dg = DepthGradientInjectionResidual(CH, 3)
    winit.init_deterministic(dg, prefix=f"{pre}depth_gradient_injection.")
    return dsams, dg


def inputs(case):
    """-> (pixel_values [B,10,H,W], ratios [B], colour maps, upstream gradients, DSAM input sizes), CPU float32."""
    cid, B, H, W = CASES[case]
    pv = torch.from_numpy(gi.pixel_values(cid, B, H, W))
    ratios = torch.linspace(0.05, 0.45, B)
    sizes = gi.swin_sizes(H, W)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(1000 + case)
    colors = [torch.randn((B, c, *sizes[k]), generator=gen) for k, c in enumerate(CH)]
    gouts = [torch.randn((B, c, *sizes[k]), generator=gen) for k, c in enumerate(CH)]
    return pv, ratios, colors, gouts, sizes[:3]


def n_modes(case):
    from oracle import edsam
    pv, ratios, _, _, _ = inputs(case)
    return [edsam.decompose(pv[b, 3:6].numpy(), float(ratios[b]))["n_modes"] for b in range(pv.shape[0])]
