"""Checker of the hot path's end-to-end mode: the arithmetic of hot_path.py restated in torch with
the colour maps left in the graph (the reference detaches them, custom_model.py:332-333), so
autograd gives the colour-map gradients the fused backward has to return:

    cp1_0 = c_0,  cp1_{k+1} = c_{k+1} + dsam_k(cp1_k)            custom_model.py:339-352
    cp2_k = c_k + enh_k(planes)                                   :354 (oracle.dggm.dggm_forward)
    out_k = cp1_k + cp2_k                                         :355
    dsam_k(x) = Proj3x3s2(x) + sum_{i<4} Conv3x3s2_i(x * m_i) + sum_{i<n_masks} b_i,  m_i = bit i of code

The masked-convolution statement is the one test_gpu_dsam_full.py checks K5 against; the region
codes are an input (the GPU tests pass the device decomposition's, ops.edsam_codes, so no mask
decision is made twice; the CPU pin passes the oracle's).  Runs in the dtype of its inputs
(float64 as the reference of the GPU tests)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import dggm as dggm_o, edsam, hot_path as hot_o


def dsam(x, code, n_masks, conv_w, conv_b, proj_w):
    """x [B,Ci,h,w]; code integer [B,h,w]; n_masks [B]; conv_w [4,Co,Ci,3,3]; conv_b [4,Co]."""
    y = F.conv2d(x, proj_w, stride=2, padding=1)
    for i in range(4):
        m = ((code >> i) & 1).to(x.dtype)[:, None]
        y = y + F.conv2d(x * m, conv_w[i], stride=2, padding=1)
    bias = torch.stack([conv_b[:int(n)].sum(0) for n in n_masks])
    return y + bias[:, :, None, None]


def forward(colors, pixel_values, codes, n_masks, sd, prefix=""):
    """The four backbone features.  ``colors``: the Swin maps (graph leaves when their gradients
    are wanted); ``codes``: three [B,h,w] integer region-code maps at the DSAM input sizes;
    ``sd``: parameters keyed like the reference module (oracle.hot_path.split_params); everything
    in one dtype and on one device."""
    _, dsam_p, dg_w, dg_b = hot_o.split_params(sd, prefix)
    cp1 = [colors[0]]
    for k in range(3):
        cp1.append(colors[k + 1] + dsam(cp1[k], codes[k].long(), n_masks, **dsam_p[k]))
    cp2 = dggm_o.dggm_forward(list(colors), pixel_values[:, 6:9], pixel_values[:, 9:10], dg_w, dg_b)
    return [a + b for a, b in zip(cp1, cp2)]


def oracle_codes(pixel_values, ratios, sizes):
    """(codes, n_masks, n_modes) of the CPU oracle's decomposition, pooled to ``sizes``."""
    decs = [edsam.decompose(pixel_values[b, 3:6].numpy(), float(ratios[b])) for b in range(pixel_values.shape[0])]
    codes = [torch.from_numpy(np.stack([edsam.pooled_codes(d["code"], h, w) for d in decs])) for h, w in sizes]
    return codes, [d["n_masks"] for d in decs], [d["n_modes"] for d in decs]


def state_dict_of(dsams, dg, dtype, device="cpu"):
    sd = {}
    for k, m in enumerate(dsams):
        for kk, v in m.state_dict().items():
            sd[f"dsam{k}.{kk}"] = v.detach().to(device, dtype)
    for kk, v in dg.state_dict().items():
        sd[f"depth_gradient_injection.{kk}"] = v.detach().to(device, dtype)
    return sd


def color_grads(colors, gouts, pixel_values, codes, n_masks, sd, dtype=torch.float64):
    """(features, colour-map gradients) of ``forward`` in ``dtype`` for upstream gradients ``gouts``."""
    cs = [c.detach().to(dtype).clone().requires_grad_(True) for c in colors]
    outs = forward(cs, pixel_values.to(dtype), codes, n_masks, sd)
    torch.autograd.backward(outs, [g.to(dtype) for g in gouts])
    return [o.detach() for o in outs], [c.grad for c in cs]
