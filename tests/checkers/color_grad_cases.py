"""Job tables for rgbd_color_grads, shared by test_gpu_color_grads.py and the guard-band test, and
the torch statement the kernel is held to bit for bit:

    out = (G.float() + D_as_nchw.float()).to(G.dtype)        D absent: G + G
"""
import torch

RAGGED = [(2, 96, 13, 18), (2, 192, 7, 9), (2, 384, 4, 5), (2, 768, 2, 3)]   # pixel counts not multiples of 8
ALIGNED = [(1, 96, 16, 24), (1, 192, 8, 12), (1, 384, 4, 6), (1, 768, 2, 3)]  # the 16-byte path (but the last)
SINGLE = [(3, 40, 7, 9)]
TABLES = {"ragged": RAGGED, "aligned": ALIGNED, "single": SINGLE}
# D as the hot path's three precision modes leave it, and absent
LAYOUTS = {"nchw_f32": (False, torch.float32), "nhwc_bf16": (True, torch.bfloat16),
           "nhwc_f32": (True, torch.float32), "none": None}


def make_jobs(shapes, g_dtype, layouts, device, seed=0):
    """-> (G_list, D_list, nhwc indices): random values; ``layouts`` one LAYOUTS key per job."""
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)
    Gs, Ds, nhwc = [], [], []
    for i, (shape, lay) in enumerate(zip(shapes, layouts)):
        B, C, H, W = shape
        Gs.append(torch.randn(shape, generator=gen).to(g_dtype).to(device))
        if LAYOUTS[lay] is None:
            Ds.append(None)
            continue
        is_nhwc, dt = LAYOUTS[lay]
        d = (torch.randn((B, H, W, C) if is_nhwc else shape, generator=gen) * 3).to(dt).to(device)
        Ds.append(d)
        if is_nhwc:
            nhwc.append(i)
    return Gs, Ds, tuple(nhwc)


def expected(Gs, Ds, nhwc):
    out = []
    for i, (g, d) in enumerate(zip(Gs, Ds)):
        if d is None:
            d = g
        elif i in nhwc:
            d = d.permute(0, 3, 1, 2)
        out.append((g.float() + d.float()).to(g.dtype))
    return out
