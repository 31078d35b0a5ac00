"""Shapes, seeded inputs and error constants shared by tests/test_dggm_ref.py (CPU: pins the
float64 checker, measures the constants) and tests/test_gpu_dggm_ragged.py (K2 against it).

The inputs are chosen so that an index error shows: white-noise gradient planes (neighbouring
source pixels are unrelated), a Bernoulli(0.5) mask (a nearest index off by one flips the gate
of every second pixel), N(0,1) weights and biases with |b| >= 0.05 (a masked-out pixel has
pre = b exactly, never near the ReLU kink)."""
import functools

import numpy as np
import torch

from checkers import dggm_ref

H, W, B = 97, 131, 2

# (C, h, w); PX is the kernel's vector width for h*w, 64*PX pixels per tile
SCALES = [
    (96, 25, 33),   # PX = 1, 13 tiles
    (40, 13, 17),   # PX = 1, C not a multiple of 32
    (32, 7, 9),     # PX = 1, one partial tile of 63 pixels
    (64, 4, 5),     # PX = 4, one partial tile
    (32, 30, 34),   # PX = 4, 4 tiles, last one partial
    (32, 24, 33),   # PX = 8, 2 tiles, last one partial
    (12, 5, 7),     # PX = 1, C not a multiple of 8 (NCHW cp1 only)
]
GROUPS = [(0, 1, 2, 3), (4, 5, 6)]  # the _multi entry points take at most four scales

# Error constants of the GPU bounds |hip - ref64| <= K * 2^-24 * (sum of magnitudes): twice the
# largest such ratio that torch's own float32 evaluation (oracle.dggm.dggm_forward and autograd
# through it, on the CPU) reaches against the checker on these inputs, rounded up.
# tests/test_dggm_ref.py measures the ratios and asserts that these values cover them.
# K_F is this large because torch's CPU build rounds the bilinear source coordinate
# scale * (dst + 0.5f) - 0.5f once (a fused multiply-add) where the checker rounds twice: a
# coordinate near 100 then differs by one ulp, 2^-17 of a pixel, all of which goes into the weight
# of two unrelated noise taps.  Measured: forward 499.64 (3.3 against the checker's fma variant),
# dW 6.45, db 1.46.  An index error moves an output by the order of A_out itself, 2^14 bounds.
K_F = 1000
K_B = 13
EPS = 2.0 ** -24


def px_of(h, w):
    return 8 if (h * w) % 8 == 0 else (4 if (h * w) % 4 == 0 else 1)


def tiles_of(h, w):
    return -(-(h * w) // (64 * px_of(h, w)))


@functools.lru_cache(maxsize=None)
def pixel_values(seed=20):
    """Shared, do not modify.  float32 [B,10,H,W]: noise in channels 0-5 (unused by K2, they put the DGGM planes at a
    channel offset inside the batch stride), white-noise gradient planes 6-8, Bernoulli mask 9."""
    g = torch.Generator().manual_seed(seed)
    pv = torch.randn((B, 10, H, W), generator=g)
    pv[:, 9] = (torch.rand((B, H, W), generator=g) < 0.5).float()
    return pv


def scale_inputs(k, dtype=torch.float32, seed=21):
    """color, cp1, dout [B,C,h,w] (rounded to ``dtype``, returned as float32), weight [C,3,1,1],
    bias [C] of scale k."""
    C, h, w = SCALES[k]
    g = torch.Generator().manual_seed(seed * 100 + k)
    color, cp1, dout = (torch.randn((B, C, h, w), generator=g).to(dtype).float() for _ in range(3))
    weight = torch.randn((C, 3, 1, 1), generator=g)
    sign = (torch.rand((C,), generator=g) < 0.5).float() * 2 - 1
    bias = sign * (0.05 + torch.randn((C,), generator=g).abs())
    return dict(color=color, cp1=cp1, dout=dout, weight=weight, bias=bias)


@functools.lru_cache(maxsize=None)
def case(k, dtype=torch.float32):
    """(inputs, ref) of scale k: the inputs with dout zeroed on the checker's near-zero set, and
    dggm_ref of them without cp1 (with cp1: out + cp1 and A_out + |cp1|).  Shared; do not modify."""
    pv = pixel_values()
    i = scale_inputs(k, dtype)
    near = dggm_ref.dggm_ref(pv[:, 6:9], pv[:, 9:10], i["color"], i["weight"], i["bias"])["near"]
    i["dout"] = i["dout"] * ~near
    return i, dggm_ref.dggm_ref(pv[:, 6:9], pv[:, 9:10], i["color"], i["weight"], i["bias"], dout=i["dout"])


def tail_tile_keep(k):
    """bool [B,1,h,w]: False on the last pixel tile of the last image (what a launch that
    skipped its tail tile would leave out of dW/db)."""
    C, h, w = SCALES[k]
    keep = np.ones((B, h * w), bool)
    keep[B - 1, (tiles_of(h, w) - 1) * 64 * px_of(h, w):] = False
    return torch.from_numpy(keep.reshape(B, 1, h, w))


# (in, out) resampling pairs of the exact index probes, two per case (rows, columns): the model's
# ragged cascades, the RealSense / NYUv2 last scales, a 1-pixel output and the identity
PROBES = [
    ((97, 25), (131, 33)), ((97, 13), (131, 17)), ((97, 7), (131, 9)), ((97, 4), (131, 5)),
    ((90, 23), (125, 32)), ((90, 12), (125, 16)), ((90, 6), (125, 8)), ((90, 3), (125, 4)),
    ((720, 23), (9, 1)), ((5, 5), (1280, 40)), ((480, 15), (5, 5)),
]
