"""The overlay sweep shared by tests/test_gpu_overlay.py and tests/test_gpu_overlay_guard.py: small
inputs at the sizes where the blend kernels can go wrong, their expected outputs from the numpy
checker (computed once), and a raw C-ABI call on buffers the caller allocates, at any byte offset.

Shapes (B, H, W): one pixel; an image of 15 pixels, smaller than a 16-pixel group; 147 pixels per
image, so groups straddle images and the flat range ends in a partial group; whole groups only;
12771 pixels = 798 groups and a tail of 3, four workgroups of 256 lanes.
"""
import ctypes
import functools

import numpy as np
import torch

from checkers import overlay_ref
from rgbd_amd import _lib

SHAPES = [(1, 1, 1), (1, 3, 5), (3, 7, 21), (2, 16, 64), (3, 33, 129)]
OFFSETS = [0, 1, 7]          # bytes into the allocation: 0 takes the 16-byte path, the others the byte path
DTYPES = ["f32", "i32"]
N_IDS = 5
ALPHA = 0.37


@functools.lru_cache(maxsize=None)
def case(shape, dtype):
    """-> (rgb uint8 [B,H,W,3], seg [B,H,W], lut int32 [B,N_IDS], expected uint8 [B,H,W,3])."""
    B, H, W = shape
    rng = np.random.RandomState(1000 + B * 7 + H * 13 + W)
    rgb = rng.randint(0, 256, size=(B, H, W, 3)).astype(np.uint8)
    seg = rng.randint(-1, N_IDS + 2, size=(B, H, W))  # -1 = none, N_IDS and N_IDS + 1 lie past the table
    seg = seg.astype(np.float32 if dtype == "f32" else np.int32)
    if dtype == "f32" and seg.size > 4:
        seg.flat[1], seg.flat[3] = 1.5, np.nan         # cells that name no id
    lut = rng.randint(0, 1 << 24, size=(B, N_IDS)).astype(np.int32)
    lut[:, 2] = -1                                      # an id without a colour
    lut[B - 1, 0] = -1                                  # tables differ between images
    lut[0, 1] = 255 | (255 << 8) | (255 << 16)
    return rgb, seg, lut, overlay_ref.blend(rgb, seg, lut, ALPHA)


def run_raw(rgb, seg, lut, alpha, off, alloc=None):
    """rgbd_overlay_blend on device copies of the arrays placed ``off`` bytes into their buffers.
    ``alloc(nbytes) -> uint8 device tensor`` (default torch.empty).  -> (out uint8 array, the three
    offset buffers' leading ``off`` bytes after the call, as one array)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    alloc = alloc or (lambda n: torch.empty((n,), dtype=torch.uint8, device=dev))
    B, H, W = seg.shape

    def put(arr):
        raw = torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1))
        buf = alloc(raw.numel() + off)
        buf[:off] = 0xA5
        buf[off:].copy_(raw)
        return buf
    b_rgb, b_seg = put(rgb), put(seg)
    b_out = alloc(rgb.size + off)
    b_out.fill_(0xA5)
    d_lut = torch.from_numpy(lut).to(dev)
    code = _lib.RGBD_F32 if seg.dtype == np.float32 else _lib.RGBD_I32
    rc = _lib.lib().rgbd_overlay_blend(ctypes.c_void_p(b_rgb.data_ptr() + off), ctypes.c_void_p(b_seg.data_ptr() + off),
                                       code, ctypes.c_void_p(d_lut.data_ptr()), B, H, W, lut.shape[1],
                                       ctypes.c_double(alpha), ctypes.c_void_p(b_out.data_ptr() + off),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, f"rgbd_overlay_blend returned {rc}"
    out = b_out[off:].cpu().numpy().reshape(rgb.shape)
    lead = torch.cat([b_rgb[:off], b_seg[:off], b_out[:off]]).cpu().numpy()
    assert (b_rgb[off:].cpu().numpy() == np.ascontiguousarray(rgb).reshape(-1)).all(), "the input image was written"
    return out, lead
