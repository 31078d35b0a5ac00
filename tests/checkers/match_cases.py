"""The segment-matching sweep shared by tests/test_gpu_segment_match.py and
tests/test_gpu_segment_match_guard.py: small maps and tables at the sizes where the kernels can go
wrong, expected outputs from the numpy checker (computed once per case), and raw C-ABI calls on
buffers the caller allocates.

Shapes (B, H, W): one pixel; 15 pixels, fewer than one wave; 147 pixels per image, so 4-cell groups
straddle images and the flat range ends in a partial group; whole groups only; 4257 pixels per image
= more than one workgroup pass of 1024 cells per image, odd, with a tail.

Id ranges (na, nb) and the accumulation path each takes — the table (na+1)(nb+1) int32 against the
160 KB of LDS: (1, 1) 16 B, (5, 7) 192 B, (100, 100) 40.8 KB and (100, 256) 103.8 KB go through the
LDS table; (256, 256) is 264 KB and goes straight to the global table.
"""
import ctypes
import functools

import numpy as np
import torch

from checkers import match_ref
from rgbd_amd import _lib

SHAPES = [(1, 1, 1), (1, 3, 5), (3, 7, 21), (2, 16, 64), (3, 33, 129)]
OFFSETS = [0, 4, 8, 12]      # bytes into the allocation: only (0, 0) takes the 16-byte loads
DTYPES = ["f32", "i32"]
RANGES = [(1, 1), (5, 7), (100, 100), (100, 256), (256, 256)]
LDS_RANGES = RANGES[:4]
KINDS = ["blocks", "noise"]


def _one_map(rng, shape, n, dtype, kind):
    B, H, W = shape
    if kind == "blocks":  # piecewise constant: the lanes of a wave share keys
        bh, bw = rng.randint(2, 6), rng.randint(3, 40)
        y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        base = (y // bh) * 7 + x // bw
        m = np.stack([(base + 3 * b) % (n + 1) - (1 if n > 1 else 0) for b in range(B)])
    else:                 # per-pixel noise: they do not
        m = rng.randint(-1, n + 1, size=shape)
    m = m.astype(np.float32 if dtype == "f32" else np.int32)
    k = m.size
    if k > 8:  # cells that name no id: NaN, a fraction, -1, the first id past the range
        at = rng.choice(k, size=min(k // 4, 8), replace=False)
        vals = [np.nan, 1.5, -1, n] if dtype == "f32" else [-7, 1 << 30, -1, n]
        for i, p in enumerate(at):
            m.flat[p] = vals[i % 4]
    return m


@functools.lru_cache(maxsize=None)
def contingency_case(shape, ranges, dtypes, kind):
    """-> (a, b, expected counts int32 [B,na+1,nb+1])."""
    na, nb = ranges
    rng = np.random.RandomState(2000 + sum(shape) * 31 + na * 7 + nb + 100 * KINDS.index(kind))
    a = _one_map(rng, shape, na, dtypes[0], kind)
    b = _one_map(rng, shape, nb, dtypes[1], kind)
    return a, b, match_ref.contingency(a, b, na, nb)


def _code(arr):
    return _lib.RGBD_F32 if arr.dtype == np.float32 else _lib.RGBD_I32


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_contingency_raw(a, b, na, nb, off_a=0, off_b=0, alloc=None):
    """rgbd_label_contingency on device copies placed ``off`` bytes into their buffers; the table
    is pre-filled with garbage (it is documented as overwritten).  -> (counts array, the maps'
    leading bytes after the call)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    alloc = alloc or (lambda n: torch.empty((n,), dtype=torch.uint8, device=dev))
    B, H, W = a.shape

    def put(arr, off):
        raw = torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1))
        buf = alloc(raw.numel() + off)
        buf[:off] = 0xA5
        buf[off:].copy_(raw)
        return buf
    b_a, b_b = put(a, off_a), put(b, off_b)
    n_out = B * (na + 1) * (nb + 1) * 4
    b_out = alloc(n_out)
    b_out.fill_(0x5A)
    rc = _lib.lib().rgbd_label_contingency(ctypes.c_void_p(b_a.data_ptr() + off_a), _code(a),
                                           ctypes.c_void_p(b_b.data_ptr() + off_b), _code(b), B, H, W, na, nb,
                                           ctypes.c_void_p(b_out.data_ptr()), _stream())
    assert rc == 0, f"rgbd_label_contingency returned {rc}"
    out = b_out.cpu().numpy().view(np.int32).reshape(B, na + 1, nb + 1)
    lead = torch.cat([b_a[:off_a], b_b[:off_b]]).cpu().numpy()
    return out, lead


@functools.lru_cache(maxsize=None)
def table_case(P, G, seed=0):
    """A random integer table with P and G listed segments -> (counts int32 [B,na+1,nb+1], a_list
    [B,La], b_list [B,Lb], hw).  Small counts, so equal IoUs abound; a few rows and columns pair
    off exactly (IoU 1); the lists are shuffled, -1 padded, and name some empty segments and ids
    outside the table."""
    B = 3
    rng = np.random.RandomState(3000 + 17 * P + G + seed)
    na, nb = max(P, 1) + 2, max(G, 1) + 3
    counts = np.zeros((B, na + 1, nb + 1), np.int32)
    for b in range(B):
        for i in range(na):
            for j in rng.choice(nb + 1, size=min(3, nb + 1), replace=False):
                counts[b, i, j] = rng.randint(0, 5)
        counts[b, na, :] = rng.randint(0, 4, size=nb + 1)
        for d in range(0, min(na, nb), 3):   # exact pairs
            counts[b, d, :], counts[b, :, d] = 0, 0
            counts[b, d, d] = rng.randint(1, 9)
        for e in range(1, min(na, nb), 5):   # empty segments that stay listed
            counts[b, e, :] = 0
    def lists(n_listed, n_ids):
        L = max(n_listed, 1) + 2
        out = np.full((B, L), -1, np.int32)
        for b in range(B):
            ids = rng.permutation(n_ids)[:n_listed]
            pos = np.sort(rng.choice(L, size=len(ids), replace=False))
            out[b, pos] = ids
            if n_listed >= 7:
                out[b, pos[0]] = n_ids + 5   # an id outside the table: names nothing
        return out
    return counts, lists(P, na), lists(G, nb), max(1, int(counts.sum(axis=(1, 2)).max()))


def run_match_raw(counts, a_list, b_list, hw, thr, place=None, new=None):
    """rgbd_greedy_iou_match -> (matched, b_match_count, n_filtered) arrays.  ``place(tensor)`` puts
    an input on the device, ``new(shape)`` allocates an int32 output (both default to torch)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    place = place or (lambda t: t.to(dev))
    new = new or (lambda shape: torch.empty(shape, dtype=torch.int32, device=dev))
    B, na, nb = counts.shape[0], counts.shape[1] - 1, counts.shape[2] - 1
    d_c, d_a, d_b = (place(torch.from_numpy(np.ascontiguousarray(x))) for x in (counts, a_list, b_list))
    La, Lb = a_list.shape[1], b_list.shape[1]
    outs = [new((B, La)), new((B, Lb)), new((B, 2))]
    for o in outs:
        o.fill_(0x5A5A5A5A)
    rc = _lib.lib().rgbd_greedy_iou_match(ctypes.c_void_p(d_c.data_ptr()), B, na, nb, hw,
                                          ctypes.c_void_p(d_a.data_ptr()), La, ctypes.c_void_p(d_b.data_ptr()), Lb,
                                          ctypes.c_double(thr), *[ctypes.c_void_p(o.data_ptr()) for o in outs], _stream())
    assert rc == 0, f"rgbd_greedy_iou_match returned {rc}"
    return tuple(o.cpu().numpy() for o in outs), (d_c, d_a, d_b, *outs)
