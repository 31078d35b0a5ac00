"""Masks, label maps and the raw C-ABI call for the device RLE encoder's tests
(tests/test_gpu_rle_encode.py, tests/test_gpu_rle_encode_guard.py).  The expected values come from
oracle/rle.py alone: ``encode(mask)["counts"]``, ``bbox_from_mask`` and ``mask.sum()``."""
import numpy as np

from oracle import rle

SIZES = [(24, 40), (23, 37), (97, 131), (128, 160)]
CHUNK_H = 97

_seen = {}


def expected(mask):
    """(counts string, bbox or None, area) of one [h, w] 0/1 mask; computed once per distinct mask."""
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    key = (m.shape, m.tobytes())
    if key not in _seen:
        _seen[key] = (rle.encode(m)["counts"], rle.bbox_from_mask(m), int(m.sum()))
    return _seen[key]


def from_column_major(flat, h, w):
    return np.asarray(flat, np.uint8).reshape(w, h).T.copy()


def from_counts(counts, h, w):
    """The mask whose counts begin with ``counts`` (the last run closes it)."""
    L, s = h * w, sum(counts)
    assert s <= L
    full = list(counts) + ([L - s] if s < L else [])
    m = rle.rle_decode(h, w, full)
    return m


def masks_of(h, w, seed=0):
    """name -> [h, w] uint8 mask: the cases every size takes."""
    L = h * w
    y, x = np.mgrid[:h, :w]
    rng = np.random.RandomState(seed + h)
    out = {
        "all_zero": np.zeros((h, w), np.uint8),
        "all_one": np.ones((h, w), np.uint8),                       # a leading 0 count
        "pixel_0": from_column_major([1] + [0] * (L - 1), h, w),
        "last_pixel": from_column_major([0] * (L - 1) + [1], h, w),
        # alternating in maskApi's order (a spatial checkerboard when h is odd): h w counts, or
        # h w + 1 from a set pixel 0, every one a single character
        "checkerboard": from_column_major(np.arange(L) % 2, h, w),
        "checkerboard_from_1": from_column_major((np.arange(L) + 1) % 2, h, w),
        "checkerboard_xy": ((x + y) % 2).astype(np.uint8),          # h even: runs of two across the column seams
        "vertical_stripes": (x % 3 == 1).astype(np.uint8),          # whole columns: one run each
        "horizontal_stripes": (y % 3 == 1).astype(np.uint8),        # a run per column and stripe
        "bar_two_columns": ((x >= 5) & (x < 7)).astype(np.uint8),   # one run across the column seam
        "neg_one_group": from_counts([10, 14, 9, 3, 1, 2], h, w),
        "neg_two_groups": from_counts([10, 300, 200, 20, 3, 4], h, w),
        "blobs": np.zeros((h, w), np.uint8),
        "noise": (rng.rand(h, w) < 0.3).astype(np.uint8),
    }
    short = out["bar_two_columns"].copy()
    short[h - 1, 5] = 0                                             # one pixel short of the seam: two runs
    out["bar_one_short"] = short
    for _ in range(4):
        y0, x0 = rng.randint(0, h - 2), rng.randint(0, w - 2)
        out["blobs"][y0:y0 + rng.randint(1, h // 2), x0:x0 + rng.randint(1, w // 2)] = 1
    out["blobs"] &= (rng.rand(h, w) < 0.9).astype(np.uint8)
    if L > 2000:
        out["neg_three_groups"] = from_counts([3, 900, 880, 100, 60, 17], h, w)
    assert len(expected(out["checkerboard_from_1"])[0]) == L + 1 and len(expected(out["checkerboard"])[0]) == L
    return out


def chunk_width(chunk):
    """The smallest w with 97 w >= 2 chunk + 2."""
    return -(-(2 * chunk + 2) // CHUNK_H)


def chunk_masks(chunk):
    """Runs that end at chunk - 1, chunk and chunk + 1 cells, and one run that spans 2 chunk + 1
    cells from cell 1, in column-major order; set runs and their complements (unset runs)."""
    h, w = CHUNK_H, chunk_width(chunk)
    L = h * w
    out = {}
    for name, n in (("chunk-1", chunk - 1), ("chunk", chunk), ("chunk+1", chunk + 1), ("2chunk-1", 2 * chunk - 1),
                    ("2chunk", 2 * chunk), ("2chunk+1", 2 * chunk + 1)):
        flat = np.zeros(L, np.uint8)
        flat[:n] = 1
        out[f"ones_to_{name}"] = from_column_major(flat, h, w)
        out[f"zeros_to_{name}"] = from_column_major(1 - flat, h, w)
    flat = np.zeros(L, np.uint8)
    flat[1:2 * chunk + 2] = 1
    out["span_2chunk+1"] = from_column_major(flat, h, w)
    flat = np.zeros(L, np.uint8)
    flat[chunk - 1] = flat[chunk] = flat[2 * chunk] = 1     # boundaries on both sides of each chunk edge
    out["pixels_at_the_edges"] = from_column_major(flat, h, w)
    return out


def label_map(h, w, n_seg, seed, background=-1):
    """An int64 [h, w] map of ``n_seg`` segments (ids 1 .. n_seg; rectangles painted over each other,
    then noise) over ``background``; some ids may end up without pixels."""
    rng = np.random.RandomState(seed)
    m = np.full((h, w), background, np.int64)
    for i in range(1, n_seg + 1):
        y0, x0 = rng.randint(0, h - 1), rng.randint(0, w - 1)
        m[y0:y0 + rng.randint(1, max(2, h // 3)), x0:x0 + rng.randint(1, max(2, w // 3))] = i
    noisy = rng.rand(h, w) < 0.05
    m[noisy] = rng.randint(1, n_seg + 1, int(noisy.sum()))
    return m


def raw_encode(mode, src, ids, n_images, n_masks, H, W, cap_counts, cap_chars, n_ids=256, guard_pool=None):
    """The C-ABI call on device tensors -> dict of device tensors chars / offsets / info / totals
    (int64 [2]) / ws.  ``guard_pool``: a checkers.guard.Pool to allocate every buffer from."""
    import torch
    from rgbd_amd import _lib
    from rgbd_amd.ops import _p, _stream
    L = _lib.lib()
    dev = src.device

    def new(shape, dtype, tag):
        if guard_pool is not None:
            return guard_pool.new(shape, dtype, dev, tag=tag).payload
        return torch.empty(shape, dtype=dtype, device=dev)
    out = {"chars": new((cap_chars,), torch.uint8, "chars"),
           "offsets": new((n_masks + 1,), torch.int32, "offsets"), "info": new((n_masks, 8), torch.int32, "info"),
           "totals": new((2,), torch.int64, "totals"),
           "ws": new((L.rgbd_rle_encode_workspace_size(mode, n_images, n_masks, H, W, cap_counts),), torch.uint8, "ws")}
    chars_p = _p(out["chars"]) if cap_chars > 0 else _p(out["ws"])  # a zero-size buffer: any non-null address
    if mode == 0:
        dtype = _lib.RGBD_F32 if src.dtype == torch.float32 else _lib.RGBD_I32
        rc = L.rgbd_rle_encode_labels(dtype, _p(src), n_images, H, W, n_ids, _p(ids), n_masks // n_images, cap_counts,
                                      cap_chars, chars_p, _p(out["offsets"]), _p(out["info"]), _p(out["totals"]),
                                      _p(out["ws"]), _stream(dev))
    else:
        rc = L.rgbd_rle_encode_stack(_p(src), n_masks, H, W, cap_counts, cap_chars, chars_p, _p(out["offsets"]),
                                     _p(out["info"]), _p(out["totals"]), _p(out["ws"]), _stream(dev))
    assert rc == 0, rc
    return out


def capacity(mode, n_images, n_masks, H, W):
    import ctypes
    from rgbd_amd import _lib
    c, ch = ctypes.c_longlong(), ctypes.c_longlong()
    assert _lib.lib().rgbd_rle_encode_capacity(mode, n_images, n_masks, H, W, ctypes.byref(c), ctypes.byref(ch)) == 0
    return c.value, ch.value


def strings_of(raw):
    """The per-mask strings of a raw_encode result (host)."""
    off = raw["offsets"].cpu().numpy()
    text = raw["chars"][:int(off[-1])].cpu().numpy().tobytes().decode("ascii")
    return [text[off[m]:off[m + 1]] for m in range(len(off) - 1)]
