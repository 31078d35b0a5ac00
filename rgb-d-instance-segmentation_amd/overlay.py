"""f5: a prediction painted over its frame on the device (csrc/overlay.hip).

The reference's last step with a prediction is an alpha blend of every segment's colour over the
frame on the host (mask2former/predictor.py:295-330 ``_create_gt_overlay_with_consistent_colors``,
:1286-1320 ``_create_prediction_overlay``).  Here the map stays where post-processing left it:
``build_lut`` turns the arrays ``rgbd_pp_instance`` writes into a per-image colour table without a
host round trip (the form a captured stream uses, stream.StreamingSegmenter), ``blend`` paints,
and ``overlay_segments`` is the reference's call shape: HF-format results and an id -> colour
mapping in, a device uint8 image out, bit for bit the reference's arithmetic under NumPy 2.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import RGBD_F32, RGBD_I32, check
from .ops import _need_cuda, _p, _stream

DEFAULT_COLOR = (128, 128, 128)  # the reference's colour for an id its mapping does not hold


def consistent_colors(n, seed=42):
    """The palette of the reference's ``generate_consistent_colors`` (predictor.py:158-178): n
    (r, g, b) tuples of ints in [50, 255).  Drawn from a private ``RandomState(seed)`` — the stream
    ``np.random.seed(seed)`` gives the reference — so the global NumPy state is left alone (the
    reference reseeds it from the OS afterwards)."""
    rs = np.random.RandomState(seed)
    return [tuple(int(rs.randint(50, 255)) for _ in range(3)) for _ in range(n)]


def _palette(palette, dev):
    if isinstance(palette, torch.Tensor):
        pal = palette.to(device=dev, dtype=torch.uint8).reshape(-1, 3).contiguous()
    else:
        arr = np.asarray(palette)
        if arr.size == 0 or arr.min() < 0 or arr.max() > 255:
            raise ValueError("palette: a non-empty list of (r, g, b) values in 0..255 expected")
        pal = torch.from_numpy(arr.astype(np.uint8).reshape(-1, 3)).to(dev)
    if pal.shape[0] == 0:
        raise ValueError("palette: at least one colour expected")
    return pal


def build_lut(seg_id, topk_idx, num_labels, palette, color_by="label", n_ids=None, out=None):
    """seg_id, topk_idx: the int32 [B,Q] arrays of ``rgbd_pp_instance``; palette: uint8 [n,3] on
    the device (or a list of tuples, copied) -> int32 [B,n_ids] colour table (n_ids defaults to
    Q: segment ids are positions among the kept queries).  ``color_by``: "label" colours a segment
    by its class, "id" by its segment id."""
    _need_cuda(seg_id, topk_idx)
    if seg_id.dtype != torch.int32 or topk_idx.dtype != torch.int32 or seg_id.dim() != 2 \
            or seg_id.shape != topk_idx.shape:
        raise ValueError("seg_id and topk_idx must be int32 [B,Q]")
    if color_by not in ("label", "id"):
        raise ValueError(f"color_by {color_by!r}: 'label' or 'id' expected")
    B, Q = seg_id.shape
    n_ids = Q if n_ids is None else int(n_ids)
    pal = _palette(palette, seg_id.device)
    _need_cuda(pal)
    if out is None:
        out = torch.empty((B, n_ids), dtype=torch.int32, device=seg_id.device)
    check(_lib.lib().rgbd_overlay_lut(_p(seg_id), _p(topk_idx), B, Q, int(num_labels), _p(pal), pal.shape[0],
                                      0 if color_by == "label" else 1, _p(out), n_ids, _stream(seg_id.device)),
          "rgbd_overlay_lut")
    return out


def blend(rgb_u8, seg, lut, alpha=0.6, out=None):
    """rgb_u8 uint8 [B,H,W,3], seg float32 | int32 [B,H,W], lut int32 [B,n_ids], all on the
    device -> uint8 [B,H,W,3]: the pixels whose id has a colour blended, the others copied."""
    _need_cuda(rgb_u8, seg, lut, out)
    if rgb_u8.dtype != torch.uint8 or rgb_u8.dim() != 4 or rgb_u8.shape[3] != 3:
        raise ValueError("rgb_u8 must be uint8 [B,H,W,3]")
    B, H, W = rgb_u8.shape[:3]
    if tuple(seg.shape) != (B, H, W) or seg.dtype not in (torch.float32, torch.int32):
        raise ValueError("seg must be float32 or int32 [B,H,W], one map per image")
    if lut.dtype != torch.int32 or lut.dim() != 2 or lut.shape[0] != B:
        raise ValueError("lut must be int32 [B,n_ids]")
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=rgb_u8.device)
    elif out.dtype != torch.uint8 or out.shape != rgb_u8.shape:
        raise ValueError("out must be uint8 [B,H,W,3]")
    check(_lib.lib().rgbd_overlay_blend(_p(rgb_u8), _p(seg), RGBD_F32 if seg.dtype == torch.float32 else RGBD_I32,
                                        _p(lut), B, H, W, lut.shape[1], ctypes.c_double(float(alpha)), _p(out),
                                        _stream(rgb_u8.device)), "rgbd_overlay_blend")
    return out


def overlay_segments(image_u8, segmentation, colors, alpha=0.6):
    """The device form of ``_create_gt_overlay_with_consistent_colors`` (and of
    ``_create_prediction_overlay`` with the colours given rather than drawn).

    image_u8: uint8 [H,W,3] or [B,H,W,3] on the device; segmentation: one HF-format result
    ``{"segmentation", "segments_info"}`` or a list of B of them, maps on the device (float32 or
    int32; int64 class maps are narrowed); colors: {id: (r, g, b)}, an id of segments_info it
    does not hold takes the reference's grey.  -> uint8 image(s) on the device, same shape."""
    single = isinstance(segmentation, dict)
    results = [segmentation] if single else list(segmentation)
    img = image_u8[None] if image_u8.dim() == 3 else image_u8
    _need_cuda(img)
    if len(results) != img.shape[0]:
        raise ValueError("one segmentation result per image expected")
    maps = []
    for r in results:
        m = r["segmentation"]
        if not isinstance(m, torch.Tensor):
            raise TypeError("segmentation maps must be torch tensors on the device")
        _need_cuda(m)
        maps.append(m.to(torch.int32) if m.dtype == torch.int64 else m)
    if len({m.dtype for m in maps}) != 1:  # e.g. a panoptic batch with a "nothing kept" float32 map
        maps = [m.to(torch.float32) for m in maps]
    seg = maps[0][None] if len(maps) == 1 else torch.stack(maps)
    ids = [[int(s["id"]) for s in r["segments_info"]] for r in results]
    n_ids = max([i + 1 for row in ids for i in row if i >= 0], default=1)
    table = np.full((len(results), n_ids), -1, dtype=np.int32)
    for b, row in enumerate(ids):
        for i in row:
            if i >= 0:
                r, g, bl = (int(v) for v in colors.get(i, DEFAULT_COLOR))
                table[b, i] = r | (g << 8) | (bl << 16)
    lut = torch.from_numpy(table).to(img.device)
    out = blend(img, seg, lut, alpha)
    return out[0] if image_u8.dim() == 3 else out
