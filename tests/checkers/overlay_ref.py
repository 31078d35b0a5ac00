"""Numpy restatement of the overlay (csrc/overlay.hip): the colour table built from the arrays
rgbd_pp_instance writes, and the blend of the reference's
_create_gt_overlay_with_consistent_colors / _create_prediction_overlay
(mask2former/predictor.py:295-330, :1286-1320).

The reference blends on a float32 copy of the image with Python-float weights; under NumPy 2
promotion (NEP 50) a Python float takes the array's dtype, so per channel

    v = float32(1 - alpha) * float32(x) + float32(alpha * c)

with the product and the sum each rounded to float32, then ``np.clip(v, 0, 255).astype(uint8)``.
``blend`` spells the casts out so that it does not depend on the promotion rules of the NumPy it
runs under (tests/test_overlay_ref.py pins it to the reference's own output, G10).
"""
import numpy as np


def build_lut(seg_id, topk_idx, C, palette, color_by, n_ids):
    """seg_id, topk_idx int [B,Q]; palette uint8 [n,3]; color_by 0 (label) | 1 (segment id)
    -> int32 [B,n_ids]: r | g << 8 | b << 16, -1 where no slot names the id."""
    seg_id, topk_idx = np.asarray(seg_id), np.asarray(topk_idx)
    palette = np.asarray(palette, dtype=np.uint8).reshape(-1, 3)
    B, Q = seg_id.shape
    lut = np.full((B, n_ids), -1, dtype=np.int32)
    for b in range(B):
        for j in range(Q):  # slot order: of two slots naming one id the later decides
            s = int(seg_id[b, j])
            if not 0 <= s < n_ids:
                continue
            k = int(topk_idx[b, j]) % C if color_by == 0 else s
            r, g, bl = (int(v) for v in palette[k % len(palette)])
            lut[b, s] = r | (g << 8) | (bl << 16)
    return lut


def lut_from_colors(colors, ids, n_ids, default=(128, 128, 128)):
    """One image's table from an {id: (r, g, b)} mapping, for the ids listed (the reference's
    ``gt_color_mapping.get(segment_id, (128, 128, 128))`` per entry of segments_info)."""
    lut = np.full((n_ids,), -1, dtype=np.int32)
    for i in ids:
        if 0 <= int(i) < n_ids:
            r, g, b = (int(v) for v in colors.get(int(i), default))
            lut[int(i)] = r | (g << 8) | (b << 16)
    return lut


def blend(rgb, seg, lut, alpha):
    """rgb uint8 [B,H,W,3]; seg [B,H,W] float32 or int32; lut int32 [B,n_ids] -> uint8 [B,H,W,3]."""
    rgb, seg, lut = np.asarray(rgb), np.asarray(seg), np.asarray(lut)
    assert rgb.dtype == np.uint8 and lut.dtype == np.int32 and seg.dtype in (np.float32, np.int32)
    B, n_ids = lut.shape
    alpha = float(alpha)
    if seg.dtype == np.float32:
        with np.errstate(invalid="ignore"):
            ok = (seg >= 0) & (seg < np.float32(n_ids))
            ids = np.where(ok, seg, 0).astype(np.int64)
            ok &= ids.astype(np.float32) == seg  # the reference's ``map == id``: exact integers only
    else:
        ok = (seg >= 0) & (seg < n_ids)
        ids = np.where(ok, seg, 0).astype(np.int64)
    col = np.take_along_axis(lut, ids.reshape(B, -1), axis=1).reshape(seg.shape)
    paint = ok & (col >= 0)
    w0 = np.float32(1.0 - alpha)
    out = rgb.copy()
    for c in range(3):
        cc = ((col >> (8 * c)) & 0xFF).astype(np.float64)
        t = (alpha * cc).astype(np.float32)                       # float32(alpha * colour)
        prod = (w0 * rgb[..., c].astype(np.float32)).astype(np.float32)
        v = (prod + t).astype(np.float32)
        v = np.clip(v, np.float32(0), np.float32(255)).astype(np.uint8)
        out[..., c] = np.where(paint, v, rgb[..., c])
    return out
