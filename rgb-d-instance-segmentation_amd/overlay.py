"""f5: a prediction painted over its frame on the device (csrc/overlay.hip).

The reference's last step with a prediction is an alpha blend of every segment's colour over the
frame on the host (mask2former/predictor.py:295-330 ``_create_gt_overlay_with_consistent_colors``,
:1286-1320 ``_create_prediction_overlay``).  Here the map stays where post-processing left it:
``build_lut`` turns the arrays ``rgbd_pp_instance`` writes into a per-image colour table without a
host round trip (the form a captured stream uses, stream.StreamingSegmenter), ``blend`` paints,
and ``overlay_segments`` is the reference's call shape: HF-format results and an id -> colour
mapping in, a device uint8 image out, bit for bit the reference's arithmetic under NumPy 2.

f6 (csrc/segment_match.hip): the step of the reference's model-versus-ground-truth
picture that paints a prediction in the ground truth's colours (predictor.py:181-292
``_create_consistent_prediction_overlay``, :95-155 ``match_predictions_to_gt``).
``label_contingency`` counts every (prediction id, GT id) pair of pixels in one pass over the two
maps, ``greedy_iou_match`` matches by descending IoU, ``match_lut`` builds the colour table;
``match_segments`` and ``consistent_prediction_overlay`` are the reference's call shapes.
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


def _stack_maps(results):
    """The maps of HF-format results as one [B,H,W] tensor of float32 or int32 on the device."""
    maps = []
    for r in results:
        m = r["segmentation"]
        if not isinstance(m, torch.Tensor):
            raise TypeError("segmentation maps must be torch tensors on the device")
        _need_cuda(m)
        maps.append(m.to(torch.int32) if m.dtype == torch.int64 else m)
    if len({m.dtype for m in maps}) != 1:  # e.g. a panoptic batch with a "nothing kept" float32 map
        maps = [m.to(torch.float32) for m in maps]
    return maps[0][None] if len(maps) == 1 else torch.stack(maps)


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
    seg = _stack_maps(results)
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


MAX_MATCH_IDS = 256  # id ranges and list lengths of csrc/segment_match.hip


def _dtype_code(t, what):
    if t.dtype not in (torch.float32, torch.int32):
        raise ValueError(f"{what} must be float32 or int32 [B,H,W]")
    return RGBD_F32 if t.dtype == torch.float32 else RGBD_I32


def label_contingency(a, b, na, nb, out=None):
    """a, b: [B,H,W] float32 | int32 label maps on the device -> counts int32 [B,na+1,nb+1]: cell
    (i, j) = pixels naming id i in ``a`` and id j in ``b``; index na / nb collects the cells that
    name no id of the range (-1, NaN, fractions, ids past it).  Areas are the row and column sums."""
    _need_cuda(a, b, out)
    if a.dim() != 3 or a.shape != b.shape:
        raise ValueError("a and b must be [B,H,W] maps of one shape")
    ca, cb = _dtype_code(a, "a"), _dtype_code(b, "b")
    B, H, W = a.shape
    na, nb = int(na), int(nb)
    if out is None:
        out = torch.empty((B, na + 1, nb + 1), dtype=torch.int32, device=a.device)
    elif out.dtype != torch.int32 or tuple(out.shape) != (B, na + 1, nb + 1):
        raise ValueError("out must be int32 [B,na+1,nb+1]")
    check(_lib.lib().rgbd_label_contingency(_p(a), ca, _p(b), cb, B, H, W, na, nb, _p(out), _stream(a.device)),
          "rgbd_label_contingency")
    return out


def _match_args(counts, a_list, b_list):
    _need_cuda(counts, a_list, b_list)
    if counts.dtype != torch.int32 or counts.dim() != 3:
        raise ValueError("counts must be int32 [B,na+1,nb+1]")
    B = counts.shape[0]
    for t in (a_list, b_list):
        if t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] != B:
            raise ValueError("a_list and b_list must be int32 [B,L]")
    return B, counts.shape[1] - 1, counts.shape[2] - 1, a_list.shape[1], b_list.shape[1]


def greedy_iou_match(counts, a_list, b_list, hw, iou_threshold=0.5, out=None):
    """counts of ``label_contingency`` over maps of ``hw`` pixels; a_list int32 [B,La], b_list
    int32 [B,Lb]: segment ids in segments_info order, -1 padded.  -> (matched int32 [B,La],
    b_match_count int32 [B,Lb], n_filtered int32 [B,2]), indexed by position among the listed
    non-empty segments as the reference's arrays are (``out``: the same three, preallocated)."""
    B, na, nb, La, Lb = _match_args(counts, a_list, b_list)
    if out is None:
        dev = counts.device
        out = (torch.empty((B, La), dtype=torch.int32, device=dev), torch.empty((B, Lb), dtype=torch.int32, device=dev),
               torch.empty((B, 2), dtype=torch.int32, device=dev))
    matched, b_count, n_f = out
    _need_cuda(matched, b_count, n_f)
    check(_lib.lib().rgbd_greedy_iou_match(_p(counts), B, na, nb, int(hw), _p(a_list), La, _p(b_list), Lb,
                                           ctypes.c_double(float(iou_threshold)), _p(matched), _p(b_count), _p(n_f),
                                           _stream(counts.device)), "rgbd_greedy_iou_match")
    return matched, b_count, n_f


def _pack_rgb(c):
    r, g, b = (int(v) for v in c)
    if min(r, g, b) < 0 or max(r, g, b) > 255:
        raise ValueError(f"colour {tuple(c)}: (r, g, b) values in 0..255 expected")
    return r | (g << 8) | (b << 16)


def match_lut(counts, a_list, b_list, matched, n_filtered, gt_colors, unmatched_color=(255, 0, 0), out=None):
    """The table ``blend`` takes, as predictor.py:266-284 colours: a listed non-empty segment takes
    its matched GT id's entry of ``gt_colors`` (int32 [B,nb], packed, -1 = the mapping lacks the
    id), else ``unmatched_color``.  -> int32 [B,na]."""
    B, na, nb, La, Lb = _match_args(counts, a_list, b_list)
    _need_cuda(matched, n_filtered, gt_colors, out)
    if gt_colors.dtype != torch.int32 or tuple(gt_colors.shape) != (B, nb):
        raise ValueError("gt_colors must be int32 [B,nb]")
    if out is None:
        out = torch.empty((B, na), dtype=torch.int32, device=counts.device)
    check(_lib.lib().rgbd_match_lut(0, _p(counts), B, na, nb, _p(a_list), La, _p(b_list), Lb, _p(matched),
                                    _p(n_filtered), _p(gt_colors), _pack_rgb(unmatched_color), None, None, 0, _p(out),
                                    _stream(counts.device)), "rgbd_match_lut")
    return out


def track_lut(track, palette, out=None):
    """track int32 [B,Q] by segment id (-1 = none) -> int32 [B,Q]: palette[track % n_colors]."""
    _need_cuda(track, out)
    if track.dtype != torch.int32 or track.dim() != 2:
        raise ValueError("track must be int32 [B,Q]")
    pal = _palette(palette, track.device)
    B, Q = track.shape
    if out is None:
        out = torch.empty((B, Q), dtype=torch.int32, device=track.device)
    check(_lib.lib().rgbd_match_lut(1, None, B, Q, 0, None, 0, None, 0, None, None, None, 0, _p(track), _p(pal),
                                    pal.shape[0], _p(out), _stream(track.device)), "rgbd_match_lut")
    return out


def track_assign(counts, matched, prev_track, next_track, out=None):
    """After ``greedy_iou_match`` with a_list = b_list = 0..Q-1 on the counts of this frame's map
    against the previous frame's: -> track int32 [B,Q] by segment id.  A matched segment inherits
    ``prev_track`` of its match, every other non-empty one takes ``next_track[b]++`` in ascending
    id order (``next_track`` int32 [B] is updated in place), empty ids get -1."""
    _need_cuda(counts, matched, prev_track, next_track, out)
    B, Q = prev_track.shape
    if tuple(counts.shape) != (B, Q + 1, Q + 1) or tuple(matched.shape) != (B, Q) or tuple(next_track.shape) != (B,) \
            or any(t.dtype != torch.int32 for t in (counts, matched, prev_track, next_track)):
        raise ValueError("counts int32 [B,Q+1,Q+1], matched and prev_track int32 [B,Q], next_track int32 [B] expected")
    if out is None:
        out = torch.empty((B, Q), dtype=torch.int32, device=counts.device)
    check(_lib.lib().rgbd_track_assign(_p(counts), B, Q, _p(matched), _p(prev_track), _p(next_track), _p(out),
                                       _stream(counts.device)), "rgbd_track_assign")
    return out


def _id_lists(results, what):
    """segments_info ids per image -> (int32 [B,L] host array, -1 padded, L >= 1; the id range)."""
    rows = [[int(s["id"]) for s in r["segments_info"]] for r in results]
    for row in rows:
        if len(set(row)) != len(row):
            raise ValueError(f"{what}: duplicate ids in segments_info {row}")
        if any(i < 0 or i >= MAX_MATCH_IDS for i in row):
            raise ValueError(f"{what}: segment ids in 0..{MAX_MATCH_IDS - 1} expected, got {row}")
    L = max([len(row) for row in rows] + [1])
    arr = np.full((len(rows), L), -1, dtype=np.int32)
    for b, row in enumerate(rows):
        arr[b, :len(row)] = row
    return arr, max([i + 1 for row in rows for i in row], default=1)


def _match(prediction, gt_prediction, iou_threshold):
    single = isinstance(prediction, dict)
    preds = [prediction] if single else list(prediction)
    if gt_prediction is None:
        raise ValueError("gt_prediction is required: without a ground truth the reference falls back to random "
                         "colours, which this path does not draw")
    gts = [gt_prediction] if isinstance(gt_prediction, dict) else list(gt_prediction)
    if len(preds) != len(gts):
        raise ValueError("one ground-truth result per prediction expected")
    a_host, na = _id_lists(preds, "prediction")
    b_host, nb = _id_lists(gts, "gt_prediction")
    seg, gt = _stack_maps(preds), _stack_maps(gts)
    if seg.shape != gt.shape:
        raise ValueError(f"prediction maps {tuple(seg.shape)} and ground-truth maps {tuple(gt.shape)} differ in shape")
    dev = seg.device
    a_list, b_list = torch.from_numpy(a_host).to(dev), torch.from_numpy(b_host).to(dev)
    counts = label_contingency(seg, gt, na, nb)
    matched, b_count, n_f = greedy_iou_match(counts, a_list, b_list, seg.shape[1] * seg.shape[2], iou_threshold)
    return dict(segmentation=seg, counts=counts, a_list=a_list, b_list=b_list, matched=matched, b_match_count=b_count,
                n_filtered=n_f), single


def match_segments(prediction, gt_prediction, iou_threshold=0.5, return_tensors=False):
    """The device form of ``match_predictions_to_gt`` on the masks
    ``_create_consistent_prediction_overlay`` cuts: HF-format results (one, or a list of B), maps
    on the device.  -> per image the reference's ``(matched_gt_indices, is_matched,
    gt_match_counts)``, indexed by position among the listed non-empty segments; with
    ``return_tensors`` the device tensors instead (counts, a_list, b_list, matched, b_match_count,
    n_filtered), no host wait."""
    t, single = _match(prediction, gt_prediction, iou_threshold)
    if return_tensors:
        return t
    m, c, n = t["matched"].cpu().numpy(), t["b_match_count"].cpu().numpy(), t["n_filtered"].cpu().numpy()
    out = []
    for b in range(m.shape[0]):
        mi = [int(v) for v in m[b, :n[b, 0]]]
        out.append((mi, [v >= 0 for v in mi], [int(v) for v in c[b, :n[b, 1]]]))
    return out[0] if single else out


def consistent_prediction_overlay(image_u8, prediction, gt_color_mapping, gt_prediction, alpha=0.6, iou_threshold=0.5,
                                  unmatched_color=(255, 0, 0)):
    """The device form of ``_create_consistent_prediction_overlay``: every listed segment of the
    prediction matched to the ground truth by IoU and painted in its GT instance's colour,
    unmatched ones in ``unmatched_color``.  image_u8: uint8 [H,W,3] or [B,H,W,3] on the device;
    prediction, gt_prediction: HF-format results (one or B), maps on the device;
    gt_color_mapping: {gt id: (r, g, b)}, or one mapping per image.  -> uint8 image(s) on the
    device, bit for bit the reference's output under NumPy 2."""
    t, single = _match(prediction, gt_prediction, iou_threshold)
    img = image_u8[None] if image_u8.dim() == 3 else image_u8
    _need_cuda(img)
    B, nb = t["counts"].shape[0], t["counts"].shape[2] - 1
    if img.shape[0] != B:
        raise ValueError("one prediction per image expected")
    mappings = [gt_color_mapping] * B if isinstance(gt_color_mapping, dict) else list(gt_color_mapping)
    if len(mappings) != B:
        raise ValueError("one colour mapping, or one per image, expected")
    table = np.full((B, nb), -1, dtype=np.int32)
    for b, mp in enumerate(mappings):
        for i, c in mp.items():
            if 0 <= int(i) < nb:
                table[b, int(i)] = _pack_rgb(c)
    lut = match_lut(t["counts"], t["a_list"], t["b_list"], t["matched"], t["n_filtered"],
                    torch.from_numpy(table).to(img.device), unmatched_color)
    out = blend(img, t["segmentation"], lut, alpha)
    return out[0] if image_u8.dim() == 3 else out
