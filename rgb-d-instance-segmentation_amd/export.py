"""f4: COCO-RLE JSON export of instance predictions and ground-truth labels.

Reference: mask2former/predictor.py — ``convert_model_a_to_json_format`` (:335-372) over
``_convert_single_prediction_to_json`` (:376-457) for the post-processed predictions, and
``convert_gt_labels_to_json_format`` (:491-525) over ``_convert_single_gt_label_to_json``
(:528-625) for the labels; one ``<image name>.json`` per image:

    {"labels": [int], "scores": [float], "bboxes": [[x, y, w, h]], "masks": [{"size": [h, w],
     "counts": <pycocotools compressed RLE string>}]}

The reference builds every instance's binary mask on the host (``segmentation == id``), its
bounding box, and ``pycocotools.mask.encode`` of it.  Here the run boundaries and boxes of all
of an image's instances come from one pass on whatever device holds the map (the device
post-processing leaves the maps on the GPU with ``keep_on_device``): the stacked masks are read
column-major, run boundaries are the positions where a mask changes (one nonzero over all of
them), and one copy brings boundaries and boxes to the host, where the compressed string
(maskApi.c ``rleToString``) is formed from the counts.  pycocotools is not
installed here: the encoding is pinned against a step-for-step restatement of maskApi.c
(oracle/rle.py) and its decode round trip (tests/test_export.py).

``encode_segments`` / ``encode_segments_batch`` / ``encode_mask_stack`` are the same encoding as
hand-written HIP (csrc/rle_encode.hip): no [N, h, w] stack, no nonzero, no per-count
Python — one upload (the id table), one launch set, two host reads whatever N is (the per-mask
block, then exactly the characters), strings as slices of one bytes object.  With
``HIP_RLE_ENCODE`` the JSON builders below take that path for GPU-resident inputs whose ids lie in
[0, 256); the JSON is byte-identical either way.
"""
import ctypes
import json
import logging
import os
from pathlib import Path

import numpy as np
import torch

from . import _lib

log = logging.getLogger(__name__)

# prediction_to_json / gt_label_to_json (and the convert_* writers over them) on rgbd_rle_encode_*
# for GPU-resident inputs; False — or RGBD_HIP_RLE_ENCODE=0 — keeps the torch path below exactly
# (A/B runs; DESIGN §5.21 has the measurement behind the default)
HIP_RLE_ENCODE = os.environ.get("RGBD_HIP_RLE_ENCODE", "1") != "0"
MAX_IDS = 256  # overlay.MAX_MATCH_IDS: the id range of a label map on the device path
MAX_DEVICE_MASKS = 65535
_DEVICE_MAP_DTYPES = (torch.float32, torch.int32, torch.uint8, torch.int16)
NO_COUNTS, NO_CHARS = 1, 2  # the status bits of rgbd_rle_encode_*


def _to_string(counts) -> str:
    """maskApi.c rleToString (counts i > 2 delta-coded against count i - 2, 5-bit groups)."""
    out = []
    prev2 = prev1 = 0
    for i, cnt in enumerate(counts):
        x = cnt - prev2 if i > 2 else cnt
        prev2, prev1 = prev1, cnt
        while True:
            c = x & 0x1F
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            out.append(chr((c | 0x20 if more else c) + 48))
            if not more:
                break
    return "".join(out)


def encode_masks(masks: torch.Tensor):
    """masks bool/0-1 [N, h, w] (any device) -> list of (rle dict, bbox [x, y, w, h] or None), the
    pycocotools.mask.encode + _calculate_bbox_from_mask pair of the reference per mask.

    All N masks at once on their device: the column-major change positions of every mask come
    from one nonzero over the [N, h*w - 1] change map, the boxes from the row / column
    occupancy, and the whole result reaches the host in one copy (no per-mask sync)."""
    N, h, w = masks.shape
    if N == 0:
        return []
    L = h * w
    mb = masks.bool()
    cm = mb.transpose(1, 2).reshape(N, L)                      # column-major per mask
    pos = torch.nonzero(cm[:, 1:] != cm[:, :-1])              # [M, 2]: (mask, change index - 1)
    rows, cols = mb.any(dim=2), mb.any(dim=1)                 # [N, h], [N, w]
    ar_h = torch.arange(h, device=mb.device)
    ar_w = torch.arange(w, device=mb.device)
    big = max(h, w) + 1
    y0 = torch.where(rows, ar_h, big).amin(1)
    y1 = torch.where(rows, ar_h, -1).amax(1)
    x0 = torch.where(cols, ar_w, big).amin(1)
    x1 = torch.where(cols, ar_w, -1).amax(1)
    meta = torch.stack([cm[:, 0].long(), y0, y1, x0, x1], 1)  # [N, 5]
    flat = torch.cat([meta.reshape(-1), pos.reshape(-1).long()]).cpu().numpy()
    meta_h = flat[:5 * N].reshape(N, 5)
    pos_h = flat[5 * N:].reshape(-1, 2)
    starts = np.searchsorted(pos_h[:, 0], np.arange(N + 1), side="left")
    out = []
    for i in range(N):
        change = pos_h[starts[i]:starts[i + 1], 1] + 1
        bounds = np.concatenate([[0], change, [L]])
        counts = np.diff(bounds).tolist()
        if meta_h[i, 0]:
            counts = [0] + counts
        bbox = None
        if meta_h[i, 2] >= 0:
            yy0, yy1, xx0, xx1 = (int(v) for v in meta_h[i, 1:])
            bbox = [float(xx0), float(yy0), float(xx1 - xx0 + 1), float(yy1 - yy0 + 1)]
        out.append(({"size": [int(h), int(w)], "counts": _to_string(counts)}, bbox))
    return out


def _capacity(mode, n_images, n_masks, H, W, extra_masks=0):
    """(counts, chars) no call of this shape exceeds (rgbd_rle_encode_capacity); ``extra_masks``:
    slots that repeat an id of their image, each of which can add a whole mask's counts."""
    c, ch = ctypes.c_longlong(), ctypes.c_longlong()
    _lib.check(_lib.lib().rgbd_rle_encode_capacity(mode, n_images, n_masks, H, W, ctypes.byref(c), ctypes.byref(ch)),
               "rgbd_rle_encode_capacity")
    per = ch.value // max(c.value, 1)
    counts = c.value + extra_masks * (H * W + 1)
    return counts, counts * per


def _encode_device(mode, src, ids, n_images, n_masks, H, W, cap_counts, cap_chars):
    """One launch set and its two host reads -> (info int32 [N, 8], offsets [N+1], totals [2], the
    characters as bytes or None when a mask did not fit)."""
    from .ops import _p, _stream, _workspace
    L = _lib.lib()
    dev = src.device
    cap_chars = min(int(cap_chars), 2 ** 31 - 1)
    head = torch.empty((4 + n_masks + 1 + 8 * n_masks,), dtype=torch.int32, device=dev)  # totals | offsets | info
    totals, offsets, info = head[:4], head[4:5 + n_masks], head[5 + n_masks:]
    chars = torch.empty((max(cap_chars, 1),), dtype=torch.uint8, device=dev)
    ws = _workspace(dev, L.rgbd_rle_encode_workspace_size(mode, n_images, n_masks, H, W, cap_counts), "rle_encode")
    if mode == 0:
        dtype = _lib.RGBD_F32 if src.dtype == torch.float32 else _lib.RGBD_I32
        rc = L.rgbd_rle_encode_labels(dtype, _p(src), n_images, H, W, MAX_IDS, _p(ids), n_masks // n_images,
                                      cap_counts, cap_chars, _p(chars), _p(offsets), _p(info), _p(totals), _p(ws),
                                      _stream(dev))
        _lib.check(rc, "rgbd_rle_encode_labels")
    else:
        rc = L.rgbd_rle_encode_stack(_p(src), n_masks, H, W, cap_counts, cap_chars, _p(chars), _p(offsets), _p(info),
                                     _p(totals), _p(ws), _stream(dev))
        _lib.check(rc, "rgbd_rle_encode_stack")
    head_h = head.cpu().numpy()                                          # host read 1: the per-mask block
    totals_h = head_h[:4].view(np.int64)
    offsets_h, info_h = head_h[4:5 + n_masks], head_h[5 + n_masks:].reshape(n_masks, 8)
    if info_h[:, 7].any():
        return info_h, offsets_h, totals_h, None
    raw = chars[:int(offsets_h[-1])].cpu().numpy().tobytes()              # host read 2: exactly the characters
    return info_h, offsets_h, totals_h, raw


def _encode_with_retry(mode, src, ids, n_images, n_masks, H, W, cap_counts, cap_chars):
    info, offsets, totals, raw = _encode_device(mode, src, ids, n_images, n_masks, H, W, cap_counts, cap_chars)
    if raw is None:  # a capacity below the need: once more with the totals the kernels reported
        cap_counts = max(cap_counts, int(totals[0]))
        if not (info[:, 7] & NO_COUNTS).any():
            cap_chars = int(totals[1])
        info, offsets, totals, raw = _encode_device(mode, src, ids, n_images, n_masks, H, W, cap_counts, cap_chars)
        if raw is None:
            raise RuntimeError(f"rgbd_rle_encode: {int(totals[0])} counts / {int(totals[1])} characters do not fit "
                               f"{cap_counts} / {cap_chars}")
    text = raw.decode("ascii")
    out = []
    for m in range(n_masks):
        n, _, area, x0, y0, x1, y1, _ = (int(v) for v in info[m])
        bbox = [float(x0), float(y0), float(x1 - x0 + 1), float(y1 - y0 + 1)] if area > 0 else None
        out.append(({"size": [int(H), int(W)], "counts": text[offsets[m]:offsets[m + 1]]}, bbox, area))
    return out


def _device_map(seg):
    """The map as the kernels read it (float32 or int32, contiguous), or ValueError."""
    if not (isinstance(seg, torch.Tensor) and seg.is_cuda):
        raise RuntimeError("rgbd_amd ops run on the GPU only (no CPU fallback); got a CPU tensor")
    if seg.dtype not in _DEVICE_MAP_DTYPES:
        raise ValueError(f"label map dtype {seg.dtype}: one of {_DEVICE_MAP_DTYPES} expected")
    if seg.dtype in (torch.uint8, torch.int16):
        seg = seg.to(torch.int32)
    return seg.contiguous()


def encode_segments_batch(maps, ids_per_image, cap_chars=None):
    """maps: a device tensor [B, H, W] (or a list of B [H, W] maps of one size and dtype), float32 or
    an integer type up to int32; ids_per_image: B lists of segment ids in [0, 256).  -> per image a
    list of ``(rle dict, bbox [x, y, w, h] or None, area)``, one per id in order: mask j is
    ``map == ids[j]`` (a float cell names an id only when it holds that integer exactly), encoded
    as ``encode_masks`` encodes it.  rgbd_rle_encode_labels: one upload, one launch set, two host
    reads.  ``cap_chars``: the character capacity of the first attempt (default: the bound that
    cannot be exceeded); if it is too small the call is repeated once with the reported need."""
    if isinstance(maps, (list, tuple)):
        maps = torch.stack([_device_map(m) for m in maps]) if len(maps) else None
    if maps is None or maps.dim() != 3:
        raise ValueError("maps: [B, H, W] expected")
    maps = _device_map(maps)
    B, H, W = (int(v) for v in maps.shape)
    rows = [[int(i) for i in row] for row in ids_per_image]
    if len(rows) != B:
        raise ValueError(f"{len(rows)} id lists for {B} maps")
    for row in rows:
        if any(i < 0 or i >= MAX_IDS for i in row):
            raise ValueError(f"segment ids in 0..{MAX_IDS - 1} expected, got {row}")
    Q = max((len(r) for r in rows), default=0)
    if Q == 0:
        return [[] for _ in rows]
    table = np.full((B, Q), -1, np.int32)
    for b, row in enumerate(rows):
        table[b, :len(row)] = row
    ids = torch.from_numpy(table).to(maps.device)                        # the one upload
    dups = sum(len(r) - len(set(r)) for r in rows)
    cap_counts, bound_chars = _capacity(0, B, B * Q, H, W, dups)
    enc = _encode_with_retry(0, maps, ids, B, B * Q, H, W, cap_counts, bound_chars if cap_chars is None else cap_chars)
    return [enc[b * Q:b * Q + len(row)] for b, row in enumerate(rows)]


def encode_segments(segmentation, ids, cap_chars=None):
    """``encode_segments_batch`` for one device map [H, W] -> a list of (rle dict, bbox | None, area)."""
    return encode_segments_batch(segmentation[None], [ids], cap_chars=cap_chars)[0]


def encode_mask_stack(masks, cap_chars=None):
    """``encode_masks`` on rgbd_rle_encode_stack: masks bool / uint8 [N, h, w] on the device (set
    where non-zero) -> a list of (rle dict, bbox | None, area)."""
    if not (isinstance(masks, torch.Tensor) and masks.is_cuda):
        raise RuntimeError("rgbd_amd ops run on the GPU only (no CPU fallback); got a CPU tensor")
    if masks.dim() != 3 or masks.dtype not in (torch.bool, torch.uint8):
        raise ValueError("masks: bool or uint8 [N, h, w] expected")
    N, h, w = (int(v) for v in masks.shape)
    if N == 0:
        return []
    src = masks.contiguous().view(torch.uint8)
    cap_counts, bound_chars = _capacity(1, N, N, h, w)
    return _encode_with_retry(1, src, None, N, N, h, w, cap_counts, bound_chars if cap_chars is None else cap_chars)


def _on_device_path(t, n_masks, ids=None):
    return (HIP_RLE_ENCODE and isinstance(t, torch.Tensor) and t.is_cuda and 0 < n_masks <= MAX_DEVICE_MASKS
            and t.shape[-2] * t.shape[-1] < 2 ** 31
            and (ids is None or (t.dtype in _DEVICE_MAP_DTYPES and all(
                isinstance(i, int) and not isinstance(i, bool) and 0 <= i < MAX_IDS for i in ids))))


def prediction_to_json(prediction: dict, original_size=None) -> dict:
    """_convert_single_prediction_to_json (predictor.py:376-457): every segment of the
    post-processed map whose mask is non-empty, in segments_info order."""
    seg = prediction["segmentation"]
    seg = seg if isinstance(seg, torch.Tensor) else torch.as_tensor(np.asarray(seg))
    info = prediction["segments_info"]
    h, w = (int(original_size[0]), int(original_size[1])) if original_size is not None else tuple(seg.shape[:2])
    labels, scores, bboxes, masks = [], [], [], []
    if info:
        id_list = [s["id"] for s in info]
        if seg.dim() == 2 and _on_device_path(seg, len(id_list), id_list):
            enc = [e[:2] for e in encode_segments(seg, id_list)]
        else:
            ids = torch.tensor(id_list, dtype=seg.dtype, device=seg.device)
            enc = encode_masks(seg[None] == ids[:, None, None])
        for s, (rle, bbox) in zip(info, enc):
            if bbox is None:
                log.warning("instance id %s has an empty mask: skipped", s["id"])
                continue
            labels.append(int(s["label_id"]))
            scores.append(float(s.get("score", 1.0)))
            bboxes.append(bbox)
            masks.append({"size": [h, w], "counts": rle["counts"]})
    return {"labels": labels, "scores": scores, "bboxes": bboxes, "masks": masks}


def gt_label_to_json(label_info, original_size=None) -> dict:
    """_convert_single_gt_label_to_json (predictor.py:528-625): label_info = [masks, ids] with
    masks [N, h, w] (one per instance, > 0 = set) or an [h, w] instance-id map; ids <= 0 and
    empty masks are skipped; scores 1.0."""
    masks, ids = label_info
    masks = masks if isinstance(masks, torch.Tensor) else torch.as_tensor(np.asarray(masks))
    if masks.dim() not in (2, 3):
        raise ValueError(f"unsupported masks shape {tuple(masks.shape)}")
    h, w = (int(original_size[0]), int(original_size[1])) if original_size is not None else tuple(masks.shape[-2:])
    if masks.dim() == 3:
        ids_l = [int(i) for i in (np.asarray(ids).reshape(-1) if hasattr(ids, "__len__") else [ids] * masks.shape[0])]
        keep = [i for i in range(masks.shape[0]) if ids_l[i] > 0]
        sel = masks[keep] > 0 if keep else masks.new_zeros((0, *masks.shape[-2:]), dtype=torch.bool)
        lab = [ids_l[i] for i in keep]
        enc = ([e[:2] for e in encode_mask_stack(sel)] if _on_device_path(sel, len(lab))
               else encode_masks(sel) if len(lab) else [])
    else:
        u = torch.unique(masks)
        u = u[u > 0]
        lab = [int(x) for x in u.tolist()]
        if _on_device_path(masks, len(lab), lab):
            enc = [e[:2] for e in encode_segments(masks, lab)]
        else:
            enc = encode_masks(masks[None] == u[:, None, None]) if len(lab) else []
    labels, scores, bboxes, rles = [], [], [], []
    for lid, (rle, bbox) in zip(lab, enc):
        if bbox is None:
            continue
        labels.append(lid)
        scores.append(1.0)
        bboxes.append(bbox)
        rles.append({"size": [h, w], "counts": rle["counts"]})
    return {"labels": labels, "scores": scores, "bboxes": bboxes, "masks": rles}


def _write_all(items, names, save_dir, convert, sizes):
    path = Path(save_dir)
    path.mkdir(parents=True, exist_ok=True)
    written = []
    for i, (item, name) in enumerate(zip(items, names)):
        data = convert(item, sizes[i] if sizes else None)
        f = path / f"{name}.json"
        with open(f, "w") as fh:
            json.dump(data, fh, indent=2)
        written.append(f)
    return written


def convert_predictions_to_json(predicted_instance_maps, image_names, save_dir, original_sizes=None):
    """convert_model_a_to_json_format (predictor.py:335-372): one JSON file per image."""
    return _write_all(predicted_instance_maps, image_names, save_dir, prediction_to_json, original_sizes)


def convert_gt_labels_to_json(label_data, image_names, save_dir, original_sizes=None):
    """convert_gt_labels_to_json_format (predictor.py:491-525)."""
    return _write_all(label_data, image_names, save_dir, gt_label_to_json, original_sizes)
