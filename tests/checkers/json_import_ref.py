"""Numpy restatement of the JSON import (csrc/rle_decode.hip, rgbd_amd/json_results.py): the string
decode, the mask decode, the PIL NEAREST resize, the composite with its filters, and the
multi-model comparison on top of the overlay and matcher checkers.

Vectorised where the oracle (oracle/rle.py, plain loops over maskApi.c) is not, so the two are
independent statements: ``counts_from_string`` decodes all groups of a string at once and undoes
the delta coding by the two stride-2 cumulative sums the kernel uses; ``decode`` places the run
ends and takes the parity of a searchsorted.  tests/test_json_import_ref.py pins this file to the
reference's recorded output, G12 (tests/golden/make_json_import_golden.py).
"""
import json

import numpy as np

from checkers import match_ref, overlay_ref
from oracle.resize import pil_nearest

BAD_COUNT, BAD_TOTAL, BAD_GROUP = 1, 2, 4


def counts_from_string(s):
    """maskApi.c rleFrString -> (int64 counts, truncated?)."""
    c = np.frombuffer(s.encode("ascii"), np.uint8).astype(np.int64) - 48
    if c.size == 0:
        return np.zeros(0, np.int64), False
    term = (c & 0x20) == 0
    truncated = not bool(term[-1])
    idx = np.cumsum(term) - term                      # count index of every character
    first = np.concatenate([[0], np.nonzero(term)[0][:-1] + 1]) if term.any() else np.zeros(0, np.int64)
    n = int(term.sum())
    pos = np.arange(c.size)
    keep = idx < n                                     # characters of a truncated last group are dropped
    g = pos[keep] - first[idx[keep]]                   # group number within its count
    x = np.zeros(n, np.int64)
    np.add.at(x, idx[keep], (c[keep] & 0x1F) << (5 * g))
    last = np.nonzero(term)[0]
    ng = last - first + 1
    neg = (c[last] & 0x10) != 0
    x = np.where(neg, x | (np.int64(-1) << (5 * ng)), x)
    cnts = x.copy()
    if n > 3:
        odd = np.arange(1, n, 2)
        even = np.arange(2, n, 2)
        cnts[odd] = np.cumsum(x[odd])
        cnts[even] = np.cumsum(x[even])
    return cnts, truncated


def status_of(cnts, truncated, h, w):
    st = 0
    if (cnts < 0).any():
        st |= BAD_COUNT
    if int(cnts.sum()) != h * w:
        st |= BAD_TOTAL
    if truncated:
        st |= BAD_GROUP
    return st


def decode(h, w, cnts):
    """maskApi.c rleDecode -> bool [h, w]: position p (column-major) lies in the run whose end is
    the first one above p; odd runs are set."""
    ends = np.cumsum(cnts)
    run = np.searchsorted(ends, np.arange(h * w), side="right")
    return (run & 1).astype(bool).reshape(w, h).T


def decode_rle(rle):
    h, w = (int(v) for v in rle["size"])
    cnts, trunc = counts_from_string(rle["counts"])
    assert status_of(cnts, trunc, h, w) == 0, "malformed RLE"
    return decode(h, w, cnts)


def load_prediction(data, image_shape):
    """_load_json_prediction_data (predictor.py:974-1065) for a parsed dict -> None or
    (int32 map [H, W], ids, labels, scores)."""
    image_shape = tuple(int(v) for v in image_shape)
    if not all(k in data for k in ("masks", "labels", "scores")):
        return None
    masks, labels, scores = data["masks"], data["labels"], data["scores"]
    if not masks:
        return None
    seg = np.zeros(tuple(masks[0]["size"]), np.int32)
    ids = []
    for i, rle in enumerate(masks):
        if i >= len(labels) or i >= len(scores):
            continue
        m = decode_rle(rle)
        if m.shape != image_shape:
            m = pil_nearest(m.astype(np.uint8) * 255, *image_shape) > 0
        if m.sum() > 0:
            if m.shape != seg.shape:  # Q20: the reference's boolean index raises and the mask is skipped
                continue
            seg[m] = i + 1
            ids.append(i + 1)
    if not ids:
        return None
    return seg, ids, [labels[i - 1] for i in ids], [scores[i - 1] for i in ids]


def comparison(image, gt_data, model_datas, alpha, iou_threshold, palette):
    """Steps 2-5 of _create_and_save_multi_model_json_comparison; ``palette``: the colours
    generate_consistent_colors gives (at least as many as GT ids).  A model whose load is None,
    and every model when the GT is None, keeps the bare image."""
    H, W = image.shape[:2]
    gt = load_prediction(gt_data, (H, W))
    outs = []
    if gt is None:
        return image.copy(), [image.copy() for _ in model_datas]
    mapping = dict(zip(gt[1], [tuple(int(v) for v in c) for c in palette]))
    lut = overlay_ref.lut_from_colors(mapping, gt[1], max(gt[1]) + 1)
    gt_overlay = overlay_ref.blend(image[None], gt[0][None], lut[None], alpha)[0]
    for d in model_datas:
        m = load_prediction(d, (H, W))
        if m is None:
            outs.append(image.copy())
        else:
            outs.append(match_ref.consistent_overlay(image, m[0], m[1], gt[0], gt[1], mapping, alpha,
                                                     iou_threshold)[0])
    return gt_overlay, outs


def case_json(g, name):
    return json.loads(str(g[name]))
