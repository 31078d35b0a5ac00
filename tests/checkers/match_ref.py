"""Numpy restatement of the segment matcher (csrc/segment_match.hip): contingency table, greedy
IoU matching, the colour tables and the track assignment, with every cast spelled out.

The reference (mask2former/predictor.py:95-155 match_predictions_to_gt, :181-292
_create_consistent_prediction_overlay) works on per-segment boolean masks; the masks of one map
are disjoint, so its intersections are cells of the contingency table of the two maps and its
mask areas are row and column sums.  ``greedy_match`` keeps the reference's own formulation —
candidates in (i, j) order, a stable descending sort, one sweep — rather than the kernel's
repeated arg-max, so the two are independent statements of one result
(tests/test_match_ref.py pins this file to the reference's recorded output, G11).
"""
import numpy as np

from checkers import overlay_ref


def cell_ids(m, n):
    """The id every cell names, ``n`` for none: float32 cells name an id only when they hold that
    integer exactly (the reference's ``map == id``)."""
    m = np.asarray(m)
    assert m.dtype in (np.float32, np.int32)
    if m.dtype == np.float32:
        with np.errstate(invalid="ignore"):
            ok = (m >= np.float32(0)) & (m < np.float32(n))
            ids = np.where(ok, m, np.float32(0)).astype(np.int64)
            ok &= ids.astype(np.float32) == m
    else:
        ok = (m >= 0) & (m < n)
        ids = np.where(ok, m, 0).astype(np.int64)
    return np.where(ok, ids, np.int64(n))


def contingency(a, b, na, nb):
    """a, b [B,H,W] float32 | int32 -> int32 [B,na+1,nb+1]; index na / nb = "none"."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.ndim == 3
    B = a.shape[0]
    out = np.zeros((B, na + 1, nb + 1), np.int32)
    for i in range(B):
        key = cell_ids(a[i], na).reshape(-1) * np.int64(nb + 1) + cell_ids(b[i], nb).reshape(-1)
        out[i] = np.bincount(key, minlength=(na + 1) * (nb + 1)).astype(np.int32).reshape(na + 1, nb + 1)
    return out


def filtered(ids, area):
    """The listed ids whose segment is not empty, in list order (-1 padding and ids outside the
    table name no segment)."""
    return [int(i) for i in ids if 0 <= int(i) < len(area) and int(area[int(i)]) > 0]


def greedy_match(counts, a_list, b_list, iou_threshold):
    """counts int32 [B,na+1,nb+1]; a_list [B,La], b_list [B,Lb] int, -1 padded -> (matched int32
    [B,La], b_match_count int32 [B,Lb], n_filtered int32 [B,2]), indexed by filtered position."""
    counts = np.asarray(counts)
    a_list, b_list = np.asarray(a_list), np.asarray(b_list)
    B, La, Lb = counts.shape[0], a_list.shape[1], b_list.shape[1]
    na, nb = counts.shape[1] - 1, counts.shape[2] - 1
    matched = np.full((B, La), -1, np.int32)
    b_count = np.zeros((B, Lb), np.int32)
    n_f = np.zeros((B, 2), np.int32)
    thr = float(iou_threshold)
    for b in range(B):
        tab = counts[b].astype(np.int64)
        area_a, area_b = tab.sum(axis=1)[:na], tab.sum(axis=0)[:nb]
        fa, fb = filtered(a_list[b], area_a), filtered(b_list[b], area_b)
        n_f[b] = len(fa), len(fb)
        cand = []
        for i, ia in enumerate(fa):
            for j, ib in enumerate(fb):
                inter = np.int64(tab[ia, ib])
                union = np.int64(area_a[ia]) + np.int64(area_b[ib]) - inter
                iou = np.float64(inter) / np.float64(union) if union > 0 else np.float64(0.0)
                if iou >= thr:
                    cand.append((i, j, float(iou)))
        cand.sort(key=lambda x: x[2], reverse=True)  # stable: equal IoUs keep (i, j) order
        used = set()
        for i, j, _ in cand:
            if matched[b, i] < 0 and j not in used:
                matched[b, i] = j
                b_count[b, j] += 1
                used.add(j)
    return matched, b_count, n_f


def pack(rgb):
    r, g, b = (int(v) for v in rgb)
    return r | (g << 8) | (b << 16)


def gt_color_table(mappings, nb):
    """Per image ``{gt id: (r, g, b)}`` -> int32 [B,nb], -1 where the mapping lacks the id."""
    out = np.full((len(mappings), nb), -1, np.int32)
    for b, m in enumerate(mappings):
        for i, c in m.items():
            if 0 <= int(i) < nb:
                out[b, int(i)] = pack(c)
    return out


def gt_lut(counts, a_list, b_list, matched, n_filtered, gt_colors, unmatched):
    """predictor.py:266-284 -> int32 [B,na].  The i-th LISTED non-empty segment reads entry i of
    the FILTERED arrays when i is below their length (the reference's indexing)."""
    counts, a_list, b_list = np.asarray(counts), np.asarray(a_list), np.asarray(b_list)
    B, na, nb = counts.shape[0], counts.shape[1] - 1, counts.shape[2] - 1
    lut = np.full((B, na), -1, np.int32)
    for b in range(B):
        tab = counts[b].astype(np.int64)
        area_a, area_b = tab.sum(axis=1)[:na], tab.sum(axis=0)[:nb]
        fb = filtered(b_list[b], area_b)
        for i, sid in enumerate(int(v) for v in a_list[b]):
            if not (0 <= sid < na and area_a[sid] > 0):
                continue
            col = int(unmatched)
            if i < int(n_filtered[b, 0]) and matched[b, i] >= 0 and matched[b, i] < len(fb):
                c = int(gt_colors[b, fb[int(matched[b, i])]])
                if c >= 0:
                    col = c
            lut[b, sid] = col
    return lut


def track_assign(counts, matched, prev_track, next_track):
    """After greedy_match with a_list = b_list = 0..Q-1 -> (track int32 [B,Q] by segment id, the
    updated next_track int32 [B])."""
    counts = np.asarray(counts)
    B, Q = counts.shape[0], counts.shape[1] - 1
    track = np.full((B, Q), -1, np.int32)
    nxt = np.array(next_track, np.int32).copy()
    for b in range(B):
        tab = counts[b].astype(np.int64)
        area_a, area_b = tab.sum(axis=1)[:Q], tab.sum(axis=0)[:Q]
        fb = [j for j in range(Q) if area_b[j] > 0]
        pos = 0
        for sid in range(Q):
            if area_a[sid] <= 0:
                continue
            m = int(matched[b, pos])
            pos += 1
            t = int(prev_track[b, fb[m]]) if 0 <= m < len(fb) else -1
            if t < 0:
                t = int(nxt[b])
                nxt[b] += 1
            track[b, sid] = t
    return track, nxt


def track_lut(track, palette):
    """int32 [B,Q]: palette[track % n_colors] packed, -1 where the id has no track."""
    track = np.asarray(track)
    palette = np.asarray(palette, np.uint8).reshape(-1, 3)
    lut = np.full(track.shape, -1, np.int32)
    for idx in np.ndindex(*track.shape):
        if track[idx] >= 0:
            lut[idx] = pack(palette[int(track[idx]) % len(palette)])
    return lut


def track_step(seg, prev_seg, prev_track, next_track, Q, iou_threshold):
    """One frame of the stream's tracking stage -> (track, next_track)."""
    ids = np.tile(np.arange(Q, dtype=np.int32), (seg.shape[0], 1))
    counts = contingency(seg, prev_seg, Q, Q)
    matched, _, _ = greedy_match(counts, ids, ids, iou_threshold)
    return track_assign(counts, matched, prev_track, next_track)


def match_triple(matched, b_count, n_filtered):
    """One image's rows -> the reference's (matched_gt_indices, is_matched, gt_match_counts)."""
    pa, pb = int(n_filtered[0]), int(n_filtered[1])
    m = [int(v) for v in matched[:pa]]
    return m, [v >= 0 for v in m], [int(v) for v in b_count[:pb]]


def consistent_overlay(image, pred, pred_ids, gt, gt_ids, colors, alpha, iou_threshold, unmatched=(255, 0, 0)):
    """_create_consistent_prediction_overlay for one image -> (uint8 [H,W,3], the match triple)."""
    ids = [int(i) for i in pred_ids] + [int(i) for i in gt_ids]
    na = max([i + 1 for i in pred_ids], default=1)
    nb = max([i + 1 for i in gt_ids], default=1)
    assert all(i >= 0 for i in ids)
    a_list = np.array([list(pred_ids) or [-1]], np.int32)
    b_list = np.array([list(gt_ids) or [-1]], np.int32)
    counts = contingency(pred[None], gt[None], na, nb)
    matched, b_count, n_f = greedy_match(counts, a_list, b_list, iou_threshold)
    lut = gt_lut(counts, a_list, b_list, matched, n_f, gt_color_table([colors], nb), pack(unmatched))
    return overlay_ref.blend(image[None], pred[None], lut, alpha)[0], match_triple(matched[0], b_count[0], n_f[0])
