"""Float64 restatement of Mask2FormerImageProcessor.post_process_panoptic_segmentation
(transformers 5.15 image_processing_pil_mask2former.py:788 with compute_segments :162,
check_segment_validity :143 and remove_low_and_no_objects :245) that exposes what the HF method
keeps to itself: the weighted probabilities, labels_px, the float64 top-2 gap per pixel and the
per-query area, orig and ratio.  tests/test_postprocess_dense_ref.py pins it against the HF method
fed float64 inputs (identical map, identical segments_info).

Also here: the fixtures of the dense post-processing tests (``blob_case``, ``CASES``) and the HF
float64 semantic reference (``semantic_ref``), shared by the CPU and the GPU tests.
"""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

S = 384  # HF's fixed intermediate size


def panoptic_ref(cl, ml, threshold=0.5, mask_threshold=0.5, overlap=0.8, fuse=None, target_size=None):
    """One image.  cl [Q, C + 1], ml [Q, h, w] (numpy or tensors, any float dtype)."""
    fuse = set() if fuse is None else fuse
    cl = torch.as_tensor(cl).double()
    ml = torch.as_tensor(ml).double()
    C = cl.shape[-1] - 1
    probs = F.interpolate(ml[None], size=(S, S), mode="bilinear", align_corners=False)[0].sigmoid()
    all_scores, all_labels = cl.softmax(-1).max(-1)  # the first maximum wins
    keep = all_labels.ne(C) & (all_scores > threshold)
    out = {"all_scores": all_scores, "all_labels": all_labels, "kept": keep.nonzero().flatten()}
    size = tuple(target_size) if target_size is not None else (S, S)
    if not bool(keep.any()):
        out.update(segmentation=torch.zeros(size) - 1, segments_info=[], P=None, labels_px=None, gap=None,
                   area=[], orig=[], ratio=[], valid=[])
        return out
    P = probs[keep]
    scores, labels = all_scores[keep], all_labels[keep]
    if target_size is not None:
        P = F.interpolate(P[None], size=size, mode="bilinear", align_corners=False)[0]
    P = P * scores.view(-1, 1, 1)  # the reference weighs in place: the mask threshold sees this P
    labels_px = P.argmax(0)
    if P.shape[0] > 1:
        top2 = P.topk(2, dim=0).values
        gap = top2[0] - top2[1]
    else:
        gap = torch.full(size, float("inf"), dtype=torch.float64)
    seg = torch.zeros(size, dtype=torch.int32)
    segments, area, orig, ratio, valid = [], [], [], [], []
    cur, memory = 0, {}
    for k in range(P.shape[0]):
        a = int((labels_px == k).sum())
        o = int((P[k] >= mask_threshold).sum())
        # torch divides the two int64 counts in float32; .item() is compared as a Python float
        r = float(np.float32(a) / np.float32(o)) if o > 0 else float("nan")
        ok = a > 0 and o > 0 and r > overlap
        area.append(a)
        orig.append(o)
        ratio.append(r)
        valid.append(ok)
        if not ok:
            continue
        lab = int(labels[k])
        cur = memory[lab] if lab in memory else cur + 1  # a remembered id replaces the running one
        seg[labels_px == k] = cur
        segments.append({"id": cur, "label_id": lab, "was_fused": lab in fuse, "score": round(float(scores[k]), 6)})
        if lab in fuse:
            memory[lab] = cur
    out.update(segmentation=seg, segments_info=segments, P=P, labels_px=labels_px, gap=gap, area=area, orig=orig,
               ratio=ratio, valid=valid, scores=scores, labels=labels)
    return out


def outputs_of(cl, ml, dtype=torch.float32):
    return types.SimpleNamespace(class_queries_logits=torch.as_tensor(cl).to(dtype),
                                 masks_queries_logits=torch.as_tensor(ml).to(dtype))


def hf_processor():
    from transformers.models.mask2former.image_processing_pil_mask2former import Mask2FormerImageProcessorPil
    return Mask2FormerImageProcessorPil()


def semantic_ref(cl, ml, target_sizes):
    """The HF method on float64 inputs: per image (map int64, scores float64 [C, Ht, Wt])."""
    res = hf_processor().post_process_semantic_segmentation(outputs_of(cl, ml, torch.float64),
                                                            target_sizes=target_sizes,
                                                            return_segmentation_scores=True)
    return [(r.segmentation, r.segmentation_scores) for r in res]


def top2_gap(scores):
    """[C, H, W] -> the gap between the largest and the second largest value per pixel."""
    if scores.shape[0] < 2:
        return torch.full(scores.shape[1:], float("inf"), dtype=scores.dtype)
    t = scores.topk(2, dim=0).values
    return t[0] - t[1]


# ------------------------------------------------------------------ fixtures
# query order of the roles; the queries after them alternate no-object and low-score
ROLES = ["background", "plain", "fused", "victim", "source", "fused", "plain2", "thief", "shadow", "noobject", "low"]


def blob_case(seed, Q, C, h, w, sigma=0.17):
    """One image of Gaussian-blob mask logits 14 exp(-r^2 / 2 sigma^2) - 6 + 0.3 noise:

    background  constant logit +0.2: wins wherever no blob does (accepted, unfused)
    plain/plain2, source   blobs of their own (accepted)
    fused (twice)          two blobs with the one label that is in the fuse set: one id
    victim / thief         the thief copies the victim's logits on one side of its centre (-6
                           elsewhere) with a higher class score: the victim keeps about half of its
                           area and is rejected with 0 < ratio < threshold
    shadow                 the source's logits with a lower class score: area 0
    noobject, low          removed as no-object / by score (all remaining queries alternate)

    Returns cl [Q, C + 1], ml [Q, h, w] float32, the fuse set and the role of every query."""
    assert Q >= len(ROLES) - 2 and C >= 5
    rng = np.random.default_rng(seed)
    roles = (ROLES + ["noobject", "low"] * Q)[:Q]
    gy, gx = (2, 3) if h < w else (3, 2)
    cells = [(i, j) for i in range(gy) for j in range(gx)]
    ch, cw = h / gy, w / gx
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ml = np.empty((Q, h, w))
    cl = 0.5 * rng.standard_normal((Q, C + 1))
    # labels: spread over the class range so that ids above 128 occur when C allows
    lab = {"background": 0, "plain": C // 4, "fused": C - 1, "victim": C // 2, "source": C // 2 + 1,
           "plain2": C // 4, "thief": C // 2 + 1, "shadow": C // 2}
    boost = {"background": 8.0, "plain": 7.0, "fused": 9.0, "victim": 5.0, "source": 8.0, "plain2": 6.0,
             "thief": 10.0, "shadow": 5.5, "noobject": 7.0}
    more = np.log(C / 5)  # the same scores at any class count
    blob_roles = ["plain", "fused", "victim", "source", "fused", "plain2"]
    centres, logits = {}, {}
    n_blob = 0
    for q, role in enumerate(roles):
        if role in blob_roles and n_blob < len(cells):
            i, j = cells[n_blob]
            n_blob += 1
            cy = (i + 0.5) * ch - 0.5 + rng.uniform(-0.4, 0.4)
            cx = (j + 0.5) * cw - 0.5 + rng.uniform(-0.4, 0.4)
            sg = sigma * min(ch, cw) * rng.uniform(0.9, 1.1)
            ml[q] = 14 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sg * sg)) - 6 + 0.3 * rng.standard_normal((h, w))
            centres[role], logits[role] = (cy, cx), ml[q]
        elif role == "background":
            ml[q] = 0.2
        elif role == "thief":
            ml[q] = np.where(xx < centres["victim"][1], logits["victim"], -6.0)
        elif role == "shadow":
            ml[q] = logits["source"]
        else:  # small stray blobs: they count in the semantic scores only
            cy, cx = rng.uniform(0, h), rng.uniform(0, w)
            ml[q] = 6 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 2.0) - 6 + 0.3 * rng.standard_normal((h, w))
        if role != "low":
            cl[q, C if role == "noobject" else lab[role]] += boost[role] + more
    cl = cl.astype(np.float32)
    # round(score, 6) must not depend on the precision of the run: nudge the boosted logit until
    # score * 1e6 is 0.2 away from a rounding boundary (a float32 softmax maximum is within about
    # 1.5 * 2^-24 = 0.09e-6 of the exact one: the largest term is exp(0) = 1, the sum and the
    # division round once each)
    for q, role in enumerate(roles):
        while role not in ("low", "noobject"):
            e = np.exp(cl[q].astype(np.float64) - cl[q].max())
            if abs((e.max() / e.sum() * 1e6) % 1.0 - 0.5) >= 0.2:
                break
            cl[q, lab[role]] += np.float32(1e-3)
    return cl, ml.astype(np.float32), {C - 1}, roles


# (name, B, Q, C, h, w, seeds, list of target_sizes arguments)
CASES = [
    ("ragged", 2, 11, 5, 12, 20, (7, 8), [None, [(37, 53), (384, 384)], [(480, 640), (97, 131)]]),
    ("workload", 2, 100, 48, 24, 32, (5, 7), [[(96, 128), (61, 45)]]),
    ("manyclass", 1, 33, 134, 17, 9, (6,), [[(50, 70)]]),
]
CASE_IDS = [f"{c[0]}-{i}" for c in CASES for i in range(len(c[7]))]
CASE_PARAMS = [(c[0], i) for c in CASES for i in range(len(c[7]))]


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """cl [B, Q, C + 1], ml [B, Q, h, w], the fuse set, the roles per image."""
    _, B, Q, C, h, w, seeds, _ = next(c for c in CASES if c[0] == name)
    parts = [blob_case(s, Q, C, h, w) for s in seeds]
    assert len(parts) == B
    return (np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), parts[0][2], [p[3] for p in parts])


def case_targets(name, i):
    return next(c for c in CASES if c[0] == name)[7][i]


@functools.lru_cache(maxsize=None)
def case_panoptic_ref(name, i):
    """The float64 panoptic reference of every image of a case; computed once, never modified."""
    cl, ml, fuse, _ = case_inputs(name)
    ts = case_targets(name, i)
    return [panoptic_ref(cl[b], ml[b], fuse=fuse, target_size=None if ts is None else ts[b])
            for b in range(cl.shape[0])]


@functools.lru_cache(maxsize=None)
def case_semantic_ref(name, i):
    cl, ml, _, _ = case_inputs(name)
    return semantic_ref(cl, ml, case_targets(name, i))


# The error bars of the issue: scores within SEM_BAR * max(1, max|S64|); maps equal wherever the
# float64 top-2 gap is at least twice the bar; at most BAND_CAP of an image inside the band.
SEM_BAR = 2e-5
PAN_BAR = 2e-6
BAND_CAP = 0.01
