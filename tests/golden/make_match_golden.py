"""Generate tests/golden/g11_match.npz by importing the REFERENCE's predictor itself.

Runs only where the reference checkout is present (not on the GPU box):
    python tests/golden/make_match_golden.py

The import shim is make_overlay_golden.import_predictor (absent cv2 / pycocotools / matplotlib /
tqdm replaced by empty modules; none is touched by the functions recorded here).  No file of the
reference is modified or copied; the fixture holds data only.  Per case k, on 24x40 maps:

  c{k}_pred, c{k}_gt          float32 maps, -1 = none
  c{k}_pred_ids, c{k}_gt_ids  the ids of the two segments_info lists, in list order
  c{k}_color_ids, c{k}_color_rgb   the GT id -> colour mapping
  c{k}_thr                    iou_threshold
  c{k}_matched, c{k}_is_matched, c{k}_gt_counts   match_predictions_to_gt on the non-empty masks,
                              cut as _create_consistent_prediction_overlay cuts them
  c{k}_overlays               _create_consistent_prediction_overlay at alpha 0.6 and 0.37

Cases: plain; ties (two pairs of IoU 2/6 = 3/9 competing for one GT segment, listed so that list
position and id disagree, and two pairs 2/6 = 3/9 competing for one prediction); an IoU equal to
the threshold (2/4 against 0.5); an empty listed segment before a matched one (the reference then
reads the filtered match arrays with the unfiltered position); a matched GT id missing
from the colour mapping; no GT segments; no prediction segments.
"""
from pathlib import Path

import numpy as np

from make_overlay_golden import import_predictor

OUT = Path(__file__).resolve().parent / "g11_match.npz"
H, W = 24, 40
ALPHAS = [0.6, 0.37]


def _blank():
    return np.full((H, W), -1, np.float32)


def _blocks(rng, n, jitter):
    """n rectangular segments on a 2 x 3 grid of cells, each moved by up to ``jitter`` pixels."""
    m = _blank()
    for k in range(n):
        r, c = divmod(k, 3)
        dy, dx = rng.randint(-jitter, jitter + 1, size=2) if jitter else (0, 0)
        y0, x0 = 1 + 12 * r + dy, 1 + 13 * c + dx
        m[max(y0, 0):y0 + 9, max(x0, 0):x0 + 10] = k
    return m


def cases():
    rng = np.random.RandomState(11)
    out = []
    # plain: six GT blocks, five jittered predictions (one far off: unmatched) and a spurious one
    gt = _blocks(rng, 6, 0)
    pred = _blocks(rng, 5, 2)
    pred[pred == 4] = -1
    pred[20:24, 30:40] = 4          # prediction 4 sits mostly outside GT 4
    pred[0:2, 36:40] = 9            # a false positive
    colors = {i: tuple(int(v) for v in rng.randint(0, 256, 3)) for i in range(6)}
    out.append(("plain", pred, [0, 1, 2, 3, 4, 9], gt, [0, 1, 2, 3, 4, 5], colors, 0.5))
    # ties.  GT 0: 5 px, 2 in prediction 3 (3 px) and 3 in prediction 1 (7 px): IoU 2/6 and 3/9, and
    # prediction 3 is listed first.  Prediction 2: 5 px, 2 in GT 5 (3 px), 3 in GT 4 (7 px): 2/6, 3/9.
    gt, pred = _blank(), _blank()
    gt[2, 2:7] = 0
    pred[2, 2:4] = 3
    pred[3, 2] = 3
    pred[2, 4:7] = 1
    pred[3, 4:8] = 1
    pred[10, 10:15] = 2
    gt[10, 10:12] = 5
    gt[11, 10] = 5
    gt[10, 12:15] = 4
    gt[11, 12:16] = 4
    colors = {0: (10, 200, 30), 4: (1, 2, 250), 5: (250, 240, 3)}
    out.append(("ties", pred, [3, 1, 2], gt, [5, 4, 0], colors, 0.3))
    # IoU == threshold: 3 px against 3 px sharing 2: 2/4 >= 0.5; and 1/3 next to it, below
    gt, pred = _blank(), _blank()
    gt[5, 5:8] = 1
    pred[5, 6:9] = 0
    gt[15, 5:7] = 2
    pred[15, 6:8] = 1
    out.append(("threshold", pred, [0, 1], gt, [1, 2], {1: (0, 255, 0), 2: (0, 0, 255)}, 0.5))
    # the quirk: id 7 is listed and empty, id 1 matches nothing, id 2 matches GT 3
    gt, pred = _blank(), _blank()
    pred[1:6, 1:9] = 1
    gt[8:20, 10:30] = 3
    pred[8:20, 11:31] = 2
    out.append(("empty_before_matched", pred, [7, 1, 2], gt, [3], {3: (20, 220, 120)}, 0.5))
    # the matched GT id 2 has no colour
    gt = _blocks(rng, 3, 0)
    pred = _blocks(rng, 3, 1)
    out.append(("color_missing", pred, [0, 1, 2], gt, [0, 1, 2], {0: (200, 100, 0), 1: (0, 100, 200)}, 0.5))
    # no GT segments listed (the map still holds some), and a GT list of empty segments only
    out.append(("no_gt", _blocks(rng, 4, 1), [0, 1, 2, 3], _blocks(rng, 2, 0), [], {0: (1, 2, 3)}, 0.5))
    out.append(("gt_all_empty", _blocks(rng, 4, 1), [0, 1, 2, 3], _blank(), [0, 1], {0: (1, 2, 3)}, 0.5))
    # no prediction segments
    out.append(("no_pred", _blank(), [], _blocks(rng, 3, 0), [0, 1, 2], {0: (1, 2, 3)}, 0.5))
    return out


def main():
    ref = import_predictor()
    # rows repeat every four, so the fixture stays a few KB; G10 holds the random image
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(3), indexing="ij")
    image = ((x * 13 + c * 71 + (y % 4) * 59) % 256).astype(np.uint8)
    rec = dict(image=image, alphas=np.array(ALPHAS, np.float64), numpy_version=np.array(np.__version__))
    names = []
    for k, (name, pred, pred_ids, gt, gt_ids, colors, thr) in enumerate(cases()):
        names.append(name)
        prediction = {"segmentation": pred, "segments_info": [{"id": i, "label_id": 0, "score": 1.0} for i in pred_ids]}
        gt_prediction = {"segmentation": gt, "segments_info": [{"id": i, "label_id": 0} for i in gt_ids]}
        pm = [pred == i for i in pred_ids if (pred == i).sum() > 0]
        gm = [gt == i for i in gt_ids if (gt == i).sum() > 0]
        matched, is_matched, gt_counts = ref.match_predictions_to_gt(pm, [0] * len(pm), [1.0] * len(pm), gm,
                                                                     [0] * len(gm), thr)
        outs = [ref._create_consistent_prediction_overlay(image, prediction, colors, gt_prediction, alpha=a,
                                                          iou_threshold=thr) for a in ALPHAS]
        cid = sorted(colors)
        rec.update({
            f"c{k}_pred": pred, f"c{k}_gt": gt, f"c{k}_pred_ids": np.array(pred_ids, np.int32),
            f"c{k}_gt_ids": np.array(gt_ids, np.int32), f"c{k}_color_ids": np.array(cid, np.int32),
            f"c{k}_color_rgb": np.array([colors[i] for i in cid], np.uint8).reshape(-1, 3),
            f"c{k}_thr": np.array(thr, np.float64), f"c{k}_matched": np.array(matched, np.int32),
            f"c{k}_is_matched": np.array(is_matched, np.bool_), f"c{k}_gt_counts": np.array(gt_counts, np.int32),
            f"c{k}_overlays": np.stack(outs).astype(np.uint8)})
        print(f"{name}: matched {matched} gt_counts {gt_counts}")
    rec["names"] = np.array(names)
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes), numpy {np.__version__}")


if __name__ == "__main__":
    main()
