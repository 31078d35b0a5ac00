"""Generate tests/golden/g12_json_import.npz by importing the REFERENCE's predictor itself.

Runs only where the reference checkout is present (not on the GPU box):
    python tests/golden/make_json_import_golden.py

The import shim is make_overlay_golden.import_predictor; pycocotools is absent, so its stubbed
``mask`` module gets a ``decode`` backed by oracle/rle.py (``rle_decode(h, w, rle_from_string(counts))``,
the step-for-step restatement of maskApi.c).  The case JSONs are written to a temporary directory
and read by ``_load_json_prediction_data`` (mask2former/predictor.py:974-1065) as files.  No file of
the reference is modified or copied; the fixture holds data only.

Load cases ``names``; per case k:
  l{k}_json, l{k}_shape      the JSON text and the image_shape passed
  l{k}_none                  whether the reference returned None
  l{k}_map, l{k}_ids, l{k}_labels, l{k}_scores   its map and segments_info (absent when None)
Comparison cases ``cmp_names``; per case k, on ``image`` with ``palette`` =
generate_consistent_colors(len(gt ids), seed=42):
  m{k}_gt, m{k}_models       the GT JSON text and the model JSON texts
  m{k}_gt_none, m{k}_model_none   which loads were None
  m{k}_gt_overlays           _create_gt_overlay_with_consistent_colors at alpha 0.6 and 0.37 (the
                             bare image where the GT is None)
  m{k}_model_overlays        [alpha][model] _create_consistent_prediction_overlay (the bare image
                             where the model's load, or the GT's, is None: with no GT the
                             reference draws random colours, which is not recorded)
"""
import json
import sys
import tempfile
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[2]
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

from make_overlay_golden import import_predictor  # noqa: E402
from oracle import rle  # noqa: E402

OUT = Path(__file__).resolve().parent / "g12_json_import.npz"
H, W = 24, 40
ALPHAS = [0.6, 0.37]


def _rect(h, w, y0, y1, x0, x1):
    m = np.zeros((h, w), np.uint8)
    m[y0:y1, x0:x1] = 1
    return m


def _file(masks, labels=None, scores=None, drop=None):
    d = {"labels": list(range(1, len(masks) + 1)) if labels is None else labels,
         "scores": [round(0.9 - 0.01 * i, 2) for i in range(len(masks))] if scores is None else scores,
         "bboxes": [rle.bbox_from_mask(m) or [0.0, 0.0, 0.0, 0.0] for m in masks],
         "masks": [rle.encode(m) for m in masks]}
    if drop:
        del d[drop]
    return d


def load_cases():
    rng = np.random.RandomState(12)
    a = _rect(H, W, 4, 10, 5, 15)
    b = _rect(H, W, 2, 14, 3, 20)           # covers a
    empty = np.zeros((H, W), np.uint8)
    blob = (rng.rand(H, W) < 0.4).astype(np.uint8)  # many short runs, set first pixel or not
    blob[0, 0] = 1
    out = [
        ("covered_empty_repeat", _file([a, b, empty, a]), (H, W)),
        ("overlap_order", _file([_rect(H, W, 0, 16, 0, 20), blob, _rect(H, W, 10, 24, 15, 40)]), (H, W)),
        ("later_upscaled", _file([a, _rect(12, 20, 6, 11, 8, 19)]), (H, W)),
        ("later_downscaled", _file([a, _rect(48, 80, 21, 47, 33, 79), (rng.rand(48, 80) < 0.5).astype(np.uint8)]),
         (H, W)),
        ("later_ragged", _file([b, (rng.rand(17, 29) < 0.3).astype(np.uint8), _rect(17, 29, 0, 5, 20, 29)]), (H, W)),
        ("downscale_vanishes", _file([a, _rect(48, 80, 0, 1, 0, 1), _rect(48, 80, 20, 21, 40, 41)]), (H, W)),
        ("first_small", _file([_rect(12, 20, 6, 11, 8, 19), a]), (H, W)),
        ("only_small", _file([_rect(12, 20, 6, 11, 8, 19)]), (H, W)),
        ("image_larger", _file([a, b]), (2 * H, 2 * W)),
        ("short_labels", _file([a, _rect(H, W, 12, 20, 22, 30), _rect(H, W, 0, 3, 30, 40)], labels=[7, 3]), (H, W)),
        ("short_scores", _file([a, _rect(H, W, 12, 20, 22, 30)], scores=[0.5]), (H, W)),
        ("empty_list", _file([]), (H, W)),
        ("only_empty", _file([empty]), (H, W)),
        ("missing_scores", _file([a], drop="scores"), (H, W)),
        ("many_255", _file([_rect(H, W, (i // 40) * 3, (i // 40) * 3 + 4, i % 40, i % 40 + 1) for i in range(255)],
                           labels=[i % 9 for i in range(255)]), (H, W)),
    ]
    return out


def cmp_cases():
    gt = _file([_rect(H, W, 1, 10, 1, 11), _rect(H, W, 1, 10, 14, 24), _rect(H, W, 13, 22, 1, 11),
                _rect(H, W, 13, 22, 27, 37)])
    good = _file([_rect(H, W, 2, 11, 1, 11), _rect(H, W, 1, 10, 15, 25), _rect(H, W, 0, 4, 30, 40),
                  _rect(H, W, 14, 22, 2, 11)])
    # Q19 through a file: mask 1 is listed but fully covered by mask 2, so its id is empty in the map
    covered = _file([_rect(H, W, 3, 8, 3, 9), _rect(H, W, 1, 10, 1, 11), _rect(H, W, 13, 22, 26, 37)])
    failed = _file([_rect(12, 20, 6, 11, 8, 19), _rect(H, W, 1, 10, 1, 11)])  # Q20: the load is None
    small = _file([_rect(H, W, 1, 10, 1, 11), _rect(12, 20, 6, 11, 13, 19)])  # a later mask upscaled
    return [
        ("three_models", gt, [good, covered, failed]),
        ("resized_model", gt, [small]),
        ("gt_none", _file([]), [good, failed]),
    ]


def main():
    ref = import_predictor()
    import pycocotools.mask as coco_mask
    coco_mask.decode = lambda r: rle.rle_decode(r["size"][0], r["size"][1], rle.rle_from_string(r["counts"]))
    import PIL
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(3), indexing="ij")
    image = ((x * 13 + c * 71 + (y % 4) * 59) % 256).astype(np.uint8)
    rec = dict(image=image, alphas=np.array(ALPHAS, np.float64), numpy_version=np.array(np.__version__),
               pillow_version=np.array(PIL.__version__))
    names = []
    with tempfile.TemporaryDirectory() as tmp:
        for k, (name, data, shape) in enumerate(load_cases()):
            names.append(name)
            text = json.dumps(data)
            path = Path(tmp) / f"l{k}.json"
            path.write_text(text)
            got = ref._load_json_prediction_data(str(path), tuple(shape))
            rec[f"l{k}_json"] = np.array(text)
            rec[f"l{k}_shape"] = np.array(shape, np.int32)
            rec[f"l{k}_none"] = np.array(got is None)
            if got is not None:
                info = got["segments_info"]
                rec[f"l{k}_map"] = got["segmentation"].astype(np.int32)
                rec[f"l{k}_ids"] = np.array([s["id"] for s in info], np.int32)
                rec[f"l{k}_labels"] = np.array([s["label_id"] for s in info], np.int32)
                rec[f"l{k}_scores"] = np.array([s["score"] for s in info], np.float64)
            print(f"{name}: " + ("None" if got is None else f"ids {[s['id'] for s in got['segments_info']]}"[:80]
                                 + f" map values {np.unique(got['segmentation'])[:8].tolist()}"))
        cmp_names = []
        for k, (name, gt_data, models) in enumerate(cmp_cases()):
            cmp_names.append(name)
            gpath = Path(tmp) / f"m{k}_gt.json"
            gpath.write_text(json.dumps(gt_data))
            gt = ref._load_json_prediction_data(str(gpath), (H, W))
            mapping = {}
            if gt is not None:
                ids = [s["id"] for s in gt["segments_info"]]
                state = np.random.get_state()
                mapping = dict(zip(ids, ref.generate_consistent_colors(len(ids), seed=42)))
                np.random.set_state(state)
            loaded = []
            for j, d in enumerate(models):
                p = Path(tmp) / f"m{k}_{j}.json"
                p.write_text(json.dumps(d))
                loaded.append(ref._load_json_prediction_data(str(p), (H, W)))
            gt_ov, model_ov = [], []
            for a in ALPHAS:
                gt_ov.append(image.copy() if gt is None else
                             ref._create_gt_overlay_with_consistent_colors(image, gt, mapping, a))
                model_ov.append([image.copy() if (m is None or gt is None) else
                                 ref._create_consistent_prediction_overlay(
                                     original_image=image, prediction=m, gt_color_mapping=mapping, gt_prediction=gt,
                                     alpha=a, iou_threshold=0.5) for m in loaded])
            rec[f"m{k}_gt"] = np.array(json.dumps(gt_data))
            rec[f"m{k}_models"] = np.array([json.dumps(d) for d in models])
            rec[f"m{k}_gt_none"] = np.array(gt is None)
            rec[f"m{k}_model_none"] = np.array([m is None for m in loaded])
            rec[f"m{k}_gt_overlays"] = np.stack(gt_ov).astype(np.uint8)
            rec[f"m{k}_model_overlays"] = np.array(model_ov).astype(np.uint8)
            print(f"{name}: gt {'None' if gt is None else 'loaded'}, models none {[m is None for m in loaded]}")
    rec["names"] = np.array(names)
    rec["cmp_names"] = np.array(cmp_names)
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes), numpy {np.__version__}, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
