"""The numpy checker of the JSON import (tests/checkers/json_import_ref.py) against the reference's
own output, G12 (tests/golden/make_json_import_golden.py: _load_json_prediction_data,
_create_gt_overlay_with_consistent_colors and _create_consistent_prediction_overlay of
mask2former/predictor.py, pycocotools' decode restated by oracle/rle.py), bit for bit."""
import json
from pathlib import Path

import numpy as np
import pytest

from checkers import json_import_ref as jr
from oracle import rle

GOLDEN = Path(__file__).parent / "golden"
LOAD_NAMES = ["covered_empty_repeat", "overlap_order", "later_upscaled", "later_downscaled", "later_ragged",
              "downscale_vanishes", "first_small", "only_small", "image_larger", "short_labels", "short_scores",
              "empty_list", "only_empty", "missing_scores", "many_255"]
CMP_NAMES = ["three_models", "resized_model", "gt_none"]


@pytest.fixture(scope="module")
def g12():
    return np.load(GOLDEN / "g12_json_import.npz")


def test_fixture_holds_the_cases_the_loader_is_held_to(g12):
    assert [str(n) for n in g12["names"]] == LOAD_NAMES and [str(n) for n in g12["cmp_names"]] == CMP_NAMES
    assert str(g12["numpy_version"]).split(".")[0] == "2"  # the blend's promotion rules (G10)
    assert g12["image"].shape == (24, 40, 3) and list(g12["alphas"]) == [0.6, 0.37]
    none = {n: bool(g12[f"l{k}_none"]) for k, n in enumerate(LOAD_NAMES)}
    assert [n for n in LOAD_NAMES if none[n]] == ["first_small", "only_small", "image_larger", "empty_list",
                                                  "only_empty", "missing_scores"]
    k = LOAD_NAMES.index("covered_empty_repeat")  # listed but covered: the file route into Q19
    assert g12[f"l{k}_ids"].tolist() == [1, 2, 4] and np.unique(g12[f"l{k}_map"]).tolist() == [0, 2, 4]
    assert g12[f"l{LOAD_NAMES.index('many_255')}_ids"].tolist() == list(range(1, 256))


@pytest.mark.parametrize("k", range(len(LOAD_NAMES)), ids=LOAD_NAMES)
def test_checker_loads_what_the_reference_loads(g12, k):
    got = jr.load_prediction(jr.case_json(g12, f"l{k}_json"), g12[f"l{k}_shape"].tolist())
    assert (got is None) == bool(g12[f"l{k}_none"])
    if got is not None:
        seg, ids, labels, scores = got
        assert seg.dtype == np.int32 and np.array_equal(seg, g12[f"l{k}_map"])
        assert ids == g12[f"l{k}_ids"].tolist() and labels == g12[f"l{k}_labels"].tolist()
        assert scores == g12[f"l{k}_scores"].tolist()


@pytest.mark.parametrize("k", range(len(CMP_NAMES)), ids=CMP_NAMES)
def test_checker_compares_as_the_reference_compares(g12, k):
    palette = np.load(GOLDEN / "g10_overlay.npz")["palette100"]  # generate_consistent_colors(100): a prefix serves
    models = [json.loads(str(t)) for t in g12[f"m{k}_models"]]
    for a, alpha in enumerate(g12["alphas"]):
        gt_ov, outs = jr.comparison(g12["image"], jr.case_json(g12, f"m{k}_gt"), models, float(alpha), 0.5, palette)
        assert np.array_equal(gt_ov, g12[f"m{k}_gt_overlays"][a])
        assert np.array_equal(np.stack(outs), g12[f"m{k}_model_overlays"][a])
    for j, none in enumerate(g12[f"m{k}_model_none"]):
        if none or bool(g12[f"m{k}_gt_none"]):
            assert np.array_equal(g12[f"m{k}_model_overlays"][0][j], g12["image"])


def test_string_decode_is_the_oracles():
    """The vectorised string decode against oracle.rle.rle_from_string, on encoded random masks
    and on hand-made count lists with zero-length runs and negative deltas."""
    rng = np.random.RandomState(3)
    lists = [[0, 5, 0, 3, 2], [960], [0, 960], [1, 1, 1, 1], [5], [3, 4], [3, 4, 5], [900, 30, 5, 1, 24],
             [0, 1, 40000, 1, 3, 70000, 2]]
    lists += [rle.rle_encode((rng.rand(23, 37) < p).astype(np.uint8))[2] for p in (0.05, 0.5, 0.95)]
    for counts in lists:
        s = rle.rle_to_string(counts)
        got, trunc = jr.counts_from_string(s)
        assert got.tolist() == rle.rle_from_string(s) == [int(c) for c in counts] and not trunc
    m = (rng.rand(23, 37) < 0.4).astype(np.uint8)
    assert np.array_equal(jr.decode_rle(rle.encode(m)), m.astype(bool))
    assert jr.counts_from_string("5" + chr(48 + 0x25))[1]  # the last group announces another
