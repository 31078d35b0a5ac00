"""The numpy checker of the segment matcher (tests/checkers/match_ref.py) against the reference's
own output, G11 (tests/golden/make_match_golden.py: match_predictions_to_gt and
_create_consistent_prediction_overlay of mask2former/predictor.py), bit for bit."""
from pathlib import Path

import numpy as np
import pytest

from checkers import match_ref

G11 = Path(__file__).parent / "golden" / "g11_match.npz"


@pytest.fixture(scope="module")
def g11():
    return np.load(G11)


def _names(g):
    return [str(n) for n in g["names"]]


def test_fixture_holds_the_cases_the_matcher_is_held_to(g11):
    assert _names(g11) == ["plain", "ties", "threshold", "empty_before_matched", "color_missing", "no_gt",
                           "gt_all_empty", "no_pred"]
    assert str(g11["numpy_version"]).split(".")[0] == "2"  # the blend's promotion rules (G10)
    assert g11["image"].shape == (24, 40, 3) and list(g11["alphas"]) == [0.6, 0.37]


@pytest.mark.parametrize("k", range(8))
def test_checker_is_the_reference_bitwise(g11, k):
    g = {n.split("_", 1)[1]: g11[n] for n in g11.files if n.startswith(f"c{k}_")}
    colors = {int(i): tuple(int(v) for v in c) for i, c in zip(g["color_ids"], g["color_rgb"])}
    for alpha, want in zip(g11["alphas"], g["overlays"]):
        got, (matched, is_matched, counts) = match_ref.consistent_overlay(
            g11["image"], g["pred"], g["pred_ids"].tolist(), g["gt"], g["gt_ids"].tolist(), colors, float(alpha),
            float(g["thr"]))
        assert np.array_equal(got, want), f"{_names(g11)[k]} at alpha {alpha}: overlay"
        assert matched == g["matched"].tolist() and is_matched == g["is_matched"].tolist()
        assert counts == g["gt_counts"].tolist()


def test_the_cases_show_what_they_are_named_for(g11):
    names = _names(g11)
    k = names.index("ties")
    # prediction 3 (listed first) wins GT 0 over prediction 1; prediction 2 takes GT 5 (listed first)
    assert g11[f"c{k}_matched"].tolist() == [2, -1, 0]
    k = names.index("threshold")
    assert g11[f"c{k}_matched"].tolist() == [0, -1]
    k = names.index("empty_before_matched")
    # filtered: id 1 unmatched, id 2 matched.  Painted: id 1 (list position 1) reads is_matched[1],
    # id 2's, and takes GT 3's colour; id 2 (position 2) lies past the filtered length: red.
    assert g11[f"c{k}_matched"].tolist() == [-1, 0]
    img, out, pred = g11["image"], g11[f"c{k}_overlays"][0], g11[f"c{k}_pred"]
    lut = np.full((1, 3), -1, np.int32)
    lut[0, 1], lut[0, 2] = match_ref.pack((20, 220, 120)), match_ref.pack((255, 0, 0))
    assert np.array_equal(out, match_ref.overlay_ref.blend(img[None], pred[None], lut, 0.6)[0])


def test_cell_rule_and_contingency_sums():
    a = np.array([[[0, 1.5, np.nan, -1, 2, 3, 1, 1]]], np.float32)
    b = np.array([[[0, 0, 1, 1, 7, 2, -5, 1]]], np.int32)
    assert match_ref.cell_ids(a[0], 3).tolist() == [[0, 3, 3, 3, 2, 3, 1, 1]]
    c = match_ref.contingency(a, b, 3, 2)
    assert c.shape == (1, 4, 3) and c.sum() == 8 and c.dtype == np.int32
    assert c[0, 0, 0] == 1 and c[0, 3, 0] == 1 and c[0, 3, 1] == 2 and c[0, 2, 2] == 1 and c[0, 1, 2] == 1 and c[0, 1, 1] == 1


def test_track_assignment():
    Q = 4
    none = np.full((1, 2, 6), -1, np.float32)
    f0 = none.copy()
    f0[0, 0, :3], f0[0, 1, :3] = 2, 0
    tr, nxt = match_ref.track_step(f0, none, np.full((1, Q), -1, np.int32), np.zeros(1, np.int32), Q, 0.5)
    assert tr.tolist() == [[0, -1, 1, -1]] and nxt.tolist() == [2]      # fresh tracks in id order
    f1 = none.copy()
    f1[0, 0, :3], f1[0, 1, 3:], f1[0, 1, :3] = 1, 3, 0               # id 1 lies where id 2 lay; id 3 is new
    tr1, nxt1 = match_ref.track_step(f1, f0, tr, nxt, Q, 0.5)
    assert tr1.tolist() == [[0, 1, -1, 2]] and nxt1.tolist() == [3]
    lut = match_ref.track_lut(tr1, [(1, 2, 3), (4, 5, 6)])
    assert lut.tolist() == [[match_ref.pack((1, 2, 3)), match_ref.pack((4, 5, 6)), -1, match_ref.pack((1, 2, 3))]]
