"""The references of the dense post-processing tests, on the CPU.

1. tests/checkers/panoptic_ref.py (float64, with the intermediates exposed) gives the same map and
   the same segments_info as the HF method fed float64 inputs, on every fixture.
2. The fixtures are fit for purpose: every branch of compute_segments is taken, and every discrete
   decision (keep by score, accept by area ratio, the rounded score, the argmax of a pixel) has a
   margin wide enough that a float32 run must decide it the same way -- so the GPU test
   (tests/test_gpu_postprocess_dense.py) may ask for identical segments_info.
"""
import numpy as np
import pytest
import torch

from checkers import panoptic_ref as pr

THRESHOLD, OVERLAP = 0.5, 0.8


@pytest.mark.parametrize("name,ti", pr.CASE_PARAMS, ids=pr.CASE_IDS)
def test_checker_matches_hf_on_float64(name, ti):
    cl, ml, fuse, _ = pr.case_inputs(name)
    ts = pr.case_targets(name, ti)
    hf = pr.hf_processor().post_process_panoptic_segmentation(pr.outputs_of(cl, ml, torch.float64),
                                                              label_ids_to_fuse=fuse, target_sizes=ts)
    for want, got in zip(hf, pr.case_panoptic_ref(name, ti)):
        assert want["segmentation"].dtype == got["segmentation"].dtype == torch.int32
        assert torch.equal(want["segmentation"], got["segmentation"])
        assert want["segments_info"] == got["segments_info"]


def test_checker_nothing_kept_and_no_fuse_set_match_hf():
    cl, ml, _, _ = pr.case_inputs("ragged")
    outs = pr.outputs_of(cl, ml, torch.float64)
    hf = pr.hf_processor().post_process_panoptic_segmentation(outs, threshold=1.1, target_sizes=[(37, 53), (9, 7)])
    for b, want in enumerate(hf):
        got = pr.panoptic_ref(cl[b], ml[b], threshold=1.1, target_size=[(37, 53), (9, 7)][b])
        assert want["segmentation"].dtype == got["segmentation"].dtype == torch.float32
        assert torch.equal(want["segmentation"], got["segmentation"]) and got["segments_info"] == []
    hf = pr.hf_processor().post_process_panoptic_segmentation(outs)  # label_ids_to_fuse=None
    for b, want in enumerate(hf):
        got = pr.panoptic_ref(cl[b], ml[b])
        assert torch.equal(want["segmentation"], got["segmentation"])
        assert want["segments_info"] == got["segments_info"]
        assert not any(s["was_fused"] for s in got["segments_info"])


@pytest.mark.parametrize("name,ti", pr.CASE_PARAMS, ids=pr.CASE_IDS)
def test_fixtures_take_every_branch_with_margins(name, ti):
    cl, _, fuse, roles = pr.case_inputs(name)
    C = cl.shape[-1] - 1
    for b, ref in enumerate(pr.case_panoptic_ref(name, ti)):
        role = [roles[b][q] for q in ref["kept"].tolist()]
        info = ref["segments_info"]
        print(name, ti, b, [(r, a, o, round(x, 4)) for r, a, o, x in zip(role, ref["area"], ref["orig"], ref["ratio"])])
        assert any(not s["was_fused"] for s in info), "no accepted, unfused segment"
        fused_ids = [s["id"] for s in info if s["was_fused"]]
        assert len(fused_ids) == 2 and fused_ids[0] == fused_ids[1], "no two queries fused into one id"
        k = role.index("victim")
        assert not ref["valid"][k] and 0 < ref["ratio"][k] < OVERLAP, "no query rejected by its ratio"
        k = role.index("shadow")
        assert ref["area"][k] == 0 and ref["orig"][k] > 0, "no query with area 0"
        assert bool((ref["all_labels"] == C).any()), "no query removed as no-object"
        real = ref["all_labels"] != C
        assert bool((real & (ref["all_scores"] <= THRESHOLD)).any()), "no query removed by its score"
        # margins: a float32 run decides the same way
        assert float((ref["all_scores"][real] - THRESHOLD).abs().min()) >= 1e-3
        ratios = [r for r, a, o in zip(ref["ratio"], ref["area"], ref["orig"]) if a > 0 and o > 0]
        assert min(abs(r - OVERLAP) for r in ratios) >= 0.02
        # round(score, 6): a float32 score is within a few 2^-24 of the float64 one, so the sixth
        # decimal is the same when score * 1e6 is at least 0.15 away from a rounding boundary
        frac = (ref["scores"] * 1e6) % 1.0
        assert float((frac - 0.5).abs().min()) >= 0.15, "a score rounds differently in float32"
        # pixels whose argmax float32 may decide differently: at most 1 % of the image
        band = ref["gap"] < pr.PAN_BAR * max(1.0, float(ref["P"].max()))
        assert float(band.double().mean()) <= pr.BAND_CAP


@pytest.mark.parametrize("name,ti", pr.CASE_PARAMS, ids=pr.CASE_IDS)
def test_semantic_reference_band_is_thin(name, ti):
    """The share of pixels whose float64 top-2 class gap is below twice the score bar: at most 1 %."""
    for seg, scores in pr.case_semantic_ref(name, ti):
        assert seg.dtype == torch.int64 and scores.dtype == torch.float64
        bar = pr.SEM_BAR * max(1.0, float(scores.abs().max()))
        band = pr.top2_gap(scores) < 2 * bar
        print(name, ti, float(band.double().mean()))
        assert float(band.double().mean()) <= pr.BAND_CAP


def test_blob_case_is_deterministic():
    a, b = pr.blob_case(3, 11, 5, 12, 20), pr.blob_case(3, 11, 5, 12, 20)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[3] == b[3]
