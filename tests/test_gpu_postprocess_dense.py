"""Semantic and panoptic post-processing on the GPU (csrc/postprocess_dense.hip) against float64:
the HF method on float64 inputs for the semantic scores and maps, tests/checkers/panoptic_ref.py
(pinned against HF in tests/test_postprocess_dense_ref.py, which also asserts the fixtures'
margins) for the panoptic maps and segments_info.

Error bars.  Semantic scores: max|S - S64| <= 2e-5 max(1, max|S64|) -- a float32 sum of Q = 100
non-negative terms is within Q 2^-24 = 6e-6 relative, plus two bilinear passes and the sigmoid.
Maps are compared wherever the float64 top-2 gap is at least twice that bar (semantic) or at
least 2e-6 max(1, max P) (panoptic: the weighted probability is one sigmoid, one bilinear pass and
one product away from the logits); at most 1 % of an image may lie inside the band.
"""
import types

import numpy as np
import pytest
import torch

from checkers import panoptic_ref as pr

pytestmark = pytest.mark.gpu


def _outs(cl, ml):
    return types.SimpleNamespace(class_queries_logits=torch.as_tensor(cl), masks_queries_logits=torch.as_tensor(ml))


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("name,ti", pr.CASE_PARAMS, ids=pr.CASE_IDS)
def test_semantic_scores_and_maps_match_float64(name, ti):
    from rgbd_amd.postprocess import post_process_semantic_segmentation
    from transformers.image_processing_outputs import SemanticSegmentationPostProcessorOutput
    cl, ml, _, _ = pr.case_inputs(name)
    ts = pr.case_targets(name, ti)
    got = post_process_semantic_segmentation(_outs(cl, ml), target_sizes=ts, return_segmentation_scores=True)
    maps_only = post_process_semantic_segmentation(_outs(cl, ml), target_sizes=ts)
    ref = pr.case_semantic_ref(name, ti)
    assert len(got) == len(ref) == len(maps_only)
    for b, (g, (seg64, s64)) in enumerate(zip(got, ref)):
        assert isinstance(g, SemanticSegmentationPostProcessorOutput)
        seg, s = g.segmentation, g.segmentation_scores
        assert seg.dtype == torch.int64 and s.dtype == torch.float32 and seg.device.type == s.device.type == "cpu"
        assert seg.shape == seg64.shape and s.shape == s64.shape
        bar = pr.SEM_BAR * max(1.0, float(s64.abs().max()))
        err = float((s.double() - s64).abs().max())
        band = pr.top2_gap(s64) < 2 * bar
        print(f"{name}-{ti} image {b}: max|S - S64| = {err:.3e} (bar {bar:.3e}, max|S64| {float(s64.abs().max()):.3f}), "
              f"band {float(band.double().mean()):.2e}, map differs at {int((seg != seg64).sum())} pixels")
        assert err <= bar
        assert float(band.double().mean()) <= pr.BAND_CAP
        assert torch.equal(seg[~band], seg64[~band])
        assert _bits_equal(maps_only[b], seg)


@pytest.mark.parametrize("name,ti", pr.CASE_PARAMS, ids=pr.CASE_IDS)
def test_panoptic_matches_float64_checker(name, ti):
    from rgbd_amd.postprocess import post_process_panoptic_segmentation
    cl, ml, fuse, _ = pr.case_inputs(name)
    ts = pr.case_targets(name, ti)
    got = post_process_panoptic_segmentation(_outs(cl, ml), label_ids_to_fuse=fuse, target_sizes=ts)
    ref = pr.case_panoptic_ref(name, ti)
    assert len(got) == len(ref)
    for b, (g, r) in enumerate(zip(got, ref)):
        seg = g["segmentation"]
        assert seg.dtype == torch.int32 and seg.device.type == "cpu" and seg.shape == r["segmentation"].shape
        assert g["segments_info"] == r["segments_info"]
        band = r["gap"] < pr.PAN_BAR * max(1.0, float(r["P"].max()))
        print(f"{name}-{ti} image {b}: {len(g['segments_info'])} segments, band {float(band.double().mean()):.2e}, "
              f"map differs at {int((seg != r['segmentation']).sum())} pixels")
        assert float(band.double().mean()) <= pr.BAND_CAP
        # areas differ from float64 by the band's pixels at the most: everything else is identical
        assert torch.equal(seg[~band], r["segmentation"][~band])


def test_semantic_exact_tie_goes_to_the_lower_class():
    """Two identical class columns give bit-identical scores; the argmax takes the lower id."""
    from rgbd_amd.postprocess import post_process_semantic_segmentation
    cl, ml, _, roles = pr.case_inputs("ragged")
    cl, ml = cl.copy(), ml.copy()
    cl[:, :, 3] = cl[:, :, 1]  # the 'plain' blob's class, twice: each column gets half its probability
    ml[:, roles[0].index("background")] = -2.0  # so that the tied pair leads on that blob
    assert roles[0] == roles[1]
    for ts in (None, [(37, 53), (97, 131)]):
        for g in post_process_semantic_segmentation(_outs(cl, ml), target_sizes=ts, return_segmentation_scores=True):
            s, seg = g.segmentation_scores, g.segmentation
            assert _bits_equal(s[1], s[3])
            tied_top = s[1] >= s.max(0).values
            assert bool(tied_top.any()) and bool((seg[tied_top] == 1).all()) and not bool((seg == 3).any())


@pytest.mark.parametrize("ts", [None, [(37, 53), (97, 131)]])
def test_panoptic_identical_queries_the_earlier_takes_every_pixel(ts):
    """A low-score query (dropped by the threshold) is overwritten with a copy of an accepted one,
    row and mask.  The copy is kept, ties the original at every pixel, loses every tie (the first
    maximum wins), has area 0 and is not a segment: map and segments_info must be bitwise those of
    the unmodified input.  (The CPU reference is no witness here: ATen's CPU bilinear kernel
    rounds the same values differently in different channels -- vector body against remainder --
    so its two copies differ in the last bit at hundreds of pixels at 37 x 53.)"""
    from rgbd_amd.postprocess import post_process_panoptic_segmentation
    cl, ml, fuse, roles = pr.case_inputs("ragged")
    want = post_process_panoptic_segmentation(_outs(cl, ml), label_ids_to_fuse=fuse, target_sizes=ts)
    cl, ml = cl.copy(), ml.copy()
    for b in range(cl.shape[0]):
        src, dup = roles[b].index("plain"), roles[b].index("low")
        assert src < dup
        cl[b, dup], ml[b, dup] = cl[b, src], ml[b, src]
    got = post_process_panoptic_segmentation(_outs(cl, ml), label_ids_to_fuse=fuse, target_sizes=ts)
    for g, w in zip(got, want):
        assert len(w["segments_info"]) > 0 and g["segments_info"] == w["segments_info"]
        assert _bits_equal(g["segmentation"], w["segmentation"])


@pytest.mark.parametrize("ts", [None, [(37, 53), (97, 131)]])
def test_panoptic_nothing_kept(ts):
    from rgbd_amd.postprocess import post_process_panoptic_segmentation
    cl, ml, fuse, _ = pr.case_inputs("ragged")
    got = post_process_panoptic_segmentation(_outs(cl, ml), threshold=1.1, label_ids_to_fuse=fuse, target_sizes=ts)
    for b, g in enumerate(got):
        seg = g["segmentation"]
        assert seg.dtype == torch.float32 and seg.shape == ((384, 384) if ts is None else ts[b])
        assert bool((seg == -1).all()) and g["segments_info"] == []


def test_panoptic_some_kept_none_valid():
    from rgbd_amd.postprocess import post_process_panoptic_segmentation
    cl, ml, fuse, _ = pr.case_inputs("ragged")
    got = post_process_panoptic_segmentation(_outs(cl, ml), overlap_mask_area_threshold=1.5, label_ids_to_fuse=fuse,
                                             target_sizes=[(37, 53), (97, 131)])
    for g in got:
        assert g["segmentation"].dtype == torch.int32 and bool((g["segmentation"] == 0).all())
        assert g["segments_info"] == []


def test_panoptic_no_fuse_set_is_the_empty_set():
    from rgbd_amd.postprocess import post_process_panoptic_segmentation
    cl, ml, _, _ = pr.case_inputs("ragged")
    a = post_process_panoptic_segmentation(_outs(cl, ml), label_ids_to_fuse=None)
    b = post_process_panoptic_segmentation(_outs(cl, ml), label_ids_to_fuse=set())
    for b_, (x, y) in enumerate(zip(a, b)):
        assert _bits_equal(x["segmentation"], y["segmentation"]) and x["segments_info"] == y["segments_info"]
        assert x["segments_info"] == pr.panoptic_ref(cl[b_], ml[b_])["segments_info"]
        assert len({s["id"] for s in x["segments_info"]}) == len(x["segments_info"]) > 0
        assert not any(s["was_fused"] for s in x["segments_info"])


def test_panoptic_fuse_set_of_numpy_integers():
    """HF asks ``label in label_ids_to_fuse``, which a set of numpy integers answers like one of ints."""
    from rgbd_amd.postprocess import post_process_panoptic_segmentation
    cl, ml, fuse, _ = pr.case_inputs("ragged")
    a = post_process_panoptic_segmentation(_outs(cl, ml), label_ids_to_fuse=fuse)
    b = post_process_panoptic_segmentation(_outs(cl, ml), label_ids_to_fuse={np.int64(c) for c in fuse})
    for x, y in zip(a, b):
        assert any(s["was_fused"] for s in x["segments_info"]) and x["segments_info"] == y["segments_info"]
        assert _bits_equal(x["segmentation"], y["segmentation"])


def test_target_size_count_mismatch_raises():
    from rgbd_amd.postprocess import post_process_panoptic_segmentation, post_process_semantic_segmentation
    cl, ml, _, _ = pr.case_inputs("ragged")
    with pytest.raises(ValueError, match="as many target sizes"):
        post_process_semantic_segmentation(_outs(cl, ml), target_sizes=[(37, 53)])
    with pytest.raises(ValueError, match="as many target sizes"):
        post_process_panoptic_segmentation(_outs(cl, ml), label_ids_to_fuse=set(), target_sizes=[(37, 53)] * 3)


def test_two_calls_give_equal_bits():
    from rgbd_amd.postprocess import post_process_panoptic_segmentation, post_process_semantic_segmentation
    cl, ml, fuse, _ = pr.case_inputs("workload")
    ts = pr.case_targets("workload", 0)
    outs = _outs(torch.as_tensor(cl).cuda(), torch.as_tensor(ml).cuda())
    sem = [post_process_semantic_segmentation(outs, target_sizes=ts, return_segmentation_scores=True,
                                              keep_on_device=True) for _ in range(2)]
    pan = [post_process_panoptic_segmentation(outs, label_ids_to_fuse=fuse, target_sizes=ts, keep_on_device=True)
           for _ in range(2)]
    for x, y in zip(*sem):
        assert x.segmentation.is_cuda and x.segmentation_scores.is_cuda
        assert _bits_equal(x.segmentation, y.segmentation) and _bits_equal(x.segmentation_scores, y.segmentation_scores)
    for x, y in zip(*pan):
        assert x["segmentation"].is_cuda
        assert _bits_equal(x["segmentation"], y["segmentation"]) and x["segments_info"] == y["segments_info"]


def test_bf16_and_cpu_inputs_are_taken_as_float32():
    """bf16 logits are widened to float32 on the device: the result is that of the widened values."""
    from rgbd_amd.postprocess import post_process_semantic_segmentation
    cl, ml, _, _ = pr.case_inputs("ragged")
    cb, mb = torch.as_tensor(cl).bfloat16(), torch.as_tensor(ml).bfloat16()
    a = post_process_semantic_segmentation(_outs(cb, mb))
    b = post_process_semantic_segmentation(_outs(cb.float().cuda(), mb.float().cuda()))
    for x, y in zip(a, b):
        assert _bits_equal(x, y)


def test_install_routes_the_tasks_asked_for():
    from transformers.models.mask2former.image_processing_pil_mask2former import Mask2FormerImageProcessorPil as P
    from rgbd_amd import postprocess as pp
    cl, ml, fuse, _ = pr.case_inputs("ragged")
    outs = _outs(cl, ml)
    proc = pp.install(P())  # the default: the instance path alone
    assert proc.post_process_semantic_segmentation.__func__ is P.post_process_semantic_segmentation
    assert proc.post_process_panoptic_segmentation.__func__ is P.post_process_panoptic_segmentation
    assert not hasattr(proc, "_hf_post_process_semantic_segmentation")
    assert proc._hf_post_process_instance_segmentation.__func__ is P.post_process_instance_segmentation
    proc = pp.install(P(), tasks=("instance", "semantic", "panoptic"))
    for name in ("instance", "semantic", "panoptic"):
        assert getattr(proc, f"_hf_post_process_{name}_segmentation").__func__ is \
            getattr(P, f"post_process_{name}_segmentation")
    # keep_on_device is an argument of the device paths only: the HF methods would refuse it
    assert proc.post_process_semantic_segmentation(outs, keep_on_device=True)[0].is_cuda
    assert proc.post_process_panoptic_segmentation(outs, label_ids_to_fuse=fuse, keep_on_device=True)[0][
        "segmentation"].is_cuda
    assert proc.post_process_instance_segmentation(outs, keep_on_device=True)[0]["segmentation"].is_cuda
    ts = [(37, 53), (97, 131)]
    want = pp.post_process_panoptic_segmentation(outs, label_ids_to_fuse=fuse, target_sizes=ts)
    got = proc.post_process_panoptic_segmentation(outs, label_ids_to_fuse=fuse, target_sizes=ts)
    for x, y in zip(want, got):
        assert _bits_equal(x["segmentation"], y["segmentation"]) and x["segments_info"] == y["segments_info"]
    with pytest.raises(ValueError, match="unknown post-processing task"):
        pp.install(P(), tasks=("depth",))


def test_inputs_beyond_the_caps_take_the_hf_method():
    """More than 1024 classes: the installed processor returns HF's own result (no device call
    could: rgbd_pp_panoptic refuses the shape)."""
    from transformers.models.mask2former.image_processing_pil_mask2former import Mask2FormerImageProcessorPil as P
    from rgbd_amd import _lib, postprocess as pp
    rng = np.random.default_rng(2)
    C = pp.MAX_CLASSES + 1
    cl = (0.5 * rng.standard_normal((1, 3, C + 1))).astype(np.float32)
    cl[0, 0, C - 1] += 14.0
    cl[0, 1, 7] += 14.0
    ml = (0.3 * rng.standard_normal((1, 3, 6, 8))).astype(np.float32)
    ml[0, 0, :, :4] += 4.0  # two segments side by side
    ml[0, 0, :, 4:] -= 4.0
    ml[0, 1] = -ml[0, 0]
    outs = _outs(cl, ml)
    want = P().post_process_panoptic_segmentation(outs, label_ids_to_fuse={7}, target_sizes=[(20, 30)])
    proc = pp.install(P(), tasks=("semantic", "panoptic"))
    got = proc.post_process_panoptic_segmentation(outs, label_ids_to_fuse={7}, target_sizes=[(20, 30)])
    assert len(want[0]["segments_info"]) > 0 and got[0]["segments_info"] == want[0]["segments_info"]
    assert _bits_equal(got[0]["segmentation"], want[0]["segmentation"])
    with pytest.raises(_lib.RgbdHipError, match="unsupported shape"):
        pp.post_process_panoptic_segmentation(outs, label_ids_to_fuse={7})
    # the semantic route, without paying for HF's [1025, 384, 384] scores: a stand-in original
    stub = types.SimpleNamespace(post_process_semantic_segmentation=lambda outputs, **kw: "original")
    assert pp.install(stub, tasks=("semantic",)).post_process_semantic_segmentation(outs) == "original"
    assert not pp._dense_covers(_outs(np.zeros((1, pp.MAX_QUERIES + 1, 3), np.float32),
                                      np.zeros((1, pp.MAX_QUERIES + 1, 2, 2), np.float32)), panoptic=True)
