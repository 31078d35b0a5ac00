"""C-ABI checks of the segment-matching entry points that run without a GPU: the symbols are
exported and bound, and every documented return code comes back from the host-side validation
before anything is launched (the pointers handed in are never dereferenced)."""
import ctypes

import pytest

from rgbd_amd import _lib

NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(0x100000)
F32, BF16, I32 = _lib.RGBD_F32, _lib.RGBD_BF16, _lib.RGBD_I32
E_ARG, E_SHAPE, E_DTYPE = -1, -2, -3
NAMES = ("rgbd_label_contingency", "rgbd_greedy_iou_match", "rgbd_match_lut", "rgbd_track_assign")


def _cont(L, a_dtype=F32, b_dtype=I32, B=2, H=3, W=5, na=4, nb=6, **ptr):
    p = dict(a=FAKE, b=FAKE, counts=FAKE)
    p.update(ptr)
    return L.rgbd_label_contingency(p["a"], a_dtype, p["b"], b_dtype, B, H, W, na, nb, p["counts"], NULL)


def _match(L, B=2, na=4, nb=6, hw=15, La=3, Lb=5, thr=0.5, **ptr):
    p = dict(counts=FAKE, a_list=FAKE, b_list=FAKE, matched=FAKE, b_match_count=FAKE, n_filtered=FAKE)
    p.update(ptr)
    return L.rgbd_greedy_iou_match(p["counts"], B, na, nb, hw, p["a_list"], La, p["b_list"], Lb, thr, p["matched"],
                                   p["b_match_count"], p["n_filtered"], NULL)


def _lut(L, mode=0, B=2, na=4, nb=6, La=3, Lb=5, unmatched=255, n_colors=3, **ptr):
    p = dict(counts=FAKE, a_list=FAKE, b_list=FAKE, matched=FAKE, n_filtered=FAKE, gt_colors=FAKE, track=FAKE,
             palette=FAKE, lut=FAKE)
    p.update(ptr)
    return L.rgbd_match_lut(mode, p["counts"], B, na, nb, p["a_list"], La, p["b_list"], Lb, p["matched"],
                            p["n_filtered"], p["gt_colors"], unmatched, p["track"], p["palette"], n_colors, p["lut"], NULL)


def _track(L, B=2, Q=5, **ptr):
    p = dict(counts=FAKE, matched=FAKE, prev_track=FAKE, next_track=FAKE, track=FAKE)
    p.update(ptr)
    return L.rgbd_track_assign(p["counts"], B, Q, p["matched"], p["prev_track"], p["next_track"], p["track"], NULL)


def test_symbols_exported_and_bound():
    L = _lib.lib()
    for n in NAMES:
        assert hasattr(L, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES and n in _lib.header_symbols()


@pytest.mark.parametrize("name", ["a", "b", "counts"])
def test_contingency_null_pointer(name):
    assert _cont(_lib.lib(), **{name: NULL}) == E_ARG


def test_contingency_sizes_dtypes_and_alignment():
    L = _lib.lib()
    for bad in (dict(B=0), dict(B=-1), dict(H=0), dict(H=-3), dict(W=0), dict(W=-1), dict(na=0), dict(na=-1),
                dict(nb=0), dict(nb=-7)):
        assert _cont(L, **bad) == E_ARG, bad
    for bad in (BF16, 3, -1):
        assert _cont(L, a_dtype=bad) == E_DTYPE and _cont(L, b_dtype=bad) == E_DTYPE, bad
    assert _cont(L, na=257) == E_SHAPE and _cont(L, nb=257) == E_SHAPE
    assert _cont(L, B=1 << 16) == E_SHAPE                  # one grid row per image
    assert _cont(L, H=1 << 16, W=1 << 15) == E_SHAPE       # 2^31 pixels per image: the counts are int32
    for off in (1, 2, 3):                                  # 4-byte alignment is required
        for name in ("a", "b", "counts"):
            assert _cont(L, **{name: ctypes.c_void_p(FAKE.value + off)}) == E_ARG, (name, off)


@pytest.mark.parametrize("name", ["counts", "a_list", "b_list", "matched", "b_match_count", "n_filtered"])
def test_match_null_pointer(name):
    assert _match(_lib.lib(), **{name: NULL}) == E_ARG


def test_match_sizes_and_threshold():
    L = _lib.lib()
    for bad in (dict(B=0), dict(B=-1), dict(na=0), dict(nb=-1), dict(hw=0), dict(hw=-5), dict(La=0), dict(La=-1),
                dict(Lb=0), dict(Lb=-2), dict(thr=float("nan")), dict(thr=float("inf")), dict(thr=float("-inf"))):
        assert _match(L, **bad) == E_ARG, bad
    for bad in (dict(na=257), dict(nb=257), dict(La=257), dict(Lb=257), dict(hw=(1 << 21) + 1)):
        assert _match(L, **bad) == E_SHAPE, bad


@pytest.mark.parametrize("name", ["counts", "a_list", "b_list", "matched", "n_filtered", "gt_colors", "lut"])
def test_lut_gt_null_pointer(name):
    assert _lut(_lib.lib(), **{name: NULL}) == E_ARG


@pytest.mark.parametrize("name", ["track", "palette", "lut"])
def test_lut_track_null_pointer(name):
    assert _lut(_lib.lib(), mode=1, **{name: NULL}) == E_ARG


def test_lut_sizes_and_modes():
    L = _lib.lib()
    for bad in (dict(mode=2), dict(mode=-1), dict(B=0), dict(na=0), dict(nb=0), dict(La=0), dict(Lb=-1),
                dict(unmatched=-1), dict(unmatched=1 << 24), dict(mode=1, n_colors=0), dict(mode=1, B=-1),
                dict(mode=1, na=0)):
        assert _lut(L, **bad) == E_ARG, bad
    for bad in (dict(na=257), dict(nb=257), dict(La=257), dict(Lb=257), dict(mode=1, na=257), dict(mode=1, B=1 << 16)):
        assert _lut(L, **bad) == E_SHAPE, bad


@pytest.mark.parametrize("name", ["counts", "matched", "prev_track", "next_track", "track"])
def test_track_null_pointer(name):
    assert _track(_lib.lib(), **{name: NULL}) == E_ARG


def test_track_sizes():
    L = _lib.lib()
    for bad in (dict(B=0), dict(B=-1), dict(Q=0), dict(Q=-1)):
        assert _track(L, **bad) == E_ARG, bad
    assert _track(L, Q=257) == E_SHAPE


def test_wrappers_refuse_cpu_tensors_duplicates_and_a_missing_ground_truth():
    import torch
    from rgbd_amd import overlay
    img = torch.zeros(4, 6, 3, dtype=torch.uint8)
    res = {"segmentation": torch.zeros(4, 6), "segments_info": [{"id": 0}, {"id": 1}]}
    with pytest.raises(RuntimeError, match="GPU only"):
        overlay.match_segments(res, res)
    with pytest.raises(RuntimeError, match="GPU only"):
        overlay.consistent_prediction_overlay(img, res, {0: (1, 2, 3)}, res)
    with pytest.raises(RuntimeError, match="GPU only"):
        overlay.label_contingency(torch.zeros(1, 4, 6), torch.zeros(1, 4, 6), 3, 3)
    dup = {"segmentation": torch.zeros(4, 6), "segments_info": [{"id": 2}, {"id": 0}, {"id": 2}]}
    for pred, gt in ((dup, res), (res, dup)):
        with pytest.raises(ValueError, match="duplicate ids"):
            overlay.match_segments(pred, gt)
        with pytest.raises(ValueError, match="duplicate ids"):
            overlay.consistent_prediction_overlay(img, pred, {}, gt)
    with pytest.raises(ValueError, match="gt_prediction is required"):
        overlay.consistent_prediction_overlay(img, res, {}, None)
