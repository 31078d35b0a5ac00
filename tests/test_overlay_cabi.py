"""C-ABI checks of the overlay entry points that run without a GPU: the symbols are exported and
bound, and every documented return code comes back from the host-side validation before anything
is launched (the pointers handed in are never dereferenced)."""
import ctypes

import pytest

from rgbd_amd import _lib

NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(0x100000)
FAKE_OUT = ctypes.c_void_p(0x40000000)  # far enough from FAKE that no rgb range reaches it
F32, BF16, I32 = _lib.RGBD_F32, _lib.RGBD_BF16, _lib.RGBD_I32
E_ARG, E_SHAPE, E_DTYPE = -1, -2, -3


def _lut(L, B=2, Q=5, C=7, n_colors=3, color_by=0, n_ids=5, **ptr):
    p = dict(seg_id=FAKE, topk_idx=FAKE, palette=FAKE, lut=FAKE)
    p.update(ptr)
    return L.rgbd_overlay_lut(p["seg_id"], p["topk_idx"], B, Q, C, p["palette"], n_colors, color_by, p["lut"], n_ids,
                              NULL)


def _blend(L, dtype=F32, B=2, H=3, W=5, n_ids=4, alpha=0.6, **ptr):
    p = dict(rgb=FAKE, seg=FAKE, lut=FAKE, out=FAKE_OUT)
    p.update(ptr)
    return L.rgbd_overlay_blend(p["rgb"], p["seg"], dtype, p["lut"], B, H, W, n_ids, alpha, p["out"], NULL)


def test_symbols_exported_and_bound():
    L = _lib.lib()
    for n in ("rgbd_overlay_lut", "rgbd_overlay_blend"):
        assert hasattr(L, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES and n in _lib.header_symbols()
    assert I32 not in (F32, BF16)


@pytest.mark.parametrize("name", ["seg_id", "topk_idx", "palette", "lut"])
def test_lut_null_pointer(name):
    assert _lut(_lib.lib(), **{name: NULL}) == E_ARG


@pytest.mark.parametrize("name", ["rgb", "seg", "lut", "out"])
def test_blend_null_pointer(name):
    assert _blend(_lib.lib(), **{name: NULL}) == E_ARG


def test_lut_sizes():
    L = _lib.lib()
    for bad in (dict(B=0), dict(B=-1), dict(Q=0), dict(Q=-2), dict(C=0), dict(C=-1), dict(n_colors=0),
                dict(n_colors=-4), dict(n_ids=0), dict(n_ids=-1), dict(color_by=2), dict(color_by=-1)):
        assert _lut(L, **bad) == E_ARG, bad
    assert _lut(L, B=1 << 16) == E_SHAPE              # one grid row per image
    assert _lut(L, B=1 << 12, n_ids=1 << 19) == E_SHAPE  # B n_ids = 2^31


def test_blend_sizes_dtype_and_aliasing():
    L = _lib.lib()
    for bad in (dict(B=0), dict(B=-1), dict(H=0), dict(H=-7), dict(W=0), dict(W=-1), dict(n_ids=0), dict(n_ids=-3),
                dict(alpha=float("nan")), dict(alpha=float("inf"))):
        assert _blend(L, **bad) == E_ARG, bad
    for bad in (BF16, 3, 7, -1):
        assert _blend(L, dtype=bad) == E_DTYPE, bad
    assert _blend(L, B=1 << 10, H=1 << 14, W=1 << 13) == E_SHAPE   # 2^37 pixels
    assert _blend(L, B=1 << 12, n_ids=1 << 19) == E_SHAPE
    # out may not overlap rgb (B H W 3 = 90 bytes here): equal, and off by less than the image
    assert _blend(L, out=FAKE) == E_ARG
    assert _blend(L, out=ctypes.c_void_p(FAKE.value + 89)) == E_ARG
    assert _blend(L, out=ctypes.c_void_p(FAKE.value - 89)) == E_ARG
    assert _blend(L, lut=ctypes.c_void_p(FAKE.value + 2)) == E_ARG  # the table is int32-aligned


def test_cpu_and_non_contiguous_tensors_are_refused():
    import torch
    from rgbd_amd import overlay
    img = torch.zeros(4, 6, 3, dtype=torch.uint8)
    res = {"segmentation": torch.zeros(4, 6), "segments_info": [{"id": 0}]}
    with pytest.raises(RuntimeError, match="GPU only"):
        overlay.overlay_segments(img, res, {0: (1, 2, 3)})
    with pytest.raises(RuntimeError, match="GPU only"):
        overlay.blend(img[None], res["segmentation"][None], torch.zeros(1, 1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="GPU only"):
        overlay.build_lut(torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 4, dtype=torch.int32), 5, [(1, 2, 3)])
