"""The C ABI of the device RLE encoder (csrc/rle_encode.hip) without a GPU: the
symbols are declared, bound and exported, every refusal of the header comes back from the host
checks on dummy non-null pointers (nothing is launched), and the two pure queries are pure, 0 for
a non-positive size, monotone in every size and at least what the worst masks need."""
import ctypes
import itertools

import pytest

from rgbd_amd import _lib

NAMES = ["rgbd_rle_encode_chunk", "rgbd_rle_encode_capacity", "rgbd_rle_encode_workspace_size",
         "rgbd_rle_encode_labels", "rgbd_rle_encode_stack"]
ARG, SHAPE, DTYPE = -1, -2, -3
LABELS, STACK = 0, 1
FAKE = 0x10000  # non-null, 16-byte aligned, never dereferenced: every call below is refused on the host


def test_symbols_are_declared_bound_and_exported():
    L = _lib.lib()
    declared = _lib.header_symbols()
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(L, name), name
    chunk = L.rgbd_rle_encode_chunk()
    assert chunk > 0 and chunk % 256 == 0 and chunk == L.rgbd_rle_encode_chunk()


def _labels(L, dtype=_lib.RGBD_F32, maps=FAKE, B=2, H=24, W=40, n_ids=256, ids=FAKE, Q=5, cap_counts=100, cap_chars=100,
            chars=FAKE, offsets=FAKE, info=FAKE, totals=FAKE, ws=FAKE):
    return L.rgbd_rle_encode_labels(dtype, maps, B, H, W, n_ids, ids, Q, cap_counts, cap_chars, chars, offsets, info,
                                    totals, ws, None)


def _stack(L, masks=FAKE, N=3, h=24, w=40, cap_counts=100, cap_chars=100, chars=FAKE, offsets=FAKE, info=FAKE,
           totals=FAKE, ws=FAKE):
    return L.rgbd_rle_encode_stack(masks, N, h, w, cap_counts, cap_chars, chars, offsets, info, totals, ws, None)


def test_label_map_refusals():
    L = _lib.lib()
    for ptr in ("maps", "ids", "chars", "offsets", "info", "totals", "ws"):
        assert _labels(L, **{ptr: None}) == ARG, ptr
    for size in ("B", "H", "W", "Q"):
        for v in (0, -1):
            assert _labels(L, **{size: v}) == ARG, size
    assert _labels(L, cap_counts=-1) == ARG and _labels(L, cap_chars=-1) == ARG
    for n_ids in (0, -1, 257):
        assert _labels(L, n_ids=n_ids) == ARG, n_ids
    for dtype in (_lib.RGBD_BF16, 3, -1):
        assert _labels(L, dtype=dtype) == DTYPE, dtype
    assert _labels(L, H=1 << 16, W=1 << 15) == SHAPE          # H W = 2^31
    assert _labels(L, B=256, Q=256) == SHAPE                  # B Q = 65536
    assert _labels(L, B=65536, Q=65536) == SHAPE              # the product does not wrap into range
    assert _labels(L, ws=FAKE + 8) == ARG and _labels(L, totals=FAKE + 4) == ARG   # alignment


def test_stack_refusals():
    L = _lib.lib()
    for ptr in ("masks", "chars", "offsets", "info", "totals", "ws"):
        assert _stack(L, **{ptr: None}) == ARG, ptr
    for size in ("N", "h", "w"):
        for v in (0, -1):
            assert _stack(L, **{size: v}) == ARG, size
    assert _stack(L, cap_counts=-1) == ARG and _stack(L, cap_chars=-1) == ARG
    assert _stack(L, h=1 << 16, w=1 << 15) == SHAPE
    assert _stack(L, N=65536) == SHAPE


def _capacity(L, mode, n_images, n_masks, H, W):
    c, ch = ctypes.c_longlong(-7), ctypes.c_longlong(-7)
    assert L.rgbd_rle_encode_capacity(mode, n_images, n_masks, H, W, ctypes.byref(c), ctypes.byref(ch)) == 0
    return c.value, ch.value


def test_capacity_query():
    L = _lib.lib()
    c = ctypes.c_longlong()
    assert L.rgbd_rle_encode_capacity(STACK, 1, 1, 4, 4, None, ctypes.byref(c)) == ARG
    assert L.rgbd_rle_encode_capacity(STACK, 1, 1, 4, 4, ctypes.byref(c), None) == ARG
    assert L.rgbd_rle_encode_capacity(2, 1, 1, 4, 4, ctypes.byref(c), ctypes.byref(c)) == ARG
    for mode in (LABELS, STACK):
        assert _capacity(L, mode, 2, 6, 24, 40) == _capacity(L, mode, 2, 6, 24, 40)     # pure
        for k in range(4):
            for v in (0, -1):
                a = [2, 6, 24, 40]
                a[k] = v
                assert _capacity(L, mode, *a) == (0, 0), (mode, a)
        base = [2, 6, 23, 37]
        for k in range(4):                                                              # monotone
            prev = _capacity(L, mode, *base)
            for step in (1, 2, 7, 100):
                a = list(base)
                a[k] += step
                cur = _capacity(L, mode, *a)
                assert cur[0] >= prev[0] and cur[1] >= prev[1], (mode, a)
                prev = cur
    for h, w in ((24, 40), (23, 37), (97, 131), (128, 160), (480, 640)):
        L_ = h * w
        counts, chars = _capacity(L, STACK, 1, 1, h, w)
        assert counts >= L_ + 1 and chars >= L_ + 1            # the checkerboard: h w + 1 one-character counts
        counts3, chars3 = _capacity(L, STACK, 3, 3, h, w)
        assert counts3 >= 3 * (L_ + 1)
        # a two-id checkerboard map: both masks have about h w counts — the worst a label map can do
        counts, chars = _capacity(L, LABELS, 1, 2, h, w)
        assert counts >= 2 * L_ + 1 and chars >= counts
        # every count of a plane of h w cells fits the characters the bound allows per count
        per = chars // counts
        assert 2 ** (5 * per - 1) > L_


def test_workspace_size_query():
    L = _lib.lib()
    f = L.rgbd_rle_encode_workspace_size
    for mode in (LABELS, STACK):
        assert f(mode, 2, 6, 24, 40, 1000) == f(mode, 2, 6, 24, 40, 1000) > 0
        for k in range(4):
            for v in (0, -1):
                a = [2, 6, 24, 40]
                a[k] = v
                assert f(mode, *a, 1000) == 0, (mode, a)
        assert f(mode, 2, 6, 24, 40, -1) == 0 and f(mode, 2, 6, 24, 40, 0) > 0
        base = [2, 6, 23, 37, 1000]
        for k in range(5):
            prev = f(mode, *base)
            for step in (1, 2, 7, 100, 100000):
                a = list(base)
                a[k] += step
                cur = f(mode, *a)
                assert cur >= prev, (mode, a)
                prev = cur
        assert f(mode, 2, 6, 24, 40, 2000) - f(mode, 2, 6, 24, 40, 1000) >= 4000   # the run ends are 4 bytes each
    assert f(2, 2, 6, 24, 40, 1000) == 0


@pytest.mark.parametrize("mode,h,w", list(itertools.product((LABELS, STACK), (1, 97), (1, 43))))
def test_queries_at_small_planes(mode, h, w):
    L = _lib.lib()
    counts, chars = _capacity(L, mode, 1, 1, h, w)
    assert counts >= 2 and chars >= counts      # all-one: a 0 count and h w
    assert L.rgbd_rle_encode_workspace_size(mode, 1, 1, h, w, counts) >= 4 * counts
