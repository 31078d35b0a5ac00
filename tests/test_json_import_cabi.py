"""The C boundary of the RLE decoder (csrc/rle_decode.hip) without a device: the symbols, the
argument codes — every one returned by the host-side validation before any HIP call — and the
size query."""
import ctypes

import numpy as np
import pytest

from rgbd_amd import _lib

E_ARG, E_SHAPE = -1, -2
NAMES = ["rgbd_rle_chunk", "rgbd_rle_workspace_size", "rgbd_rle_counts", "rgbd_rle_paint", "rgbd_rle_stack"]


def _meta(strings_len, sizes, H, W, ranges=None, take=None):
    """The meta words of include/rgbd_hip.h for masks of ``sizes`` with strings of the given lengths."""
    N = len(sizes)
    resized = [i for i, s in enumerate(sizes) if tuple(s) != (H, W)]
    slot = np.full(N, -1, np.int32)
    slot[resized] = np.arange(len(resized))
    rz = np.full(N, -1, np.int32)
    rz[:len(resized)] = resized
    ranges = [0, N] if ranges is None else ranges
    return np.concatenate([np.concatenate([[0], np.cumsum(strings_len)]), np.array(sizes).reshape(-1),
                           np.ones(N) if take is None else take, slot, rz, ranges]).astype(np.int32)


class _Call:
    """rgbd_rle_paint / _counts / _stack on dummy non-null device pointers: validation must answer
    before anything is launched (there is no device here)."""

    def __init__(self):
        self.L = _lib.lib()
        self.buf = ctypes.create_string_buffer(4096)
        self.p = ctypes.c_void_p(ctypes.addressof(self.buf) + (-ctypes.addressof(self.buf)) % 256)

    def paint(self, meta, N, B, H, W):
        mh = meta.ctypes.data_as(ctypes.c_void_p)
        return self.L.rgbd_rle_paint(self.p, mh, self.p, N, B, H, W, self.p, self.p, self.p, None)

    def counts(self, meta, N, B, H, W):
        mh = meta.ctypes.data_as(ctypes.c_void_p)
        return self.L.rgbd_rle_counts(self.p, mh, self.p, N, B, H, W, self.p, self.p, None)

    def stack(self, meta, N, h, w):
        mh = meta.ctypes.data_as(ctypes.c_void_p)
        return self.L.rgbd_rle_stack(self.p, mh, self.p, N, h, w, self.p, self.p, self.p, None)


@pytest.fixture(scope="module")
def call():
    return _Call()


def test_symbols_are_exported_and_declared():
    L = _lib.lib()
    for n in NAMES:
        assert n in _lib.SIGNATURES and n in _lib.header_symbols() and hasattr(L, n)
    assert L.rgbd_rle_chunk() == 256


def test_negative_and_zero_sizes_are_refused(call):
    good = _meta([3, 4], [(24, 40), (24, 40)], 24, 40)
    for N, B, H, W in [(-1, 1, 24, 40), (0, 1, 24, 40), (2, 0, 24, 40), (2, -1, 24, 40), (2, 1, -24, 40),
                       (2, 1, 24, 0)]:
        assert call.paint(good, N, B, H, W) == E_ARG
        assert call.counts(good, N, B, H, W) == E_ARG
    assert call.stack(good, -2, 24, 40) == E_ARG and call.stack(good, 2, 24, -40) == E_ARG
    bad = _meta([3, 4], [(24, 40), (-24, 40)], 24, 40)
    assert call.paint(bad, 2, 1, 24, 40) == E_ARG and call.counts(bad, 2, 1, 24, 40) == E_ARG


def test_offsets_and_ranges_out_of_order_are_refused(call):
    m = _meta([3, 4], [(24, 40), (24, 40)], 24, 40)
    m[1], m[2] = 7, 3                       # offsets 0, 7, 3
    assert call.paint(m, 2, 1, 24, 40) == E_ARG and call.counts(m, 2, 1, 24, 40) == E_ARG
    assert call.stack(m, 2, 24, 40) == E_ARG
    m = _meta([3, 4], [(24, 40), (24, 40)], 24, 40)
    m[0] = 1                                # offsets must start at 0
    assert call.paint(m, 2, 1, 24, 40) == E_ARG
    m = _meta([3, 4, 5], [(24, 40)] * 3, 24, 40, ranges=[0, 2, 1, 3])
    assert call.paint(m, 3, 3, 24, 40) == E_ARG
    m = _meta([3, 4, 5], [(24, 40)] * 3, 24, 40, ranges=[0, 1, 2])  # does not end at N
    assert call.paint(m, 3, 2, 24, 40) == E_ARG
    m = _meta([3], [(24, 40)], 24, 40, take=[2])
    assert call.paint(m, 1, 1, 24, 40) == E_ARG


def test_slot_table_must_describe_the_resized_masks(call):
    m = _meta([3, 4], [(24, 40), (12, 20)], 24, 40)
    assert m[2 * 4 + 1:].tolist()[:4] == [-1, 0, 1, -1]
    m[2 * 4 + 1 + 1] = -1                   # mask 1 differs in size but names no slot
    assert call.paint(m, 2, 1, 24, 40) == E_ARG
    m = _meta([3, 4], [(24, 40), (12, 20)], 24, 40)
    assert call.stack(m, 2, 24, 40) == E_ARG  # stack mode: one size only


def test_pixel_counts_past_the_limit_are_refused(call):
    big = _meta([3], [(65536, 32768)], 65536, 32768)
    assert call.paint(big, 1, 1, 65536, 32768) == E_SHAPE and call.stack(big, 1, 65536, 32768) == E_SHAPE
    assert call.counts(big, 1, 1, 65536, 32768) == E_SHAPE
    m = _meta([3], [(65536, 32768)], 24, 40)   # one mask's own h w past it
    assert call.paint(m, 1, 1, 24, 40) == E_SHAPE
    ok = _meta([3], [(46340, 46340)], 46340, 46340)  # 46340^2 < 2^31: passes validation, so NULL chars decide
    L = _lib.lib()
    assert L.rgbd_rle_counts(None, ok.ctypes.data_as(ctypes.c_void_p), call.p, 1, 1, 46340, 46340, call.p, call.p,
                             None) == E_ARG


def test_null_pointers_are_refused(call):
    m = _meta([3], [(24, 40)], 24, 40)
    L = _lib.lib()
    assert L.rgbd_rle_paint(call.p, None, call.p, 1, 1, 24, 40, call.p, call.p, call.p, None) == E_ARG
    assert L.rgbd_rle_paint(call.p, m.ctypes.data_as(ctypes.c_void_p), call.p, 1, 1, 24, 40, call.p, call.p, None,
                            None) == E_ARG


def test_size_query_is_pure_and_monotone():
    L = _lib.lib()
    q = L.rgbd_rle_workspace_size
    assert q(0, 10, 0, 24, 40) == 0 and q(1, -1, 0, 24, 40) == 0 and q(1, 10, -1, 24, 40) == 0
    assert q(1, 10, 0, 0, 40) == 0 and q(1, 10, 0, 24, -1) == 0
    base = (4, 1000, 1, 24, 40)
    assert q(*base) == q(*base) == 4096 + 256  # 4 bytes per character, (H + W) ints per resized mask, 256-aligned
    for i, step in [(1, 1), (1, 5000), (2, 1), (2, 3), (3, 97), (4, 131)]:
        more = list(base)
        more[i] += step
        assert q(*more) >= q(*base)
    assert q(4, 2 ** 31 - 1, 0, 24, 40) >= 4 * (2 ** 31 - 1)
