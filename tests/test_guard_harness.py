"""The guard-band harness (tests/checkers/guard.py) reports what it is there to report.

The same classes run on CPU tensors here: a write one element past the end (made through the base
buffer, as a kernel's stray store would be), one element before the start, into a stride gap and
one full payload past the end is each reported with its side and payload-relative offsets; an
untouched buffer passes; the torch proxy guards nothing on the CPU; entering and leaving
``guarded_allocations()`` restores ``ops._ws_cache`` and every module's ``torch``.  So the GPU
sweeps of tests/test_gpu_guard_bands.py and tests/test_gpu_swin_window.py would fail on an overrun.
"""
import sys

import pytest
import torch

from checkers import guard


def _elem(g, index):
    """Element ``index`` (may be negative or past the end) of the payload's flat element space,
    addressed through the base buffer."""
    isz = g.payload.element_size()
    return g.base[g.off + index * isz: g.off + (index + 1) * isz]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8, torch.int64])
@pytest.mark.parametrize("shape", [(3, 5), (1,), (7, 33, 2), (70000,)])
def test_layout_and_untouched_buffer_passes(dtype, shape):
    g = guard.Guarded(shape, dtype, "cpu", tag="t")
    p = g.payload
    assert p.shape == shape and p.dtype == dtype and p.is_contiguous()
    assert p.data_ptr() % 256 == 0
    assert g.end - g.off == p.numel() * p.element_size()  # back guard: last payload byte + 1
    want = min(max(64 * 1024, g.nbytes), 1024 * 1024)
    assert g.off >= want and g.base.numel() - g.end >= want
    assert bool((g.base == 0xFF).all())  # payload poisoned too: NaN in float32 / bf16
    if dtype in (torch.float32, torch.bfloat16):
        assert bool(torch.isnan(p).all())
    g.check()
    p.copy_(torch.arange(p.numel()).reshape(shape).to(dtype))  # writing the whole payload is fine
    g.check()
    assert g.report() is None and int(g.touched()) == 0


def test_zeros_request_zeroes_only_the_payload():
    g = guard.Guarded((4, 6), torch.float32, "cpu", zero=True)
    assert bool((g.payload == 0).all())
    assert bool((g.base[:g.off] == 0xFF).all()) and bool((g.base[g.end:] == 0xFF).all())
    g.check()


def test_guard_size_caps_at_one_mib():
    g = guard.Guarded((3 << 20,), torch.uint8, "cpu")
    assert 1 << 20 <= g.off < (1 << 20) + 256 and g.base.numel() - g.end >= 1 << 20


def test_one_element_past_the_end_is_reported():
    g = guard.Guarded((3, 5), torch.float32, "cpu", tag="out")
    _elem(g, 15).view(torch.float32)[0] = 1.5
    with pytest.raises(AssertionError) as e:
        g.check()
    msg = str(e.value)
    assert "'out'" in msg and "back guard" in msg and "front guard" not in msg
    # 1.5f = 00 00 C0 3F little-endian: four bytes changed, offsets 60..63 from the payload start
    assert "4 bytes touched" in msg and "60..63" in msg


def test_one_element_before_the_start_is_reported():
    g = guard.Guarded((8,), torch.bfloat16, "cpu", tag="ws")
    _elem(g, -1).view(torch.bfloat16)[0] = 1.0
    with pytest.raises(AssertionError, match=r"front guard: 2 bytes touched, payload-relative offsets -2\.\.-1"):
        g.check()


def test_store_of_the_fill_pattern_itself_is_the_only_blind_spot():
    g = guard.Guarded((8,), torch.uint8, "cpu")
    g.base[g.end] = 0xFF
    g.check()
    g.base[g.end] = 0xFE
    assert int(g.touched()) == 1


def test_write_into_a_stride_gap_is_reported():
    g = guard.strided(4, 6, 8, torch.float32, "cpu", zero=True, tag="ldc")
    p = g.payload
    assert p.shape == (4, 6) and p.stride() == (8, 1) and p.data_ptr() % 256 == 0
    assert g.nbytes == (3 * 8 + 6) * 4  # the last row ends the payload: the back guard follows it
    p.fill_(2.0)  # every payload cell: still clean
    g.check()
    _elem(g, 1 * 8 + 6).view(torch.float32)[0] = 0.0  # row 1, first gap column
    with pytest.raises(AssertionError) as e:
        g.check()
    assert "stride gap: 4 bytes touched, payload-relative offsets 56..59" in str(e.value)
    # the trailing gap of the last row is back guard
    g2 = guard.strided(4, 6, 8, torch.float32, "cpu")
    _elem(g2, 3 * 8 + 6).view(torch.float32)[0] = 0.0
    with pytest.raises(AssertionError, match="back guard"):
        g2.check()


def test_batched_stride_gap_is_guard():
    """[batch][M][N] at strides (sc, ldc, 1) with sc > M * ldc: the rows between batches are guard."""
    g = guard.Guarded((2, 3, 4), torch.float32, "cpu", zero=True, strides=(20, 5, 1))
    g.check()
    _elem(g, 3 * 5).view(torch.float32)[0] = 0.0  # the row after batch 0's last
    with pytest.raises(AssertionError, match="stride gap"):
        g.check()


def test_write_one_full_payload_past_the_end_is_reported():
    """Off by a whole buffer (a wrong batch or tile stride): the guard is as large as the payload."""
    for n in (10, 100000):
        g = guard.Guarded((n,), torch.float32, "cpu", tag="far")
        _elem(g, 2 * n - 1).view(torch.float32)[0] = 0.0
        with pytest.raises(AssertionError, match="back guard"):
            g.check()
        g = guard.Guarded((n,), torch.float32, "cpu", tag="far")
        _elem(g, -n).view(torch.float32)[0] = 0.0
        with pytest.raises(AssertionError, match="front guard"):
            g.check()


def test_pool_check_all_names_every_touched_buffer_and_place_copies():
    pool = guard.Pool()
    a = pool.new((5,), torch.float32, "cpu", tag="a")
    b = pool.new((5,), torch.float32, "cpu", tag="b")
    src = torch.arange(12.0).reshape(3, 4)
    c = pool.place(src, tag="in")
    assert torch.equal(c, src) and c.data_ptr() != src.data_ptr()
    d = pool.place(src[:, 1:3], tag="in_strided")  # strides kept, gap columns guarded
    assert d.stride() == (4, 1) and torch.equal(d, src[:, 1:3])
    assert pool.check_all() == 4
    b.base[b.end + 7] = 0
    a.base[a.off - 1] = 0
    with pytest.raises(AssertionError) as e:
        pool.check_all()
    assert "2 of 4 guarded buffers touched" in str(e.value) and "'a'" in str(e.value) and "'b'" in str(e.value)


def test_proxy_returns_plain_tensors_for_cpu_requests():
    pool = guard.Pool()
    px = guard.TorchProxy(pool)
    assert px.float32 is torch.float32 and px.nn is torch.nn and px.Tensor is torch.Tensor
    src = torch.ones((2, 3))
    outs = [px.empty((2, 3)), px.zeros(4, dtype=torch.int32), px.zeros((2,), device="cpu"), px.ones((3,)),
            px.full((2, 2), 7.0), px.full((2,), fill_value=3, dtype=torch.int64, device=torch.device("cpu")),
            px.empty_like(src), px.zeros_like(src), px.empty(0, dtype=torch.bfloat16)]
    assert not pool.bufs and pool.passed_through == 0
    assert all(isinstance(t, torch.Tensor) and t.device.type == "cpu" for t in outs)
    assert float(outs[4].sum()) == 28.0 and int(outs[5].sum()) == 6 and float(outs[7].abs().sum()) == 0.0


def test_proxy_guards_what_it_is_asked_to(monkeypatch):
    """The GPU branch, exercised on the CPU by declaring every device a GPU: shapes, dtypes, fills
    and the dense non-contiguous layouts of the *_like factories come out as torch's would."""
    monkeypatch.setattr(guard, "_is_gpu", lambda device: True)
    pool = guard.Pool()
    px = guard.TorchProxy(pool)
    dev = torch.device("cpu")
    e = px.empty((3, 4), dtype=torch.bfloat16, device=dev)
    z = px.zeros(5, dtype=torch.int64, device=dev)
    z2 = px.zeros((), dtype=torch.float32, device=dev)
    o = px.ones((2, 2), device=dev)
    f = px.full((2, 3), fill_value=48, dtype=torch.int64, device=dev)
    cl = torch.zeros((2, 8, 3, 5)).to(memory_format=torch.channels_last)
    like = px.empty_like(cl)
    zl = px.zeros_like(torch.ones((4, 2), dtype=torch.bfloat16), memory_format=torch.preserve_format)
    assert len(pool.bufs) == 7 and pool.passed_through == 0
    assert e.shape == (3, 4) and e.dtype == torch.bfloat16 and e.is_contiguous() and not e._is_view()
    assert z.tolist() == [0] * 5 and float(z2) == 0.0 and o.tolist() == [[1.0, 1.0], [1.0, 1.0]]
    assert f.dtype == torch.int64 and f.tolist() == [[48] * 3] * 2
    assert like.shape == cl.shape and like.stride() == cl.stride()
    assert zl.dtype == torch.bfloat16 and float(zl.abs().sum()) == 0.0
    assert "test_guard_harness.py" in pool.bufs[0].tag  # the caller's file and line
    assert pool.check_all() == 7
    pool.bufs[3].base[pool.bufs[3].end] = 0
    with pytest.raises(AssertionError, match="back guard"):
        pool.check_all()


def test_context_swaps_and_restores_torch_and_workspace_cache():
    from rgbd_amd import dense, ops, point_loss, swin  # noqa: F401
    mods = [m for n, m in sys.modules.items() if n.startswith("rgbd_amd.") and m.__dict__.get("torch") is torch]
    assert len(mods) >= 4
    cache, zeroed = ops._ws_cache, ops._ws_zeroed
    marker = ("marker",)
    cache[marker] = torch.zeros(1)
    zeroed.add(marker)
    retired = len(ops._ws_retired)
    try:
        with guard.guarded_allocations() as sweep:
            assert all(isinstance(m.torch, guard.TorchProxy) for m in mods)
            assert ops._ws_cache == {} and ops._ws_cache is not cache
            assert ops._ws_zeroed == set() and ops._ws_zeroed is not zeroed
            assert dense.torch.float32 is torch.float32
            # a CPU request made by package code passes through
            assert ops.torch.zeros((2,)).device.type == "cpu" and not sweep.bufs
            ops._ws_cache[("k",)] = torch.zeros(3)  # what _workspace would have stored
        assert all(m.torch is torch for m in mods)
        assert ops._ws_cache is cache and ops._ws_zeroed is zeroed and marker in cache and marker in zeroed
        assert len(ops._ws_retired) == retired + 1  # retired, never freed
        assert sweep.check_all() == 0
        with pytest.raises(RuntimeError):
            with guard.guarded_allocations():
                raise RuntimeError("restored on error too")
        assert all(m.torch is torch for m in mods) and ops._ws_cache is cache
    finally:
        cache.pop(marker, None)
        zeroed.discard(marker)
        del ops._ws_retired[retired:]
