"""C-ABI checks of rgbd_color_grads that run without a GPU: the symbol is exported and bound, and
every documented return code comes back from the host-side validation before anything is launched
(the pointers handed in are never dereferenced; without a device a launch would answer with a
HIP error, so RGBD_OK here also shows that nothing was launched)."""
import ctypes

import pytest

from rgbd_amd import _lib, ops

FAKE, FAKE2, FAKE3 = 0x1000, 0x2000, 0x3000
F32, BF16 = _lib.RGBD_F32, _lib.RGBD_BF16
OK, E_ARG, E_SHAPE, E_DTYPE = 0, -1, -2, -3


def _job(g=FAKE, d=FAKE2, out=FAKE3, B=2, C=16, H=3, W=5, g_dtype=F32, d_dtype=BF16, d_nhwc=1):
    return ops._ColorGradJob(g, d, out, B, C, H, W, g_dtype, d_dtype, d_nhwc)


def _call(jobs, n=None):
    arr = (ops._ColorGradJob * max(len(jobs), 1))(*jobs)
    return _lib.lib().rgbd_color_grads(len(jobs) if n is None else n, arr, None)


EMPTY = dict(B=0)  # a job that describes no work: validated, never launched


def test_symbol_exported_and_bound():
    assert hasattr(_lib.lib(), "rgbd_color_grads")
    assert "rgbd_color_grads" in _lib.SIGNATURES and "rgbd_color_grads" in _lib.header_symbols()
    assert ctypes.sizeof(ops._ColorGradJob) == 3 * 8 + 7 * 4 + 4  # three pointers, seven ints, tail padding


@pytest.mark.parametrize("n", [0, 5, -1])
def test_job_count_out_of_range(n):
    assert _call([_job(**EMPTY)] * 5, n=n) == E_ARG


def test_null_job_table():
    assert _lib.lib().rgbd_color_grads(1, None, None) == E_ARG


@pytest.mark.parametrize("name", ["g", "out"])
def test_null_pointer(name):
    assert _call([_job(**{name: None})]) == E_ARG
    assert _call([_job(**EMPTY), _job(**{name: None}, **EMPTY)]) == E_ARG  # checked for every job, work or not


@pytest.mark.parametrize("name", ["B", "C", "H", "W"])
def test_negative_size(name):
    assert _call([_job(**{name: -1})]) == E_ARG


def test_nhwc_source_needs_channels_in_eights():
    assert _call([_job(C=12)]) == E_SHAPE
    assert _call([_job(C=12, d_dtype=F32)]) == E_SHAPE
    assert _call([_job(**EMPTY), _job(C=12)]) == E_SHAPE
    # an NCHW source or none is flat: any C (no work here, so no launch)
    assert _call([_job(C=12, d_nhwc=0, B=0)]) == OK
    assert _call([_job(C=12, d=None, B=0)]) == OK


def test_sizes_past_2_31():
    assert _call([_job(B=1 << 12, C=1 << 9, H=1 << 5, W=1 << 5)]) == E_SHAPE  # B C H W = 2^31
    assert _call([_job(B=1, C=8, H=1 << 16, W=1 << 15)]) == E_SHAPE           # H W = 2^31
    assert _call([_job(B=1 << 16, C=1 << 15, H=1, W=1, d=None)]) == E_SHAPE


@pytest.mark.parametrize("bad", [7, -1, 2])
def test_bad_dtype_code(bad):
    assert _call([_job(g_dtype=bad)]) == E_DTYPE
    assert _call([_job(d_dtype=bad)]) == E_DTYPE
    assert _call([_job(d_dtype=bad, **EMPTY)]) == E_DTYPE
    assert _call([_job(d_dtype=bad, d=None, **EMPTY)]) == OK  # no D: its dtype code is not read


@pytest.mark.parametrize("empty", [dict(B=0), dict(C=0), dict(H=0), dict(W=0)])
def test_no_work_is_ok_without_a_launch(empty):
    assert _call([_job(**empty)]) == OK
    assert _call([_job(**empty)] * 4) == OK
    assert _call([_job(d=None, **empty), _job(d_nhwc=0, d_dtype=F32, **empty)]) == OK


def test_cpu_tensors_are_refused():
    import torch
    g = torch.zeros(1, 8, 2, 2)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.color_grads([g], [None])
    with pytest.raises(ValueError):
        ops.color_grads([], [])
    with pytest.raises(ValueError):
        ops.color_grads([g] * 5, [None] * 5)
