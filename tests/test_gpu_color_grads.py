"""rgbd_color_grads (the end-to-end mode's colour-gradient launch) against its torch statement,
bit for bit: every D layout with both G dtypes, D absent, the two four-job tables (ragged pixel
counts; the 16-byte path), a single odd job, and misaligned pointers (the element-wise fallback)."""
import pytest
import torch

import _rgbd_import  # noqa: F401
from rgbd_amd import ops
from checkers import color_grad_cases as cc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _check(Gs, Ds, nhwc, outs):
    want = cc.expected(Gs, Ds, nhwc)
    assert len(outs) == len(want)
    for i, (a, b) in enumerate(zip(outs, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.is_contiguous()
        assert torch.equal(a, b), f"job {i}: {int((a != b).sum())} of {a.numel()} elements differ"


@pytest.mark.parametrize("table", sorted(cc.TABLES))
@pytest.mark.parametrize("g_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("layout", ["nchw_f32", "nhwc_bf16", "nhwc_f32"])
def test_every_layout_and_dtype(table, g_dtype, layout):
    shapes = cc.TABLES[table]
    Gs, Ds, nhwc = cc.make_jobs(shapes, g_dtype, [layout] * len(shapes), DEV, seed=1)
    _check(Gs, Ds, nhwc, ops.color_grads(Gs, Ds, nhwc=nhwc))


@pytest.mark.parametrize("table", ["ragged", "aligned"])
@pytest.mark.parametrize("g_dtype", [torch.float32, torch.bfloat16])
def test_null_d_on_any_job(table, g_dtype):
    """D absent (out = G + G) in each position of a mixed table, and on all jobs at once."""
    shapes = cc.TABLES[table]
    base = ["nhwc_bf16", "nchw_f32", "nhwc_f32", "nhwc_bf16"]
    for lays in [base[:i] + ["none"] + base[i + 1:] for i in range(4)] + [["none"] * 4]:
        Gs, Ds, nhwc = cc.make_jobs(shapes, g_dtype, lays, DEV, seed=2)
        _check(Gs, Ds, nhwc, ops.color_grads(Gs, Ds, nhwc=nhwc))


def test_hot_path_tables():
    """The tables the hot path's three modes issue: scales 0-2 from the cascade, scale 3 doubled."""
    for g_dtype, lay in [(torch.float32, "nchw_f32"), (torch.bfloat16, "nhwc_bf16"), (torch.float32, "nhwc_bf16")]:
        for shapes in (cc.RAGGED, cc.ALIGNED):
            Gs, Ds, nhwc = cc.make_jobs(shapes, g_dtype, [lay] * 3 + ["none"], DEV, seed=3)
            _check(Gs, Ds, nhwc, ops.color_grads(Gs, Ds, nhwc=nhwc))


def _offset_view(t, off=1):
    """The values of ``t`` in a contiguous view that starts ``off`` elements into its storage."""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=t.device)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


@pytest.mark.parametrize("g_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("layout,which", [(lay, w) for lay in ["nchw_f32", "nhwc_bf16", "nhwc_f32", "none"]
                                          for w in ["g", "out", "d"] if (lay, w) != ("none", "d")])
def test_misaligned_pointer_takes_the_fallback_with_the_same_bits(g_dtype, layout, which):
    shapes = cc.ALIGNED[:2]  # sizes that take the 16-byte path when aligned
    Gs, Ds, nhwc = cc.make_jobs(shapes, g_dtype, [layout, layout], DEV, seed=4)
    outs = [torch.empty_like(g) for g in Gs]
    if which == "g":
        Gs[1] = _offset_view(Gs[1])
    elif which == "d":
        Ds[0] = _offset_view(Ds[0])
    else:
        outs[0] = _offset_view(outs[0])
    got = ops.color_grads(Gs, Ds, nhwc=nhwc, out=outs)
    assert all(a is b for a, b in zip(got, outs))
    _check(Gs, Ds, nhwc, got)
