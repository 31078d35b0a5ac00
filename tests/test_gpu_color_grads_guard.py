"""rgbd_color_grads writes nothing outside ``out`` (tests/checkers/guard.py: the outputs the
wrapper allocates and the inputs sit between 0xFF guard bands, which read as NaN), and the guarded
run gives the torch statement's bits -- so no output element is left unwritten and no guard value
is read."""
import pytest
import torch

from checkers import color_grad_cases as cc, guard

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("table", sorted(cc.TABLES))
@pytest.mark.parametrize("g_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("layout", ["nchw_f32", "nhwc_bf16", "nhwc_f32", "mixed"])
def test_color_grads_stay_inside_their_buffers(table, g_dtype, layout):
    from rgbd_amd import ops
    dev = torch.device("cuda", 0)
    shapes = cc.TABLES[table]
    lays = (["nhwc_bf16", "nchw_f32", "nhwc_f32", "none"] if layout == "mixed" else [layout] * 4)[:len(shapes)]
    Gs, Ds, nhwc = cc.make_jobs(shapes, g_dtype, lays, dev, seed=5)
    with guard.guarded_allocations() as sw:
        got = ops.color_grads([sw.place(g, "G") for g in Gs], [None if d is None else sw.place(d, "D") for d in Ds],
                              nhwc=nhwc)
        n = sw.check_all()
        assert sw.passed_through == 0 and not sw.workspaces()
    assert n == 2 * len(shapes) + sum(d is not None for d in Ds)  # G, out and D of every job
    for i, (a, b) in enumerate(zip(got, cc.expected(Gs, Ds, nhwc))):
        assert a.dtype == b.dtype and torch.equal(a, b), f"job {i} differs"
