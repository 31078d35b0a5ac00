"""The fused hot path's end-to-end mode (hot_path(..., color_grads=True)) in its
three precision modes: outputs and all 35 parameter gradients bitwise those of the default mode;
the four colour-map gradients against the float64 checker (tests/checkers/hot_path_e2e.py, a
restatement of custom_model.py:324-355 with the colour maps left in the graph) on the same
float32 master values and the device decomposition's region codes; and the default mode still
gives the colour maps no gradient (the reference's detach, custom_model.py:332-333, Q1).

Bars: float32 max-abs error / max-abs reference <= 1e-4 per tensor (the a4 row's bar for forward +
all gradients); both bf16 modes <= 3e-2 (BF16_REL of tests/test_gpu_parity.py)."""
import functools

import pytest
import torch

import _rgbd_import  # noqa: F401
from checkers import hot_path_e2e as chk, hot_path_e2e_cases as cases

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
F32_REL, BF16_REL = 1e-4, 3e-2
MODES = {"float32": (torch.float32, None), "bf16": (torch.bfloat16, None),
         "bf16_f32io": (torch.bfloat16, torch.float32)}


@functools.lru_cache(maxsize=None)
def _modules():
    dsams, dg = cases.modules()
    return [m.to(DEV) for m in dsams], dg.to(DEV)


@functools.lru_cache(maxsize=None)
def _reference(case):
    """float64 colour-map gradients for the case, computed once and shared (read-only)."""
    from rgbd_amd import ops
    pv, ratios, colors, gouts, sizes = cases.inputs(case)
    codes, info = ops.edsam_codes(ops.edsam_modes(pv.to(DEV)), ratios.to(DEV)[:, None], sizes)
    n_masks = [int(n) for n in ops.decode_info(info)["n_masks"]]
    dsams, dg = _modules()
    _, dc = chk.color_grads(colors, gouts, pv, [c.cpu() for c in codes], n_masks,
                            chk.state_dict_of(dsams, dg, torch.float64))
    return dc


def _params():
    dsams, dg = _modules()
    return [p for m in dsams for p in m.parameters()] + list(dg.parameters())


def _run(case, mode, color_grads, prepared_with=None):
    """One forward + backward -> (outputs, parameter gradients, colour-map gradients)."""
    from rgbd_amd import hot_path as hp
    dtype, interface = MODES[mode]
    pv, ratios, colors, gouts, _ = cases.inputs(case)
    dsams, dg = _modules()
    params = _params()
    assert len(params) == 35
    for p in params:
        p.grad = None
    pv, ratios = pv.to(DEV), ratios.to(DEV)[:, None]
    cols = [c.to(DEV).requires_grad_(True) for c in colors]
    prep = None
    if prepared_with is not None:
        prep = hp.prepare(pv, cols, dtype, dsam_modules=dsams, interface_dtype=interface, color_grads=prepared_with)
    outs = hp.hot_path(pv, ratios, cols, dsams, dg, dtype=dtype, check_status=True, interface_dtype=interface,
                       prepared=prep, color_grads=color_grads)
    torch.autograd.backward(outs, [g.to(DEV).to(o.dtype) for g, o in zip(gouts, outs)])
    torch.cuda.synchronize()
    return [o.detach() for o in outs], [p.grad.clone() for p in params], [c.grad for c in cols]


def _rel(a, e):
    return float((a.double().cpu() - e).abs().max() / e.abs().max())


@pytest.mark.parametrize("case", range(len(cases.CASES)))
@pytest.mark.parametrize("mode", list(MODES))
def test_end_to_end_mode(case, mode):
    outs0, pg0, cg0 = _run(case, mode, color_grads=False)
    # default mode: the colour maps require gradients and still receive none (Q1)
    assert all(g is None for g in cg0)
    outs1, pg1, cg1 = _run(case, mode, color_grads=True)
    # identical modes: the forward and the dW legs see the same operands
    for k, (a, b) in enumerate(zip(outs0, outs1)):
        assert a.dtype == b.dtype and torch.equal(a, b), f"feature {k}"
    for i, (a, b) in enumerate(zip(pg0, pg1)):
        assert torch.equal(a, b), f"parameter gradient {i}"
    # the colour-map gradients, in the colour maps' dtype
    ref = _reference(case)
    bar = F32_REL if mode == "float32" else BF16_REL
    errs = []
    for k in range(4):
        assert cg1[k] is not None and cg1[k].dtype == torch.float32 and cg1[k].shape == ref[k].shape
        assert torch.isfinite(cg1[k]).all()
        errs.append(_rel(cg1[k], ref[k]))
    print(f"e2e case {cases.CASES[case]} {mode}: colour-gradient errors " + " ".join(f"{e:.3g}" for e in errs)
          + f" (bar {bar:g}: fractions " + " ".join(f"{e / bar:.2g}" for e in errs) + ")")
    for k in range(4):
        assert errs[k] <= bar, f"d c_{k}: {errs[k]:.3g} > {bar:g}"


@pytest.mark.parametrize("mode", ["bf16", "bf16_f32io"])
@pytest.mark.parametrize("prepared_with", [False, True])
def test_prepared_without_dsam0_backward_filters_is_repacked(mode, prepared_with):
    """prepare() packs dsam0's backward filters only when told of the mode; a Prepared built
    without them is not reused as it is: the forward packs them, and the gradients are the bits
    of the run that prepared nothing."""
    _, pg, cg = _run(0, mode, color_grads=True)
    _, pg1, cg1 = _run(0, mode, color_grads=True, prepared_with=prepared_with)
    for a, b in zip(pg + cg, pg1 + cg1):
        assert torch.equal(a, b)


def test_only_some_colour_maps_require_gradients():
    """A colour map that does not require a gradient gets none; the others get the same bits."""
    from rgbd_amd import hot_path as hp
    _, _, cg = _run(1, "float32", color_grads=True)
    pv, ratios, colors, gouts, _ = cases.inputs(1)
    dsams, dg = _modules()
    cols = [c.to(DEV).requires_grad_(k in (1, 3)) for k, c in enumerate(colors)]
    outs = hp.hot_path(pv.to(DEV), ratios.to(DEV)[:, None], cols, dsams, dg, color_grads=True)
    torch.autograd.backward(outs, [g.to(DEV) for g in gouts])
    assert cols[0].grad is None and cols[2].grad is None
    assert torch.equal(cols[1].grad, cg[1]) and torch.equal(cols[3].grad, cg[3])
