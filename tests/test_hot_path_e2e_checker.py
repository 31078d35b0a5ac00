"""The end-to-end checker (tests/checkers/hot_path_e2e.py) pinned to the oracle on the CPU: with
the oracle's own region codes its forward is oracle.hot_path.hot_path_forward
(custom_model.py:324-355), in float32 to a few ulps and in float64 to float32 rounding; and its
colour-map gradients are the closed form of the end-to-end arithmetic at scale 3, d c_3 = 2 G_3."""
import pytest
import torch

from checkers import hot_path_e2e as chk, hot_path_e2e_cases as cases
from oracle import hot_path as hot_o


@pytest.fixture(scope="module")
def mods():
    return cases.modules()


@pytest.mark.parametrize("case", range(len(cases.CASES)))
def test_checker_forward_is_the_oracle(case, mods):
    pv, ratios, colors, gouts, sizes = cases.inputs(case)
    sd32 = chk.state_dict_of(*mods, torch.float32)
    ref, _, decs = hot_o.hot_path_forward(colors, pv, sd32, ratios=ratios[:, None])
    codes, n_masks, _ = chk.oracle_codes(pv, ratios, sizes)
    assert n_masks == [d["n_masks"] for d in decs]
    got32 = chk.forward(colors, pv, codes, n_masks, sd32)
    got64 = chk.forward([c.double() for c in colors], pv.double(), codes, n_masks,
                        chk.state_dict_of(*mods, torch.float64))
    for k in range(4):
        scale = float(ref[k].abs().max())
        # same convolutions in another summation order (masks applied per bit, biases summed first)
        assert float((got32[k] - ref[k]).abs().max()) <= 1e-5 * scale, f"float32 feature {k}"
        assert float((got64[k] - ref[k].double()).abs().max()) <= 1e-5 * scale, f"float64 feature {k}"


def test_checker_colour_gradients_closed_form(mods):
    pv, ratios, colors, gouts, sizes = cases.inputs(0)
    codes, n_masks, _ = chk.oracle_codes(pv, ratios, sizes)
    _, dc = chk.color_grads(colors, gouts, pv, codes, n_masks, chk.state_dict_of(*mods, torch.float64))
    assert torch.equal(dc[3], 2 * gouts[3].double())
    for k in range(3):  # d c_k = 2 G_k + dX_k(d cp1_{k+1}): the cascade term is there and finite
        extra = dc[k] - 2 * gouts[k].double()
        assert torch.isfinite(extra).all() and float(extra.abs().max()) > 0


def test_end_to_end_mode_refuses_the_overlapped_reducer_hook(mods):
    """Data parallelism is not extended: the grad_hook groups hold the hot path's own parameters
    only, so the combination is refused before anything runs (not left silent)."""
    from rgbd_amd.hot_path import hot_path
    pv, ratios, colors, _, _ = cases.inputs(0)
    with pytest.raises(ValueError, match="grad_hook"):
        hot_path(pv, ratios, colors, *mods, grad_hook=lambda i, grads: None, color_grads=True)


def test_cases_find_three_modes():
    """The synthetic scenes of the case list all decompose into three modes (four masks)."""
    assert all(n == 3 for c in range(len(cases.CASES)) for n in cases.n_modes(c))
