"""The float64 restatement of Swin's window attention (tests/checkers/swin_window.py) pinned
against the installed transformers ``SwinLayer`` itself (CPU, no GPU needed).

The layer runs in double with ``o_proj`` the identity and ``always_partition=True`` (the window
stays 7 and the shift as given, also for maps smaller than a window, which is what the kernel
computes).  Forward hooks capture the output of ``layernorm_before`` and the input of
``layernorm_after``; the attention branch is that input minus the layer input, and q / k / v are
the three projections of the captured LayerNorm output on the original token layout.  Measured
over this grid: worst relative difference 5.5e-7 — HF's eager softmax runs in float32 even inside
a double layer.  Bar 5e-6.
"""
import pytest
import torch

from checkers.swin_window import window_attention_ref

SIZES = [(7, 7), (8, 10), (13, 7), (3, 16), (15, 20), (14, 21)]
SHIFTS = [0, 1, 3, 6]


def _hf_attention_branch(H, W, heads, shift, biases, B, seed):
    from transformers import SwinConfig
    from transformers.models.swin.modeling_swin import SwinLayer
    torch.manual_seed(seed)
    C = 32 * heads
    cfg = SwinConfig(window_size=7, qkv_bias=biases, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    cfg._attn_implementation = "eager"
    layer = SwinLayer(cfg, C, (H, W), heads, 0.0, shift).double().eval()
    attn = layer.attention
    with torch.no_grad():
        attn.relative_position_bias.relative_position_bias_table.normal_(0, 0.5)
        attn.o_proj.weight.copy_(torch.eye(C))
        attn.o_proj.bias.zero_()
        for p in (attn.q_proj, attn.k_proj, attn.v_proj):
            if p.bias is not None:
                p.bias.normal_(0, 0.5)
    got = {}
    h1 = layer.layernorm_before.register_forward_hook(lambda m, i, o: got.__setitem__("ln", o.detach()))
    h2 = layer.layernorm_after.register_forward_pre_hook(lambda m, i: got.__setitem__("res", i[0].detach()))
    x = torch.randn((B, H * W, C), dtype=torch.float64)
    with torch.no_grad():
        layer(x, (H, W), always_partition=True)
    h1.remove()
    h2.remove()
    assert int(layer.window_size) == 7 and int(layer.shift_size) == shift
    branch = (got["res"] - x).reshape(B * H * W, C)
    ln = got["ln"].reshape(B * H * W, C)
    with torch.no_grad():
        q, k, v = attn.q_proj(ln), attn.k_proj(ln), attn.v_proj(ln)
    bq, bk, bv = (p.bias.detach() if p.bias is not None else None for p in (attn.q_proj, attn.k_proj, attn.v_proj))
    table = attn.relative_position_bias.relative_position_bias_table.detach()
    return branch, (q, k, v, bq, bk, bv, table, B, H, W, heads, shift, attn.scaling)


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("biases", [True, False], ids=["biases", "no_biases"])
def test_restatement_matches_hf_swin_layer(heads, biases):
    worst = 0.0
    for n, (H, W) in enumerate(SIZES):
        for shift in SHIFTS:
            branch, args = _hf_attention_branch(H, W, heads, shift, biases, B=2, seed=100 * n + shift)
            ref = window_attention_ref(*args)
            assert ref.shape == branch.shape and ref.dtype == torch.float64
            err = float((ref - branch).abs().max() / branch.abs().max())
            worst = max(worst, err)
            assert err <= 5e-6, f"{H}x{W} shift {shift}: {err:.3g}"
    print(f"heads {heads}, biases {biases}: worst relative difference to HF SwinLayer {worst:.3g}")


def test_restatement_sees_shift_padding_and_biases():
    """The pin is not vacuous: dropping the shift mask, the bias rows of the padding or the
    relative-position table each moves the result by far more than the bar."""
    branch, args = _hf_attention_branch(8, 10, 3, 3, True, B=1, seed=5)
    q, k, v, bq, bk, bv, table, B, H, W, heads, shift, scale = args
    scale_ = float(branch.abs().max())
    for wrong in (window_attention_ref(q, k, v, bq, bk, bv, table, B, H, W, heads, 0, scale),
                  window_attention_ref(q, k, v, None, None, None, table, B, H, W, heads, shift, scale),
                  window_attention_ref(q, k, v, bq, bk, bv, table * 0, B, H, W, heads, shift, scale)):
        assert float((wrong - branch).abs().max()) / scale_ > 1e-2
