"""f2 training path: HipSwinLayer with gradients (rgbd_amd/swin.py: QKVFunction,
WindowAttentionFunction over rgbd_swin_window_attn_bwd, dense.LinearResidualFunction,
dense.GeluFFNFunction) against the Hugging Face layer and backbone with the same weights.

Three arms on the same inputs: HF in float64 (the truth), HF in the precision under test, HIP in
that precision.  For the output, the input gradient and every parameter gradient the error is the
max-abs difference from the truth relative to the truth's max (the max floored at 1e-3 as ``rel``
of tests/test_gpu_masked_attention.py floors it: the k bias of an unpadded map has a gradient that
is zero but for rounding, the softmax being invariant to it).  The HIP arm's error must be at
most 1.5 x the HF arm's + a slack: 1e-5 in float32 and 1e-3 under bf16 autocast, the two project
bars of tests/test_gpu_masked_attention.py (test_core_forward_backward_vs_float64 and
test_module_bf16_autocast_vs_torch).  The HF bf16 arm is asserted finite (inputs are
randn, tables normal(0, 0.5), as tests/test_gpu_swin.py; it is finite on an MI355X at these sizes).

Measured on an MI355X, worst HIP error / (1.5 x HF error + slack): float32 0.88 (k_proj.bias of the
dim 384 layer, 14x14, shift 3: hip 6.7e-4, hf 5.0e-4 of a gradient that is zero but for rounding),
bf16 autocast 0.86 (a stage-3 q_proj.bias of the backbone: hip 1.9e-2, hf 1.4e-2)."""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
STAGES = [(96, 3), (192, 6), (384, 12), (768, 24)]


def _rel(a, truth):
    return float((a.double() - truth).abs().max()) / max(float(truth.abs().max()), 1e-3)


def _tables(m):
    with torch.no_grad():  # non-trivial relative-position tables (HF initialises them to zero)
        for x in m.modules():
            if hasattr(x, "relative_position_bias_table"):
                x.relative_position_bias_table.normal_(0, 0.5)


def _arms(ref):
    """(HF float64, HF, HIP) sharing ref's weights."""
    from rgbd_amd import dense, swin
    hip = copy.deepcopy(ref)
    assert swin.install(hip) >= 1
    dense.install(hip)
    return copy.deepcopy(ref).double(), ref, hip


def _run(m, call, x, gout, amp, dtype=None):
    """forward + backward of ``call(m, x)``; returns [output, dx, parameter gradients...] and the names."""
    m.zero_grad(set_to_none=True)
    x = x.detach().to(dtype or x.dtype).requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        outs = call(m, x)
    loss = sum((o.double() * g.double()).sum() for o, g in zip(outs, gout))
    loss.backward()
    named = [(n, p.grad) for n, p in m.named_parameters()]
    return [torch.cat([o.detach().flatten() for o in outs]), x.grad] + [g for _, g in named], \
        ["output", "dx"] + [n for n, _ in named]


def _compare(truth, hf, hip, names, slack, tag):
    worst = (0.0, None)
    for t, a, b, n in zip(truth, hf, hip, names):
        assert (t is None) == (a is None) == (b is None), f"{tag} {n}: gradient present in some arms only"
        if t is None:
            continue
        assert torch.isfinite(a).all(), f"{tag} {n}: HF arm not finite"
        assert torch.isfinite(b).all(), f"{tag} {n}: HIP arm not finite"
        ea, eb = _rel(a, t), _rel(b, t)
        frac = eb / (1.5 * ea + slack)
        if frac > worst[0]:
            worst = (frac, f"{n}: hip {eb:.3g}, hf {ea:.3g}")
    print(f"{tag}: worst hip / (1.5 hf + {slack:g}) = {worst[0]:.3g} ({worst[1]})")
    assert worst[0] <= 1.0, f"{tag}: {worst[1]}"


@pytest.mark.parametrize("amp", [False, True], ids=["f32", "bf16_autocast"])
@pytest.mark.parametrize("dim,heads", STAGES, ids=[f"dim{d}" for d, _ in STAGES])
def test_swin_layer_forward_backward_vs_hf(dim, heads, amp):
    """Single SwinLayers of the four stage shapes, shift 0 and 3, on 8x10 (ragged: padded to 14x14)
    and 14x14 (no padding) maps, B = 2, called as the backbone calls them (always_partition)."""
    from transformers.models.swin.modeling_swin import SwinLayer
    from rgbd_amd.config import standard_config
    cfg = standard_config(48).backbone_config
    for shift in (0, 3):
        for (H, W) in ((8, 10), (14, 14)):
            torch.manual_seed(100 + dim + shift + H)
            ref = SwinLayer(cfg, dim, (H, W), heads, 0.0, shift).to(DEV).eval()
            _tables(ref)
            r64, ref, hip = _arms(ref)
            x = torch.randn((2, H * W, dim), device=DEV)
            gout = [torch.randn((2, H * W, dim), device=DEV)]

            def call(m, x):
                return [m(x, (H, W), always_partition=True)[0]]
            truth, names = _run(r64, call, x, gout, False, torch.float64)
            hf, _ = _run(ref, call, x, gout, amp)
            got, _ = _run(hip, call, x, gout, amp)
            _compare(truth, hf, got, names, 1e-3 if amp else 1e-5, f"dim {dim} shift {shift} {H}x{W}")


@functools.lru_cache(maxsize=None)
def _backbones():
    from transformers import SwinBackbone
    from rgbd_amd.config import standard_config
    torch.manual_seed(3)
    ref = SwinBackbone(standard_config(48).backbone_config).to(DEV).eval()
    _tables(ref)
    return _arms(ref)


def _features(m, x):
    return list(m(x).feature_maps)


@pytest.mark.parametrize("amp", [False, True], ids=["f32", "bf16_autocast"])
def test_swin_backbone_forward_backward_vs_hf(amp):
    """The SwinBackbone at 224x224, B = 1: the four feature maps, the image gradient and every
    parameter gradient (patch embedding, 12 layers, patch merging, output norms)."""
    r64, ref, hip = _backbones()
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn((1, 3, 224, 224), device=DEV, generator=g)
    with torch.no_grad():
        shapes = [f.shape for f in ref(x).feature_maps]
    gout = [torch.randn(s, device=DEV, generator=g) for s in shapes]
    truth, names = _run(r64, _features, x, gout, False, torch.float64)
    hf, _ = _run(ref, _features, x, gout, amp)
    got, _ = _run(hip, _features, x, gout, amp)
    _compare(truth, hf, got, names, 1e-3 if amp else 1e-5, "backbone 224x224")


def test_all_layers_take_the_kernels_with_gradients(monkeypatch):
    """With gradients enabled every one of the 12 layers reaches swin.window_attention (through
    WindowAttentionFunction) and its backward kernel; float32 forward results with gradients
    enabled equal the no_grad results bit for bit."""
    from rgbd_amd import swin
    _, _, hip = _backbones()
    fwd, bwd = [], []
    real_f, real_b = swin.window_attention, swin.window_attention_bwd

    def counted_f(qkv, bqkv, table, B, H, W, heads, shift, scale):
        fwd.append((H, W, heads, int(shift)))
        return real_f(qkv, bqkv, table, B, H, W, heads, shift, scale)

    def counted_b(qkv, bqkv, table, gout, B, H, W, heads, shift, scale):
        bwd.append((H, W, heads, int(shift)))
        return real_b(qkv, bqkv, table, gout, B, H, W, heads, shift, scale)
    monkeypatch.setattr(swin, "window_attention", counted_f)
    monkeypatch.setattr(swin, "window_attention_bwd", counted_b)
    x = torch.randn((1, 3, 224, 224), device=DEV)
    hip.zero_grad(set_to_none=True)
    feats = hip(x).feature_maps
    assert all(f.requires_grad for f in feats)
    assert len(fwd) == 12 and [c[3] for c in fwd] == [0, 3] * 6, fwd
    sum(f.sum() for f in feats).backward()
    assert sorted(bwd) == sorted(fwd), bwd
    with torch.no_grad():
        plain = hip(x).feature_maps
    assert len(fwd) == 24
    for k, (a, b) in enumerate(zip(feats, plain)):
        assert torch.equal(a.detach(), b), f"stage {k + 1}: the float32 forward differs with gradients enabled"


def test_rgb_baseline_trains_its_encoder():
    """version 0.0.0 (the RGB baseline, whose encoder is not detached) at 224x224: one loss backward
    leaves a finite, non-zero gradient on every encoder parameter.  In eval mode: with B = 1 an
    active DropPath drops a layer's whole attention branch, whose gradients are then zero by design."""
    from rgbd_amd import init as winit
    from rgbd_amd.config import standard_config
    from rgbd_amd.custom_model import CustomMask2FormerForUniversalSegmentation
    m = CustomMask2FormerForUniversalSegmentation(standard_config(48), version="0.0.0")
    winit.init_deterministic(m)
    m = m.to(DEV).eval()
    enc = m.model.pixel_level_module.encoder
    _tables(enc)
    g = torch.Generator(device=DEV).manual_seed(11)
    pv = torch.randn((1, 3, 224, 224), device=DEV, generator=g)
    out = m(pixel_values=pv)
    loss = out.masks_queries_logits.float().square().mean() + out.class_queries_logits.float().square().mean()
    loss.backward()
    # SwinBackbone never calls SwinModel's final ``swin.layernorm`` (it normalises the stage outputs
    # through hidden_states_norms): no gradient reaches it in HF either (the arms of
    # test_swin_backbone_forward_backward_vs_hf agree on which gradients are None)
    bad = [n for n, p in enc.named_parameters() if not n.startswith("swin.layernorm.")
           and (p.grad is None or not torch.isfinite(p.grad).all() or not p.grad.any())]
    assert not bad, f"encoder parameters without a finite, non-zero gradient: {bad}"
