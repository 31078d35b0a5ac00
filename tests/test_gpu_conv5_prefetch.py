"""conv5's item-to-item hand-offs in the rebuilt step loop (k_rp_conv5_v4: fragments streamed
column by column, copies from scalar bases, tile origins once per item): the contract and
tolerance of tests/test_gpu_conv5.py — pooled features (`rgbd_ratio_pooled_offset`) against
float64 arithmetic on the same bf16 gated features and bf16-rounded weights, rtol 2e-4 / atol 1e-5
of the largest pooled value — at the smallest shapes that exercise those hand-offs:

* a 256-CU card runs 128 workgroup pairs, so with more than 128 tiles of 16x32 px some pairs run
  two items and others one: the last steps of an item copy the next item's quarter 0 and step-0
  weights from the next tile's origin across the epilogue (`has_next` true) or copy nothing
  (`has_next` false).  Train (2, 160, 288): 180 tiles, MODE 0, generic pool.  Eval (2, 160, 320):
  200 tiles, MODE 1 (bin sums in the epilogue).  Eval (2, 160, 288): MODE 2.
* ragged (3, 90, 125), train and eval; (1, 64, 96): every pair runs at most one item.

In the train cases feature_extractor.1's updated running mean and variance are checked against
float64 batch moments of the same conv outputs, with the bound of tests/test_gpu_ratio_train.py
(2e-6 (1 + max|want|)): the statistics are summed from the float32 accumulators in the epilogue.
The test runs the product kernel only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_inputs as gi
from checkers import ratio_ws
from rgbd_amd import init as winit

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRE = "model.pixel_level_module.ratio_predictor."
MOMENTUM = 0.1


def tol32(ref):
    """float32 kernel against float64 arithmetic on the same input (tests/test_gpu_ratio_train.py)."""
    return 2e-6 * (1.0 + float(ref.abs().max()))


@pytest.mark.parametrize("B,H,W,training", [
    (2, 160, 288, True), (2, 160, 320, False), (2, 160, 288, False),
    (3, 90, 125, True), (3, 90, 125, False), (1, 64, 96, True), (1, 64, 96, False)])
def test_conv5_prefetch_bn_relu_pool(B, H, W, training):
    from rgbd_amd import _lib, ops
    from rgbd_amd.modules import EnhancedDepthImageRatioPredictor
    pv = gi.pixel_values(21, B, H, W)
    m = EnhancedDepthImageRatioPredictor(3)
    winit.init_deterministic(m, prefix=PRE)
    m.compute_dtype = torch.bfloat16
    fe = m.feature_extractor
    bn = fe[1]
    # distinct running statistics, so that eval mode's affine is not the identity
    g = torch.Generator().manual_seed(5)
    bn.running_mean.copy_(torch.randn(256, generator=g) * 0.05)
    bn.running_var.copy_(torch.rand(256, generator=g) * 0.5 + 0.5)
    run_mean, run_var = bn.running_mean.clone().double(), bn.running_var.clone().double()
    m = m.to(DEV).train(training)
    x = torch.from_numpy(pv).to(DEV)[:, 3:6]
    with torch.no_grad():
        m(x)
    torch.cuda.synchronize()
    L = _lib.lib()
    ws = ops._workspace(x.device, L.rgbd_ratio_workspace_size(1, B, H, W), "ratio")
    off = L.rgbd_ratio_features_offset(1, B, H, W)
    assert ratio_ws.ratio_pad_is_zero(ws, off, B, H, W)  # conv5's halo reads zeros outside the image
    xin = ratio_ws.ratio_features_bf16(ws, off, B, H, W).double().cpu()
    poff = L.rgbd_ratio_pooled_offset(1, B, H, W)
    got = ws[poff:poff + B * 256 * 16 * 4].view(torch.float32).reshape(B, 256, 4, 4).double().cpu()

    conv = fe[0]
    w5 = conv.weight.detach().cpu().to(torch.bfloat16).double()
    yf = F.conv2d(xin, w5, conv.bias.detach().cpu().double(), padding=1)
    bmean, bvar = yf.mean((0, 2, 3)), yf.var((0, 2, 3), unbiased=False)
    if training:
        mean, var = bmean.float(), bvar.float()
    else:
        mean, var = run_mean.float(), run_var.float()
    gamma, beta = bn.weight.detach().cpu().float(), bn.bias.detach().cpu().float()
    sc = gamma / torch.sqrt(var + 1e-5)
    sh = beta - mean * sc
    yb = yf.float().to(torch.bfloat16).float()
    z = torch.clamp_min(yb * sc[None, :, None, None] + sh[None, :, None, None], 0.0)
    ref = F.adaptive_avg_pool2d(z.double(), 4)
    scale = float(ref.abs().max())
    assert scale > 1e-3
    d = (got - ref).abs()
    bad = d > 2e-4 * ref.abs() + 1e-5 * scale
    print(f"{B}x{H}x{W} train={training}: max |d| {float(d.max()):.3g} (scale {scale:.3g}), {int(bad.sum())} bad")
    assert not bool(bad.any()), (float(d.max()), scale, np.argwhere(bad.numpy())[:5].tolist())

    got_rm, got_rv = bn.running_mean.detach().double().cpu(), bn.running_var.detach().double().cpu()
    if training:
        n = B * H * W
        want_rm = (1 - MOMENTUM) * run_mean + MOMENTUM * bmean
        want_rv = (1 - MOMENTUM) * run_var + MOMENTUM * bvar * n / (n - 1)
        e_rm, e_rv = float((got_rm - want_rm).abs().max()), float((got_rv - want_rv).abs().max())
        print(f"  running_mean max|d| {e_rm:.3g} (tol {tol32(want_rm):.3g}), running_var max|d| {e_rv:.3g} "
              f"(tol {tol32(want_rv):.3g})")
        assert e_rm <= tol32(want_rm)
        assert e_rv <= tol32(want_rv)
    else:
        assert torch.equal(got_rm, run_mean) and torch.equal(got_rv, run_var)
