"""dX of dsam0 (96 -> 192, so the implicit GEMM has N = Cin = 96, half a column tile): the leg the
hot path's end-to-end mode adds to the cascade.  Reference path: the input gradient of
DSAModule.forward (custom_model.py:682-699),

    dx = gin + sum_{i<4} m_i * ConvT3x3s2(gy, W_i) + ConvT3x3s2(gy, W_proj),   m_i = bit i of code

bf16: the planned NHWC-only form the cascade uses equals the unplanned form and the NCHW form bit
for bit (what test_dsam_bf16_dx_nhwc_only_and_nhwc_bias_sums asserts for dsam1 / dsam2).
float32: against the statement above in float64, max-abs error over max-abs value <= 1e-4."""
import pytest
import torch
import torch.nn.functional as F

import _rgbd_import  # noqa: F401
from rgbd_amd import ops, synthetic

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
CIN, COUT, B = 96, 192, 2
F32_REL = 1e-4


def _case(H, W):
    h, w = (H + 3) // 4, (W + 3) // 4
    planes, _, _ = synthetic.make_batch(11, B, H, W)
    d3 = torch.from_numpy(planes[:, 3:6]).to(DEV)
    codes, info = ops.edsam_decompose(d3, torch.linspace(0.05, 0.45, B, device=DEV), [(h, w)])
    g = torch.Generator(device="cpu")
    g.manual_seed(H)
    ho, wo = (h + 1) // 2, (w + 1) // 2
    cw = (torch.randn((4, COUT, CIN, 3, 3), generator=g) * 0.03).to(DEV)
    pw = (torch.randn((COUT, CIN, 3, 3), generator=g) * 0.03).to(DEV)
    gy = (torch.randn((B, ho, wo, COUT), generator=g) * 0.1).to(DEV)   # NHWC
    gin = (torch.randn((B, CIN, h, w), generator=g) * 0.1).to(DEV)    # NCHW
    return codes[0], cw, pw, gy, gin


def _dx_f64(code, cw, pw, gy_nhwc, gin):
    code, cw, pw, gin = code.cpu().long(), cw.cpu().double(), pw.cpu().double(), gin.cpu().double()
    gy = gy_nhwc.cpu().double().permute(0, 3, 1, 2)
    h, w = code.shape[1:]
    pad = (h - (2 * gy.shape[2] - 1), w - (2 * gy.shape[3] - 1))

    def convt(wt):
        return F.conv_transpose2d(gy, wt, stride=2, padding=1, output_padding=pad)
    dx = gin + convt(pw)
    for i in range(4):
        dx = dx + ((code >> i) & 1).double()[:, None] * convt(cw[i])
    return dx


@pytest.mark.parametrize("H,W", [(52, 72), (64, 96)])  # maps 13 x 18 and 16 x 24
def test_dx0_bf16_planned_nhwc_only_equals_unplanned_and_nchw(H, W):
    code, cw, pw, gy, gin = _case(H, W)
    gy, gin = gy.bfloat16(), gin.bfloat16()
    _, wb = ops.dsam_pack(cw, pw, torch.bfloat16, code_mask=ops.dsam_code_masks([code])[0:1])
    gin_nhwc = ops.nchw_to_nhwc(gin)
    dx_ref, dx_ref_nhwc = ops.dsam_bwd_data(gy, code, wb, gin, want_nhwc=True)
    none, dx0 = ops.dsam_bwd_data(gy, code, wb, None, want_nhwc=True, want_nchw=False, gin_nhwc=gin_nhwc)
    # planned as the end-to-end step plans it: six conv legs at once, dsam0's dX the last
    other = torch.zeros((B, (code.shape[1] + 1) // 2, (code.shape[2] + 1) // 2), dtype=torch.uint8, device=DEV)
    plans = ops.dsam_plan([(ops.LEG_FWD, code, CIN, COUT), (ops.LEG_FWD, other, 192, 384),
                           (ops.LEG_DX, other, 192, 384), (ops.LEG_DX, code, CIN, COUT)])
    none2, dx1 = ops.dsam_bwd_data(gy, code, wb, None, want_nhwc=True, want_nchw=False, gin_nhwc=gin_nhwc,
                                   plan=plans[3])
    assert none is None and none2 is None
    assert tuple(dx1.shape) == (B, *code.shape[1:], CIN)
    assert torch.equal(dx1, dx0)
    assert torch.equal(dx1, dx_ref_nhwc)
    assert torch.equal(dx1, dx_ref.permute(0, 2, 3, 1))
    # and it is the gradient: bf16 operands with float32 accumulation against float64 on the same
    # gy / gin and the float32 filters, the bar of test_gpu_dsam_full.py (max error <= 2e-2 of the
    # reference's max magnitude)
    want = _dx_f64(code, cw, pw, gy, gin)
    err = float((dx1.permute(0, 3, 1, 2).cpu().double() - want).abs().max() / want.abs().max())
    print(f"dx0 bf16 {H}x{W}: max-abs error / max-abs value = {err:.3g}")
    assert err <= 2e-2


@pytest.mark.parametrize("H,W", [(52, 72), (64, 96)])
def test_dx0_float32_against_float64(H, W):
    code, cw, pw, gy, gin = _case(H, W)
    _, wb = ops.dsam_pack(cw, pw, torch.float32)
    dx, _ = ops.dsam_bwd_data(gy, code, wb, gin)
    want = _dx_f64(code, cw, pw, gy, gin)
    err = float((dx.cpu().double() - want).abs().max() / want.abs().max())
    print(f"dx0 float32 {H}x{W}: max-abs error / max-abs value = {err:.3g}")
    assert err <= F32_REL
