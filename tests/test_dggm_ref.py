"""The float64 restatement of K2 (tests/checkers/dggm_ref.py) pinned on the CPU, and the two
yardsticks of tests/test_gpu_dggm_ragged.py measured.

1. The checker's nearest source indices equal F.interpolate(mode="nearest") of an index plane
   exactly, for every resampling pair the GPU tests use.
2. Its forward agrees with oracle.dggm.dggm_forward (torch CPU float32) and its dW/db with
   autograd through the oracle, at the ragged scales and inputs of checkers/dggm_cases.py.  The
   largest error ratios of torch's float32 path against the checker are the yardsticks: K_F and
   K_B of dggm_cases are twice them, rounded up, and this file asserts that they cover them.
   Measured with the torch build the suite runs on: forward 499.64 (scale 96x25x33; 72.7 at
   32x30x34, at most 3.3 elsewhere), forward with cp1 444.5, dW 6.45, db 1.46.  Against the
   checker's fma variant (the source coordinate rounded once) the forward ratio is at most 3.3,
   so what K_F covers is one ulp of a float32 source coordinate, not an arithmetic difference.
3. A reference whose dW/db leave out the tail tile of the last image misses the K_B bound by
   four orders of magnitude or more at most entries: the bound can see a skipped tile.
4. Upsampling (out == in, and out == 2*in, which torch's CPU nearest kernel special-cases as
   dst >> 1): the float32 rule floor(dst * scale) has scale 1 or 0.5 exactly there, so the
   checker, the kernel's rule and torch agree; no disagreement to record.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from checkers import dggm_cases as cases
from checkers import dggm_ref as ref
from oracle import dggm as dggm_o

EPS = cases.EPS
AXIS_PAIRS = sorted({p for probe in cases.PROBES for p in probe} |
                    {(cases.H, h) for _, h, _ in cases.SCALES} | {(cases.W, w) for _, _, w in cases.SCALES} |
                    {(7, 3), (9, 1), (7, 7), (7, 14), (9, 18)})


@pytest.mark.parametrize("n_in,n_out", AXIS_PAIRS)
def test_nearest_index_equals_torch(n_in, n_out):
    plane = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, n_in, 1)
    want = F.interpolate(plane, size=(n_out, 1), mode="nearest").reshape(-1).long().numpy()
    np.testing.assert_array_equal(ref.nearest_index(n_in, n_out), want)
    want = F.interpolate(plane.reshape(1, 1, 1, n_in), size=(1, n_out), mode="nearest").reshape(-1).long().numpy()
    np.testing.assert_array_equal(ref.nearest_index(n_in, n_out), want)


@pytest.mark.parametrize("n_in,n_out", AXIS_PAIRS)
def test_bilinear_of_a_ramp_matches_torch(n_in, n_out):
    """Bilinear resampling of the index ramp returns the source coordinate itself: the checker's
    (i0, i1, l1) against torch's float32 kernel within two ulp of the coordinate."""
    ramp = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, n_in, 1).expand(1, 1, n_in, 2).contiguous()
    want = F.interpolate(ramp, size=(n_out, 2), mode="bilinear", align_corners=False)[0, 0, :, 0].double().numpy()
    i0, i1, l1 = ref.bilinear_index(n_in, n_out)
    assert i0.min() >= 0 and i1.max() <= n_in - 1 and (i1 - i0).max() <= 1
    got = i0 * (1.0 - l1.astype(np.float64)) + i1 * l1.astype(np.float64)
    np.testing.assert_allclose(got, want, rtol=2.0 ** -22, atol=2.0 ** -22)


def _oracle(k):
    i, r = cases.case(k)
    pv = cases.pixel_values()
    wt = i["weight"].clone().requires_grad_(True)
    bs = i["bias"].clone().requires_grad_(True)
    out = dggm_o.dggm_forward([i["color"]], pv[:, 6:9], pv[:, 9:10], [wt], [bs])[0]
    out.backward(i["dout"])
    return i, r, out.detach(), wt.grad.reshape(-1, 3), bs.grad


@pytest.mark.parametrize("k", range(len(cases.SCALES)), ids=[f"{c}x{h}x{w}" for c, h, w in cases.SCALES])
def test_checker_vs_oracle_and_yardsticks(k):
    i, r, out, dw, db = _oracle(k)
    # share of elements that may take either ReLU branch in float32
    assert float(r["near"].double().mean()) <= 1e-3
    # the checker rounded to float32 is the oracle's output up to float32 rounding of its terms
    f = ref.ratio(out.double() - r["out"], EPS * r["A_out"])
    f1 = ref.ratio((i["cp1"] + out).double() - (r["out"] + i["cp1"].double()), EPS * (r["A_out"] + i["cp1"].abs().double()))
    w = ref.ratio(dw.double() - r["dw"], EPS * r["S_dw"])
    b = ref.ratio(db.double() - r["db"], EPS * r["S_db"])
    pv = cases.pixel_values()
    ffma = ref.ratio(out.double() - ref.dggm_ref(pv[:, 6:9], pv[:, 9:10], i["color"], i["weight"], i["bias"],
                                                 fma=True)["out"], EPS * r["A_out"])
    print(f"scale {cases.SCALES[k]}: near {int(r['near'].sum())}  torch-f32/checker ratios: fwd {f:.2f} "
          f"fwd+cp1 {f1:.2f} dW {w:.2f} db {b:.2f}  fwd vs fma checker {ffma:.2f}")
    assert math.ceil(2 * max(f, f1)) <= cases.K_F
    assert math.ceil(2 * max(w, b)) <= cases.K_B


@pytest.mark.parametrize("k", range(len(cases.SCALES)), ids=[f"{c}x{h}x{w}" for c, h, w in cases.SCALES])
def test_dropped_tail_tile_misses_the_bound(k):
    i, r = cases.case(k)
    pv = cases.pixel_values()
    cut = ref.dggm_ref(pv[:, 6:9], pv[:, 9:10], i["color"], i["weight"], i["bias"], dout=i["dout"],
                       keep=cases.tail_tile_keep(k))
    for key in ("dw", "db"):
        s = r["S_" + key]
        miss = ((cut[key] - r[key]).abs() > cases.K_B * EPS * s)[s > 0]
        assert float(miss.double().mean()) > 0.5, key


@pytest.mark.parametrize("H,W,h,w", [(7, 9, 7, 9), (7, 9, 14, 18), (5, 9, 5, 18)])
def test_upsample_branch(H, W, h, w):
    g = torch.Generator().manual_seed(H * 100 + h)
    grad = torch.randn((2, 3, H, W), generator=g)
    mask = (torch.rand((2, 1, H, W), generator=g) < 0.5).float()
    color = torch.randn((2, 8, h, w), generator=g)
    weight, bias = torch.randn((8, 3, 1, 1), generator=g), torch.randn((8,), generator=g)
    r = ref.dggm_ref(grad, mask, color, weight, bias)
    out = dggm_o.dggm_forward([color], grad, mask, [weight], [bias])[0]
    assert ref.ratio(out.double() - r["out"], EPS * r["A_out"]) <= cases.K_F
    idx = torch.arange(H * W, dtype=torch.float32).reshape(1, 1, H, W)
    want = F.interpolate(idx, size=(h, w), mode="nearest")[0, 0].long().numpy()
    got = ref.nearest_index(H, h)[:, None] * W + ref.nearest_index(W, w)[None, :]
    np.testing.assert_array_equal(got, want)
    if h == 2 * H:
        np.testing.assert_array_equal(ref.nearest_index(H, h), np.arange(h) >> 1)
    if h == H:
        np.testing.assert_array_equal(ref.nearest_index(H, h), np.arange(h))
        i0, _, l1 = ref.bilinear_index(H, h)
        np.testing.assert_array_equal(i0, np.arange(h))
        assert not l1.any()
