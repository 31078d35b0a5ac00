"""K5, the masked 3x3 stride-2 DSAM convolutions (forward, dX, dW/db; csrc/dsam_lds.hip,
dsam_wgrad.hip, dsam_f32.hip, dsam_pack.hip), against the float64 restatement of
checkers/dsam_ref.py at the ragged shapes of checkers/dsam_cases.py: every k_dsam_lds<KC> and
k_dsam_wgrad_mm<FM> instantiation, linear / blocked-exact / blocked-ragged tiles, a second and
partly empty N tile, a ragged kk tile, unequal and empty dX parity classes, n_masks 0..4, under
five region-code maps each (tests/test_dsam_cases.py asserts that the table reaches them).

Bounds, element-wise over every element (EPS = 2^-24; A = the sum of the magnitudes of the
element's summands; K from torch's CPU float32 path, see dsam_cases):
    float32 outputs   |hip - ref| <= K * EPS * A           (float32 legs, the float32-interface
                                                            forward, dW, db)
    bf16 outputs      |hip - ref| <= 2^-8 |ref| + K * EPS * A
The bf16 references use the merged filters Wq_k as the kernels are documented to round them, so
the forward through ops.dsam_fwd_nhwc_f32io, whose float32 output is not rounded, is the sharp
check: tests/test_dsam_ref.py shows that a filter rounded after every addition, a bias prefix off
by one mask, a code taken at the wrong pixel, a wrapped edge tap or a dropped unit / kk tile all
miss these bounds.  Every test prints the largest error / bound and the failing share.

Case F (1x1 and 1x9 maps): the dX parity classes with py = 1 (and px = 1 at 1x1) are empty.  Read
in csrc/dsam_lds.hip before the first run: ld_geom gives such a class Hc = 0 (or Wc = 0), hence
ntiles = 0 in both tilings; plan_tile returns at ``tile >= G.ntiles`` and items_body gives such
tiles no chunks (``if (tile < G.ntiles) nc = ...``), so no item of an empty class exists and
ld_row's unconditional code load is never issued for a pixel the map lacks.

Measured on the MI355X (profiles/dsam_parity/errors.txt has every figure; largest error / bound
per entry point and leg over all cases and code maps; beside it the torch CPU float32 path's
unrounded value under the K * EPS * A term alone):
  bwd_data f32           dx      0.143 at E zero     (cpu: 0.108)
  bwd_data nhwc bf16     dx      0.993 at E zero     (cpu: 0.049)
  bwd_weight f32         dbias   0.123 at F2 const0  (cpu: 0.093)
  bwd_weight f32         dconv   0.980 at F1 const0  (cpu: 0.980)
  bwd_weight f32         dproj   0.980 at F1 const0  (cpu: 0.980)
  bwd_weight nchw        dbias   0.002 at E const0   (cpu: 0.002)
  bwd_weight nhwc        dbias   0.002 at E const0   (cpu: 0.002)
  bwd_weight nhwc        dconv   0.130 at F2 const0  (cpu: 0.108)
  bwd_weight nhwc        dproj   0.135 at F2 const0  (cpu: 0.135)
  bwd_weight_multi       dconv   0.033 at E rand     (cpu: 0.055)
  bwd_weight_multi       dproj   0.029 at E rand     (cpu: 0.065)
  fwd f32                y       0.381 at E fifteen  (cpu: 0.018)
  fwd_nhwc bf16          y       0.994 at C zero     (cpu: 0.044)
  fwd_nhwc_f32io bf16    y       0.994 at C zero     (cpu: 0.044)
  fwd_nhwc_f32io f32     y       0.100 at D fifteen  (cpu: 0.027)
The bf16 outputs sit at 0.99 because 2^-8 |ref| is the output rounding itself; the float32 output of
the same launch uses a tenth of its bound.  dW of case F1 has one summand per element (K capped
at 1): 0.98 is the rounding of the one float32 product.  No kernel or shape check had to change;
the guard-band sweep (test_gpu_guard_bands.py) was run once after these tests passed, all passing.
"""
import functools

import numpy as np
import pytest
import torch

import _rgbd_import  # noqa: F401
from checkers import dsam_cases as cases
from checkers import dsam_ref as R
from rgbd_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
BF16, F32 = torch.bfloat16, torch.float32
BF_PAIRS = [(n, k) for n in cases.BF16_CASES for k in cases.MAPS]
F32_PAIRS = [(n, k) for n in cases.CASES for k in cases.MAPS]


def _info(n_masks):
    rec = np.zeros(len(n_masks), dtype=ops.DECOMP_INFO_DTYPE)
    rec["n_masks"] = n_masks
    return torch.from_numpy(rec.view(np.uint8).reshape(len(n_masks), -1)).to(DEV)


def _nhwc(t, dtype):
    return t.permute(0, 2, 3, 1).contiguous().to(device=DEV, dtype=dtype)


def _nchw(t_nhwc):
    return t_nhwc.permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=4)
def _dev(name, kind, bf16):
    """The case's operands on the device, in the layouts the entry points take."""
    i, code, ref = cases.reference(name, kind, bf16)
    dt = BF16 if bf16 else F32
    d = dict(i=i, ref=ref, code=code.to(torch.uint8).to(DEV), info=_info(i["n_masks"]),
             x=_nhwc(i["x"], dt), gy=_nhwc(i["gy"], dt), res=_nhwc(i["residual"], dt), gin=_nhwc(i["gin"], dt),
             cw=i["conv_w"].to(DEV), pw=i["proj_w"].to(DEV), b4=i["bias4"].to(DEV))
    for k in ("x", "gy", "res", "gin"):
        assert torch.equal(_nchw(d[k]).float().cpu(), i[{"res": "residual"}.get(k, k)]), k  # nothing rounded again
    if bf16:
        d["wf"], d["wb"] = ops.dsam_pack(d["cw"], d["pw"], BF16, code_mask=ops.dsam_code_masks([d["code"]])[0:1])
    else:
        d["wf"], d["wb"] = ops.dsam_pack(d["cw"], d["pw"], F32)
    return d


def _check(tag, name, kind, leg, got_nchw, ref, rel=0.0):
    ratio, share = R.compare(got_nchw, ref[leg][0], ref[leg][1], cases.k_of(name, leg), rel)
    print(f"K5PARITY {name:2s} {kind:7s} {tag:22s} {leg:5s} error/bound {ratio:.3f} failing {share:.4f}")
    return [] if ratio <= 1 else [f"{tag} {leg}: error / bound {ratio:.3g}, failing share {share:.3g}"]


@pytest.mark.parametrize("name,kind", BF_PAIRS)
def test_bf16_legs_against_float64(name, kind):
    d = _dev(name, kind, True)
    B, Ci, Co, h, w = cases.CASES[name]
    ref, bad = d["ref"], []
    y16, y32 = ops.dsam_fwd_nhwc_f32io(d["x"], d["code"], d["info"], d["wf"], d["b4"],
                                       residual_f32_nhwc=d["res"].float())
    bad += _check("fwd_nhwc_f32io f32", name, kind, "y", _nchw(y32), ref)
    bad += _check("fwd_nhwc_f32io bf16", name, kind, "y", _nchw(y16), ref, R.BF16_REL)
    assert torch.equal(y16, y32.bfloat16()), "the bf16 output is the one rounding of the float32 one"
    y = ops.dsam_fwd_nhwc(d["x"], d["code"], d["info"], d["wf"], d["b4"], residual_nhwc=d["res"])
    bad += _check("fwd_nhwc bf16", name, kind, "y", _nchw(y), ref, R.BF16_REL)
    none, dx = ops.dsam_bwd_data(d["gy"], d["code"], d["wb"], None, want_nhwc=True, want_nchw=False, cin=Ci,
                                 gin_nhwc=d["gin"])
    assert none is None
    bad += _check("bwd_data nhwc bf16", name, kind, "dx", _nchw(dx), ref, R.BF16_REL)
    dconv, dproj, db = ops.dsam_bwd_weight(None, d["x"], d["code"], d["info"], gout_nhwc=d["gy"])
    for leg, got in (("dconv", dconv), ("dproj", dproj), ("dbias", db)):
        bad += _check("bwd_weight nhwc", name, kind, leg, got, ref)
    assert not bad, f"{name} {kind}: " + "; ".join(bad)


@pytest.mark.parametrize("name,kind", BF_PAIRS)
def test_bf16_entry_points_agree_bitwise(name, kind):
    """The NCHW entry points and the planned legs against the NHWC-only calls the test above
    holds to the float64 reference: bit for bit, db of the NCHW gradient within the db bound (its
    sums run in another order)."""
    d = _dev(name, kind, True)
    B, Ci, Co, h, w = cases.CASES[name]
    x, code, info, gy = d["x"], d["code"], d["info"], d["gy"]
    y = ops.dsam_fwd_nhwc(x, code, info, d["wf"], d["b4"], residual_nhwc=d["res"])
    _, dx = ops.dsam_bwd_data(gy, code, d["wb"], None, want_nhwc=True, want_nchw=False, cin=Ci, gin_nhwc=d["gin"])
    dw = ops.dsam_bwd_weight(None, x, code, info, gout_nhwc=gy)
    res_nchw, gin_nchw, gy_nchw = (_nchw(d[k]).contiguous() for k in ("res", "gin", "gy"))
    y_nchw, y_nhwc = ops.dsam_fwd(x, code, info, d["wf"], d["b4"], residual=res_nchw, want_nhwc=True)
    assert torch.equal(y_nhwc, y) and torch.equal(y_nchw, _nchw(y))
    dx_nchw, dx_nhwc = ops.dsam_bwd_data(gy, code, d["wb"], gin_nchw, want_nhwc=True)
    assert torch.equal(dx_nhwc, dx) and torch.equal(dx_nchw, _nchw(dx))
    dw2 = ops.dsam_bwd_weight(gy_nchw, x, code, info, gout_nhwc=gy)
    assert torch.equal(dw2[0], dw[0]) and torch.equal(dw2[1], dw[1])
    assert not _check("bwd_weight nchw", name, kind, "dbias", dw2[2], d["ref"])
    plans = ops.dsam_plan([(ops.LEG_FWD, code, Ci, Co), (ops.LEG_DX, code, Ci, Co), (ops.LEG_DW, code, Ci, Co)])
    assert torch.equal(ops.dsam_fwd_nhwc(x, code, info, d["wf"], d["b4"], residual_nhwc=d["res"], plan=plans[0]), y)
    assert torch.equal(ops.dsam_bwd_data(gy, code, d["wb"], None, want_nhwc=True, want_nchw=False, cin=Ci,
                                         gin_nhwc=d["gin"], plan=plans[1])[1], dx)
    for a, b in zip(ops.dsam_bwd_weight(None, x, code, info, gout_nhwc=gy, plan=plans[2]), dw):
        assert torch.equal(a, b)


@pytest.mark.parametrize("pair", [("A", "B"), ("D", "E")], ids=["A+B_same_FM", "D+E_FM4+FM6"])
def test_bwd_weight_multi_equals_single_legs(pair):
    """Two legs' dW GEMMs in one persistent launch, bit for bit the single launches.  The info
    records are shared by the launch (image b of either leg reads record b): the second leg's."""
    ds = [_dev(n, "rand", True) for n in pair]
    info = ds[1]["info"]
    shapes = [cases.CASES[n] for n in pair]
    assert shapes[0][0] <= shapes[1][0]
    single = [ops.dsam_bwd_weight(None, d["x"], d["code"], info[:s[0]].contiguous(), gout_nhwc=d["gy"])
              for d, s in zip(ds, shapes)]
    plans = ops.dsam_plan([(ops.LEG_DW, d["code"], s[1], s[2]) for d, s in zip(ds, shapes)])
    multi = ops.dsam_bwd_weight_multi([(d["gy"], d["x"], d["code"], p) for d, p in zip(ds, plans)], info)
    for n, got, want in zip(pair, multi, single):
        for a, b, leg in zip(got, want, ("dconv", "dproj", "dbias")):
            assert torch.equal(a, b), f"{n} {leg}"
    for leg, got in zip(("dconv", "dproj"), multi[1]):  # the second leg ran with its own records
        assert not _check("bwd_weight_multi", pair[1], "rand", leg, got, ds[1]["ref"])


@pytest.mark.parametrize("name,kind", F32_PAIRS)
def test_float32_legs_against_float64(name, kind):
    """The float32 legs (the literal five-convolution formula, nothing merged), cases A to G."""
    d = _dev(name, kind, False)
    ref, bad = d["ref"], []
    res_nchw, gin_nchw, gy_nchw = (_nchw(d[k]).contiguous() for k in ("res", "gin", "gy"))
    y, y_nhwc = ops.dsam_fwd(d["x"], d["code"], d["info"], d["wf"], d["b4"], residual=res_nchw, want_nhwc=True)
    bad += _check("fwd f32", name, kind, "y", y, ref)
    assert torch.equal(_nchw(y_nhwc), y)
    dx, dx_nhwc = ops.dsam_bwd_data(d["gy"], d["code"], d["wb"], gin_nchw, want_nhwc=True)
    bad += _check("bwd_data f32", name, kind, "dx", dx, ref)
    assert torch.equal(_nchw(dx_nhwc), dx)
    for leg, got in zip(("dconv", "dproj", "dbias"), ops.dsam_bwd_weight(gy_nchw, d["x"], d["code"], d["info"])):
        bad += _check("bwd_weight f32", name, kind, leg, got, ref)
    assert not bad, f"{name} {kind}: " + "; ".join(bad)
