"""K2, the DGGM gated fusion (csrc/dggm.hip), against its float64 restatement
(tests/checkers/dggm_ref.py) at ragged sizes and every vector width.

pixel_values is 97x131, B = 2, the 10-channel tensor with noise in channels 0-5; gradient planes
are white noise, the mask Bernoulli(0.5), weights N(0,1), |b| >= 0.05 (checkers/dggm_cases.py),
so a wrong tap, a wrong nearest index or a skipped tail tile moves outputs by their own size.
Seven scales cover PX = 1 (13 tiles; C % 32 != 0; one partial tile; C % 8 != 0), PX = 4 (one
partial tile; 4 tiles) and PX = 8 (2 tiles), in float32 and bfloat16, without cp1, with NCHW
and with NHWC cp1, through the per-scale entry points and the _multi ones.

Bounds (EPS = 2^-24; K_F, K_B from torch's own float32 path against the same checker, measured
on the CPU by tests/test_dggm_ref.py, never from the HIP output):
  forward float32   |hip - ref64| <= K_F * EPS * A_out,   A_out = |cp1| + |color| + |b| + sum|w||g|
  forward bfloat16  |hip - ref64| <= 2^-8 * |ref64| + K_F * EPS * A_out
  dW, db            |hip - ref64| <= K_B * EPS * S,        S = sum of the absolute summands
with dout zeroed where |pre| <= 1e-5 * A_pre (either ReLU branch is a correct float32 answer
there; the share of such elements is asserted <= 0.1 % per scale and is 0 on these inputs).
A reference that leaves the tail tile of the last image out of dW/db misses the K_B bound, so
the bound resolves a skipped tile (asserted here on the CPU, no extra launch).

K_F = 1000, K_B = 13.  K_F is that large because torch's CPU kernel rounds the bilinear source
coordinate once (a fused multiply-add) where the checker, like the kernel (csrc is compiled with
-ffp-contract=off), rounds each operation; see checkers/dggm_cases.py.  Largest HIP error / bound
measured on an MI355X, the same for the per-scale and the _multi entry points
(profiles/dggm_ragged/errors.txt has every scale, dtype, cp1 layout and entry point):
  forward float32   PX=1 0.0043, PX=4 0.0037, PX=8 0.0033 (no cp1); 0.0032 / 0.0027 / 0.0027 (cp1 NCHW
                    and NHWC); that is at most 4.3 * EPS * A_out at every scale
  forward bfloat16  PX=1 0.981, PX=4 0.981, PX=8 0.979: the output's own round-to-nearest-even,
                    which reaches 2^-8 relative just above a power of two
  dW / db float32   PX=1 0.16 / 0.052, PX=4 0.20 / 0.059, PX=8 0.15 / 0.034
  dW / db bfloat16  PX=1 0.16 / 0.013, PX=4 0.17 / 0.002, PX=8 0.055 / 0.002
  bilinear probes   at most 0.0024 (2.4 * EPS * A_out)

The exact index probes run one scale per resampling pair (rows and columns are independent, so
a long axis is paired with a short one): an index plane as the mask reads the nearest source
index back exactly, and column / row ramps as gradient planes read the bilinear source
coordinate back within the forward float32 bound.
"""
import numpy as np
import pytest
import torch

from checkers import dggm_cases as cases
from checkers import dggm_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS, K_F, K_B = cases.EPS, cases.K_F, cases.K_B
DTYPES = [torch.float32, torch.bfloat16]
NAME = {torch.float32: "f32", torch.bfloat16: "bf16"}


def _ops():
    from rgbd_amd import ops
    return ops


def _pv():
    return cases.pixel_values().to(DEV)


def _scale_id(k):
    C, h, w = cases.SCALES[k]
    return f"{C}x{h}x{w} PX={cases.px_of(h, w)}"


def _run_fwd(entry, cp1_mode, dtype):
    """-> {k: hip output (float64, CPU)} of all seven scales through one kind of entry point."""
    ops, pv = _ops(), _pv()
    ins = {k: cases.case(k, dtype)[0] for k in range(len(cases.SCALES))}
    dev = {k: {n: (t.to(DEV, dtype) if n in ("color", "cp1", "dout") else t.to(DEV)) for n, t in i.items()}
           for k, i in ins.items()}
    outs = {}
    if entry == "single":
        for k, d in dev.items():
            outs[k] = ops.dggm_fuse_fwd(d["cp1"] if cp1_mode == "nchw" else None, d["color"], pv, d["weight"], d["bias"])
    else:
        for grp in cases.GROUPS:
            nhwc = tuple(j for j, k in enumerate(grp) if cp1_mode == "nhwc" and cases.SCALES[k][0] % 8 == 0)
            cp1s = None
            if cp1_mode != "none":
                cp1s = [dev[k]["cp1"].permute(0, 2, 3, 1).contiguous() if j in nhwc else dev[k]["cp1"]
                        for j, k in enumerate(grp)]
            res = ops.dggm_fuse_fwd_multi(cp1s, [dev[k]["color"] for k in grp], pv, [dev[k]["weight"] for k in grp],
                                          [dev[k]["bias"] for k in grp], cp1_nhwc=nhwc)
            outs.update(dict(zip(grp, res)))
    for k, o in outs.items():
        assert o.dtype == dtype and o.shape == dev[k]["color"].shape
    return {k: o.double().cpu() for k, o in outs.items()}


FWD_CASES = [(e, c) for e in ("single", "multi") for c in ("none", "nchw", "nhwc") if (e, c) != ("single", "nhwc")]


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("entry,cp1_mode", FWD_CASES)
def test_forward_vs_float64(entry, cp1_mode, dtype):
    outs = _run_fwd(entry, cp1_mode, dtype)
    pv = cases.pixel_values()
    worst = []
    for k in range(len(cases.SCALES)):
        i, r = cases.case(k, dtype)
        assert float(r["near"].double().mean()) <= 1e-3, _scale_id(k)
        want, a_out = r["out"], r["A_out"]
        if cp1_mode != "none":
            want, a_out = want + i["cp1"].double(), a_out + i["cp1"].abs().double()
        bound = K_F * EPS * a_out
        if dtype == torch.bfloat16:
            bound = bound + 2.0 ** -8 * want.abs()
        err = (outs[k] - want).abs()
        q = ref.ratio(err, bound)
        line = f"fwd {entry:6s} cp1={cp1_mode:4s} {NAME[dtype]:4s} {_scale_id(k):16s} err/bound {q:.4f}"
        if dtype == torch.float32:   # for the record: against the source coordinate rounded once
            fma = ref.dggm_ref(pv[:, 6:9], pv[:, 9:10], i["color"], i["weight"], i["bias"], fma=True)["out"]
            if cp1_mode != "none":
                fma = fma + i["cp1"].double()
            line += f"   err/(EPS*A_out) {ref.ratio(err, EPS * a_out):.2f}, against the fma checker " \
                    f"{ref.ratio(outs[k] - fma, EPS * a_out):.2f}"
        print(line)
        worst.append((q, _scale_id(k)))
    assert max(worst)[0] <= 1.0, max(worst)


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("entry", ["single", "multi"])
def test_backward_vs_float64(entry, dtype):
    ops, pv = _ops(), _pv()
    n = len(cases.SCALES)
    dev = {}
    for k in range(n):
        i = cases.case(k, dtype)[0]
        dev[k] = (i["dout"].to(DEV, dtype), i["weight"].to(DEV), i["bias"].to(DEV))
    got = {}
    if entry == "single":
        for k, (d, wt, bs) in dev.items():
            got[k] = ops.dggm_fuse_bwd(d, pv, wt, bs)
    else:
        for grp in cases.GROUPS:
            res = ops.dggm_fuse_bwd_multi([dev[k][0] for k in grp], pv, [dev[k][1] for k in grp],
                                          [dev[k][2] for k in grp])
            got.update(dict(zip(grp, res)))
    cpu_pv = cases.pixel_values()
    worst = []
    for k in range(n):
        i, r = cases.case(k, dtype)
        dw, db = (t.double().cpu() for t in got[k])
        qw = ref.ratio(dw - r["dw"], K_B * EPS * r["S_dw"])
        qb = ref.ratio(db - r["db"], K_B * EPS * r["S_db"])
        print(f"bwd {entry:6s} {NAME[dtype]:4s} {_scale_id(k):16s} dW err/bound {qw:.4f}  db err/bound {qb:.4f}")
        worst += [(qw, "dW " + _scale_id(k)), (qb, "db " + _scale_id(k))]
        # the same bound rejects a reference without the last image's tail tile
        cut = ref.dggm_ref(cpu_pv[:, 6:9], cpu_pv[:, 9:10], i["color"], i["weight"], i["bias"], dout=i["dout"],
                           keep=cases.tail_tile_keep(k))
        for key in ("dw", "db"):
            s = r["S_" + key]
            miss = ((cut[key] - r[key]).abs() > K_B * EPS * s)[s > 0]
            assert float(miss.double().mean()) > 0.5, (key, _scale_id(k))
    assert max(worst)[0] <= 1.0, max(worst)


# ------------------------------------------------------------------ exact index probes
PROBES = cases.PROBES + [((7, 14), (9, 9))]   # out == 2*in: torch's CPU nearest special case (dst >> 1)
PROBE_IDS = [f"{a}to{b}_{c}to{d}" for (a, b), (c, d) in PROBES]
PROBE_C = 8


@pytest.mark.parametrize("rows,cols", PROBES, ids=PROBE_IDS)
def test_nearest_source_index_exact(rows, cols):
    """mask = y*W + x (exact in float32), grad = 1, w = (1, 0, 0), b = 0, colour = 0: the output is
    the nearest source index times bilinear(ones) = 1 +- a few ulp; rounded, it is the index."""
    (H, h), (W, w) = rows, cols
    assert H * W <= 2 ** 24
    pv = torch.ones((1, 4, H, W))
    pv[0, 3] = torch.arange(H * W, dtype=torch.float32).reshape(H, W)
    weight = torch.tensor([1.0, 0.0, 0.0]).repeat(PROBE_C, 1).reshape(PROBE_C, 3, 1, 1)
    out = _ops().dggm_fuse_fwd(None, torch.zeros((1, PROBE_C, h, w), device=DEV), pv.to(DEV), weight.to(DEV),
                               torch.zeros(PROBE_C, device=DEV))
    want = ref.nearest_index(H, h)[:, None] * W + ref.nearest_index(W, w)[None, :]
    got = out.double().cpu().round().long().numpy()[0]
    for c in range(PROBE_C):
        np.testing.assert_array_equal(got[c], want)


@pytest.mark.parametrize("rows,cols", PROBES, ids=PROBE_IDS)
def test_bilinear_source_coordinate(rows, cols):
    """grad plane 0 = column ramp, plane 1 = row ramp, mask = 1, non-negative weights, b = 0,
    colour = 0: the output is a combination of the two source coordinates."""
    (H, h), (W, w) = rows, cols
    pv = torch.zeros((1, 4, H, W))
    pv[0, 0] = torch.arange(W, dtype=torch.float32)[None, :]
    pv[0, 1] = torch.arange(H, dtype=torch.float32)[:, None]
    pv[0, 3] = 1.0
    weight = torch.randn((PROBE_C, 3), generator=torch.Generator().manual_seed(H + W)).abs()
    weight[0], weight[1] = torch.tensor([1.0, 0.0, 0.0]), torch.tensor([0.0, 1.0, 0.0])
    color, bias = torch.zeros((1, PROBE_C, h, w)), torch.zeros(PROBE_C)
    out = _ops().dggm_fuse_fwd(None, color.to(DEV), pv.to(DEV), weight.reshape(PROBE_C, 3, 1, 1).to(DEV), bias.to(DEV))
    r = ref.dggm_ref(pv[:, 0:3], pv[:, 3:4], color, weight, bias)
    q = ref.ratio(out.double().cpu() - r["out"], K_F * EPS * r["A_out"])
    print(f"bilinear probe {H}->{h}, {W}->{w}: err/bound {q:.4f}  err/(EPS*A_out) {q * K_F:.2f}")
    assert q <= 1.0
