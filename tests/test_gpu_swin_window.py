"""rgbd_swin_window_attn (csrc/swin_attn.hip) at kernel level against float64.

The reference is tests/checkers/swin_window.py, the float64 restatement of HF's SwinLayer around
its attention core that tests/test_oracle_swin_window.py pins against transformers itself.  The
grid varies what the kernel's index arithmetic depends on: maps smaller than a window, exact
multiples of 7 (no padding), ragged maps, shifts (0 / 1 / 3 / 6 over the whole grid, every shift
0..6 at two sizes), 1 and 3 heads, B = 2 and B = 1 with 3 heads (B * nwy * nwx * heads not a
multiple of the four waves of a workgroup), NULL projection biases, q / k / v as slices of one
[rows, 3C] buffer (what swin.py passes) and as three tensors, ``out`` dense and with
``ldo = C + 16 bytes`` inside a guarded strided buffer.  At model level the backbone runs at
224x224 and 192x224 (stage 4 a single 7x7 window, and a 6x7 map padded to one) and the stage-4
layers are called the way HF clamps window and shift.  Every input sits between 0xFF (NaN)
guards (tests/checkers/guard.py), every output between guards that must stay untouched.

Bars, per element:
* float32: |err| <= 2e-6 * (1 + max|ref|) — the project's bar for the same arithmetic (f32 MFMA
  scores, float32 softmax, f32 MFMA P.V: test_core_forward_backward_vs_float64 in
  tests/test_gpu_masked_attention.py).  Measured: see test_window_attention_vs_float64.
* bf16: the reference consumes the same bf16-valued q / k / v and the biases rounded to bf16 as the
  kernel rounds them; what remains is one rounding of P and one of the output, each at most 2^-8
  relative, so |err| <= 2^-7 * max|v| (over v and the rounded bv), worst case.
"""
import copy
import functools

import pytest
import torch

from checkers import guard
from checkers.swin_window import window_attention_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SIZES = [(7, 7), (8, 10), (13, 7), (3, 16), (15, 20), (14, 21)]
SHIFTS = [0, 1, 3, 6]
SCALE = 32 ** -0.5
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]


def _grid():
    """(B, H, W, heads, shift, biases)"""
    g = [(2, H, W, heads, shift, biases) for (H, W) in SIZES for shift in SHIFTS for heads in (1, 3)
         for biases in (True, False)]
    g += [(1, H, W, 3, shift, biases) for (H, W) in SIZES for shift in SHIFTS for biases in (True, False)]
    g += [(2, H, W, 3, shift, True) for (H, W) in ((8, 10), (15, 20)) for shift in range(7)]
    return g


@functools.lru_cache(maxsize=None)
def _cases(dtype):
    """Inputs (CPU, already rounded to ``dtype``) and the float64 reference of every grid case,
    computed once per dtype and shared by the tests (never modified)."""
    out = []
    for n, (B, H, W, heads, shift, biases) in enumerate(_grid()):
        g = torch.Generator().manual_seed(1000 + n)
        C = 32 * heads
        rows = B * H * W
        qkv = torch.randn((rows, 3 * C), generator=g).to(dtype)
        table = torch.randn((169, heads), generator=g) * 0.5
        b3 = torch.randn((3, C), generator=g) * 0.5 if biases else None
        # the kernel rounds the biases of padded positions to the operand dtype
        bref = [None] * 3 if b3 is None else [b.to(dtype) for b in b3]
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        ref = window_attention_ref(q, k, v, *bref, table, B, H, W, heads, shift, SCALE)
        vmax = max(float(v.double().abs().max()), 0.0 if b3 is None else float(bref[2].double().abs().max()))
        out.append(dict(key=(B, H, W, heads, shift, biases), qkv=qkv, table=table, b3=b3, ref=ref, vmax=vmax))
    return out


def _call(pool, case, dtype, fused, ldo_pad):
    """One kernel call on guarded operands; returns the output [rows, C] (a view of a guarded
    buffer, dense or strided)."""
    from rgbd_amd import _lib
    from rgbd_amd.dense import _CODE
    from rgbd_amd.ops import _p, _stream
    B, H, W, heads, shift, biases = case["key"]
    C = 32 * heads
    rows = B * H * W
    qkv = case["qkv"].to(DEV)
    if fused:
        buf = pool.place(qkv, "qkv")
        q, k, v, ldq = buf[:, :C], buf[:, C:2 * C], buf[:, 2 * C:], 3 * C
    else:
        q, k, v = (pool.place(qkv[:, i * C:(i + 1) * C].contiguous(), "qkv"[i]) for i in range(3))
        ldq = C
    bq = bk = bv = None
    if biases:
        bq, bk, bv = (pool.place(b.to(DEV), "bias") for b in case["b3"])
    table = pool.place(case["table"].to(DEV), "table")
    ldo = C + (16 // qkv.element_size() if ldo_pad else 0)
    out = guard.strided(rows, C, ldo, dtype, DEV, tag=f"out {case['key']}") if ldo_pad else \
        guard.Guarded((rows, C), dtype, DEV, tag=f"out {case['key']}")
    pool.bufs.append(out)
    rc = _lib.lib().rgbd_swin_window_attn(_CODE[dtype], _p(q), _p(k), _p(v), ldq, _p(bq), _p(bk), _p(bv), _p(table),
                                          B, H, W, heads, 7, shift, SCALE, _p(out.payload), ldo, _stream(DEV))
    assert rc == 0, (rc, case["key"])
    return out.payload


def _errors(got, case, dtype):
    """(worst |err| / bar, worst |err|) of one case, per element."""
    ref = case["ref"]
    err = float((got.double().cpu() - ref).abs().max())
    bar = 2e-6 * (1 + float(ref.abs().max())) if dtype == torch.float32 else 2.0 ** -7 * case["vmax"]
    return err / bar, err


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_window_attention_vs_float64(dtype):
    """The whole grid in swin.py's layout (q | k | v slices of one buffer, dense out).
    Measured on an MI355X over the 158 cases: float32 max |err| 1.15e-6 = 0.18 of the bar (worst at
    B = 1, 8x10, 3 heads, shift 0); bf16 max |err| 1.43e-2 = 0.49 of the bar (worst at 3x16, shift 3)."""
    pool = guard.Pool()
    outs = [_call(pool, c, dtype, fused=True, ldo_pad=False) for c in _cases(dtype)]
    n = pool.check_all()
    worst, worst_abs, where = 0.0, 0.0, None
    for got, c in zip(outs, _cases(dtype)):
        assert torch.isfinite(got).all(), c["key"]  # no cell left unwritten, no guard value read
        frac, err = _errors(got, c, dtype)
        worst_abs = max(worst_abs, err)
        if frac > worst:
            worst, where = frac, c["key"]
    print(f"swin window attention {dtype}: {len(outs)} cases, {n} guarded buffers clean, max |err| {worst_abs:.3g}, "
          f"worst |err| / bar {worst:.3g} at (B, H, W, heads, shift, biases) = {where}")
    assert worst <= 1.0, f"{where}: |err| is {worst:.3g} x the bar"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fused,ldo_pad", [(False, False), (True, True), (False, True)],
                         ids=["separate_qkv", "ldo_padded", "separate_qkv_ldo_padded"])
def test_window_attention_layouts(dtype, fused, ldo_pad):
    """Other operand layouts the C ABI promises (ldq = C, ldo > C): the same bars, the same bits
    as the fused / dense layout, gap columns and guards untouched."""
    pool = guard.Pool()
    cases = _cases(dtype)
    outs = [_call(pool, c, dtype, fused, ldo_pad) for c in cases]
    base = [_call(pool, c, dtype, True, False) for c in cases]
    pool.check_all()
    worst = 0.0
    for got, b, c in zip(outs, base, cases):
        frac, _ = _errors(got, c, dtype)
        worst = max(worst, frac)
        assert frac <= 1.0, f"{c['key']}: |err| is {frac:.3g} x the bar"
        assert torch.equal(got, b), f"{c['key']}: differs from the fused / dense layout"
    print(f"{dtype} fused {fused} ldo_pad {ldo_pad}: worst |err| / bar {worst:.3g}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_wrapper_allocates_and_passes_what_the_kernel_needs(dtype):
    """swin.window_attention (the wrapper HipSwinLayer calls) under guarded allocation: its own
    output buffer stays inside its guards and holds the bits of the direct call."""
    from rgbd_amd import swin
    pool = guard.Pool()
    for c in _cases(dtype)[::7]:
        B, H, W, heads, shift, biases = c["key"]
        direct = _call(pool, c, dtype, True, False)
        with guard.guarded_allocations() as sweep:
            qkv = sweep.place(c["qkv"].to(DEV))
            b = None if c["b3"] is None else sweep.place(c["b3"].reshape(-1).to(DEV))
            got = swin.window_attention(qkv, b, c["table"].to(DEV), B, H, W, heads, shift, SCALE)
            assert sweep.check_all() >= 2 + biases
        assert torch.equal(got, direct), c["key"]
    pool.check_all()


@functools.lru_cache(maxsize=None)
def _backbones():
    """(HF backbone, the same with HipSwinLayer installed); shared, never modified."""
    from transformers import SwinBackbone
    from rgbd_amd import dense, swin
    from rgbd_amd.config import standard_config
    torch.manual_seed(3)
    ref = SwinBackbone(standard_config(48).backbone_config).to(DEV).eval()
    with torch.no_grad():  # non-trivial relative-position tables (HF initialises them to zero)
        for m in ref.modules():
            if hasattr(m, "relative_position_bias_table"):
                m.relative_position_bias_table.normal_(0, 0.5)
    hip = copy.deepcopy(ref)
    assert swin.install(hip) == 12
    dense.install(hip)
    return ref, hip


def _count_kernel_calls(monkeypatch):
    from rgbd_amd import swin
    calls = []
    real = swin.window_attention

    def counted(qkv, bqkv, table, B, H, W, heads, shift, scale):
        calls.append((H, W, heads, int(shift)))
        return real(qkv, bqkv, table, B, H, W, heads, shift, scale)
    monkeypatch.setattr(swin, "window_attention", counted)
    return calls


def _max_rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


@pytest.mark.parametrize("hw,last", [((224, 224), (7, 7)), ((192, 224), (6, 7))], ids=["224x224", "192x224"])
def test_backbone_small_maps_run_the_kernel(hw, last, monkeypatch):
    """The backbone as the model calls it.  transformers' SwinBackbone passes
    ``always_partition=True`` to every layer, so the window stays 7 and the second block of each
    stage keeps shift 3 at every resolution: at 224x224 stage 4 is one unpadded 7x7 window, at
    192x224 it is a 6x7 map (smaller than a window) padded to 7x7 — both shifted.  All twelve
    layers take the kernel and the features match HF float32 (1e-4 of each map's maximum, the bar
    of tests/test_gpu_swin.py)."""
    ref, hip = _backbones()
    calls = _count_kernel_calls(monkeypatch)
    x = torch.randn((2, 3, *hw), device=DEV)
    with torch.no_grad():
        want = ref(x).feature_maps
        got = hip(x).feature_maps
    assert len(calls) == 12, calls
    assert [c[3] for c in calls] == [0, 3] * 6
    assert calls[-2:] == [(*last, 24, 0), (*last, 24, 3)]
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape
        err = _max_rel(a, b)
        print(f"{hw} stage {k + 1} {tuple(a.shape)}: rel err vs HF float32 {err:.3g}")
        assert err < 1e-4, f"stage {k + 1}"


def test_layer_window_clamp_takes_the_right_path(monkeypatch):
    """The stage-4 layers called as HF's SwinEncoder calls them by default (``always_partition``
    False), where HF clamps.  On a 7x7 map the window stays 7 and HF forces the shift to 0:
    ``_covered`` holds, both blocks run the kernel with shift 0 and the output is the HF layer's.
    On a 6x7 map HF shrinks the window to 6: ``_covered`` must refuse, so the kernel (whose window
    is 7) never sees it.  (That HF path cannot be run to the end here: transformers 5.15 adds the
    49 x 49 relative-position bias to the 36 x 36 scores of the shrunk window and raises.)"""
    from rgbd_amd import swin
    ref, hip = _backbones()
    rb, hb = (copy.deepcopy(m.swin.encoder.layers[3].blocks) for m in (ref, hip))  # the clamp stays on the layer
    assert [int(h.shift_size) for h in hb] == [0, 3]
    calls = _count_kernel_calls(monkeypatch)
    x = torch.randn((2, 49, 768), device=DEV)
    want, got = x, x
    with torch.no_grad():
        for r, h in zip(rb, hb):
            want, got = r(want, (7, 7))[0], h(got, (7, 7))[0]
            assert int(h.window_size) == 7 and int(h.shift_size) == 0 and swin._covered(h, x)
    assert calls == [(7, 7, 24, 0)] * 2, calls
    assert _max_rel(got, want) < 1e-4
    with torch.no_grad():
        for h in copy.deepcopy(hip.swin.encoder.layers[3].blocks):
            assert swin._covered(h, x)
            h.set_shift_and_window_size((6, 7))
            assert int(h.window_size) == 6 and int(h.shift_size) == 0 and not swin._covered(h, x)
