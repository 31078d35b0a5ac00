"""rgbd_swin_window_attn_bwd (csrc/swin_attn.hip) and rgbd_gelu / rgbd_gelu_bwd (csrc/act.hip) at
kernel level against float64 autograd.

The reference is float64 autograd through tests/checkers/swin_window.window_attention_ref (the
restatement of HF's SwinLayer that tests/test_oracle_swin_window.py pins against transformers),
differentiated in q, k, v, bk, bv and the table.  The grid is the smallest that varies what the
index arithmetic depends on: a single unpadded window (7x7), ragged maps (8x10, 15x20), a map
smaller than a window (3x16), an exact multiple (14x21); shifts 0 / 3 / 6; 1 and 3 heads; B = 2,
and B = 1 with 3 heads (an item count that is no multiple of the waves of a workgroup); biases
present and NULL (then dbk / dbv NULL too).  Layouts: q / k / v and dq / dk / dv as slices of one
[rows, 3C] buffer each (what swin.py passes), as three dense tensors, and dq / dk / dv with
``ldd = C + 16 bytes`` inside guarded strided buffers.  Every input sits between 0xFF (NaN) guards
(tests/checkers/guard.py); every output and the workspace start as 0xFF bytes (NaN), and afterwards
every payload cell is finite and every guard and gap byte untouched.

Bars, per gradient (dq, dk, dv, dbk, dbv, dtable) and case:
* float32: |err| <= 1e-5 * (1 + max|want|), the project's bar for the same arithmetic
  (tests/test_gpu_masked_attention.py, test_core_forward_backward_vs_float64).
* bf16: the reference takes the same bf16-valued inputs (biases rounded as the kernel rounds them).
  The yardstick is ``_bf16_restatement``: plain torch bf16 on the CPU — Q K^T, float32 softmax
  rounded to bf16, P V — differentiated by autograd.  The kernel's error against float64 is at most
  1.5 x that restatement's own error + 1e-3 of the gradient's max (the rule and slack of
  test_module_bf16_autocast_vs_torch in tests/test_gpu_masked_attention.py).
Exact: dbk = dbv = 0 when H and W are multiples of 7; two calls agree bitwise.
"""
import functools

import pytest
import torch

from checkers import guard
from checkers.swin_window import WS, _region, window_attention_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SIZES = [(7, 7), (8, 10), (3, 16), (15, 20), (14, 21)]
SHIFTS = [0, 3, 6]
SCALE = 32 ** -0.5
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]
NAMES = ("dq", "dk", "dv", "dbk", "dbv", "dtable")


def _grid():
    """(B, H, W, heads, shift, biases)"""
    g = [(2, H, W, heads, shift, biases) for (H, W) in SIZES for shift in SHIFTS for heads in (1, 3)
         for biases in (True, False)]
    g += [(1, H, W, 3, shift, biases) for (H, W) in SIZES for shift in SHIFTS for biases in (True, False)]
    return g


def _bf16_restatement(q, k, v, bq, bk, bv, table, B, H, W, heads, shift, scale):
    """window_attention_ref's steps in plain torch bf16 (CPU): bf16 windows, S = Q K^T in bf16,
    scale / bias / mask and the softmax in float32, P rounded to bf16, O = P V in bf16."""
    C = q.shape[1]
    hd = C // heads
    Hp, Wp = -(-H // WS) * WS, -(-W // WS) * WS
    nwy, nwx = Hp // WS, Wp // WS

    def windows(x, bias):
        row = torch.zeros(C, dtype=torch.bfloat16) if bias is None else bias.to(torch.bfloat16)
        m = torch.cat([torch.cat([x.view(B, H, W, C), row.expand(B, H, Wp - W, C)], 2),
                       row.expand(B, Hp - H, Wp, C)], 1)
        if shift > 0:
            m = torch.roll(m, shifts=(-shift, -shift), dims=(1, 2))
        m = m.view(B, nwy, WS, nwx, WS, heads, hd).permute(0, 1, 3, 5, 2, 4, 6)
        return m.reshape(B, nwy, nwx, heads, WS * WS, hd)

    Q, K, V = windows(q, bq), windows(k, bk), windows(v, bv)
    t = torch.arange(WS * WS)
    ty, tx = t // WS, t % WS
    idx = (ty[:, None] - ty[None, :] + WS - 1) * (2 * WS - 1) + (tx[:, None] - tx[None, :] + WS - 1)
    bias = table[idx.reshape(-1)].view(WS * WS, WS * WS, heads).permute(2, 0, 1)
    S = (Q @ K.transpose(-1, -2)).float() * float(scale) + bias
    if shift > 0:
        reg = 3 * _region(Hp, shift)[:, None] + _region(Wp, shift)[None, :]
        reg = reg.view(nwy, WS, nwx, WS).permute(0, 2, 1, 3).reshape(nwy, nwx, WS * WS)
        differ = reg[:, :, :, None] != reg[:, :, None, :]
        S = S + (-100.0 * differ.float())[None, :, :, None]
    O = torch.softmax(S, dim=-1).to(torch.bfloat16) @ V
    O = O.view(B, nwy, nwx, heads, WS, WS, hd).permute(0, 1, 4, 2, 5, 3, 6).reshape(B, Hp, Wp, C)
    if shift > 0:
        O = torch.roll(O, shifts=(shift, shift), dims=(1, 2))
    return O[:, :H, :W].reshape(B * H * W, C)


def _grads(fn, dtype, qkv, b3, table, dout, key):
    """(dq, dk, dv, dbk, dbv, dtable) in float64 of ``fn`` run on leaves of ``dtype``."""
    B, H, W, heads, shift, _ = key
    C = 32 * heads
    q, k, v = (qkv[:, i * C:(i + 1) * C].to(dtype).clone().requires_grad_() for i in range(3))
    bs = [None] * 3 if b3 is None else [b.to(dtype).clone().requires_grad_() for b in b3]
    tab = table.to(torch.float64 if dtype == torch.float64 else torch.float32).clone().requires_grad_()
    out = fn(q, k, v, *bs, tab, B, H, W, heads, shift, SCALE)
    out.backward(dout.to(out.dtype))
    zero = torch.zeros(C, dtype=torch.float64)
    if b3 is not None:  # the cropped output rows: no gradient reaches the q bias
        assert bs[0].grad is None or float(bs[0].grad.abs().max()) == 0.0
    return (q.grad.double(), k.grad.double(), v.grad.double(), zero if b3 is None else bs[1].grad.double(),
            zero if b3 is None else bs[2].grad.double(), tab.grad.double())


@functools.lru_cache(maxsize=None)
def _cases(dtype):
    """Inputs (CPU, rounded to ``dtype``), the float64 gradients and, in bf16, the restatement's own
    error per gradient; computed once per dtype and shared by the tests (never modified)."""
    out = []
    for n, key in enumerate(_grid()):
        B, H, W, heads, shift, biases = key
        g = torch.Generator().manual_seed(2000 + n)
        C = 32 * heads
        rows = B * H * W
        qkv = torch.randn((rows, 3 * C), generator=g).to(dtype)
        table = torch.randn((169, heads), generator=g) * 0.5
        b3 = torch.randn((3, C), generator=g) * 0.5 if biases else None
        dout = torch.randn((rows, C), generator=g).to(dtype)
        bref = None if b3 is None else b3.to(dtype)  # the kernel rounds the padded positions' biases
        want = _grads(window_attention_ref, torch.float64, qkv, bref, table, dout, key)
        own = None
        if dtype == torch.bfloat16:
            re = _grads(_bf16_restatement, torch.bfloat16, qkv, bref, table, dout, key)
            own = [float((a - w).abs().max()) for a, w in zip(re, want)]
        out.append(dict(key=key, qkv=qkv, table=table, b3=b3, dout=dout, want=want, own=own))
    return out


def _call(pool, case, dtype, layout):
    """One kernel call on guarded operands.  layout: "fused" (slices of [rows, 3C] buffers),
    "separate" (three dense tensors each), "padded" (separate, ldd = C + 16 bytes).  Returns the six
    outputs (dbk / dbv None when the biases are NULL)."""
    from rgbd_amd import _lib
    from rgbd_amd.dense import _CODE
    from rgbd_amd.ops import _p, _stream
    key = case["key"]
    B, H, W, heads, shift, biases = key
    C = 32 * heads
    rows = B * H * W
    qkv = case["qkv"].to(DEV)
    esz = qkv.element_size()
    if layout == "fused":
        buf = pool.place(qkv, "qkv")
        q, k, v, ldq = buf[:, :C], buf[:, C:2 * C], buf[:, 2 * C:], 3 * C
        dbuf = pool.new((rows, 3 * C), dtype, DEV, tag=f"dqkv {key}").payload
        dq, dk, dv, ldd = dbuf[:, :C], dbuf[:, C:2 * C], dbuf[:, 2 * C:], 3 * C
    else:
        q, k, v = (pool.place(qkv[:, i * C:(i + 1) * C].contiguous(), "qkv"[i]) for i in range(3))
        ldq = C
        ldd = C + (16 // esz if layout == "padded" else 0)
        dq, dk, dv = (pool.new((rows, C), dtype, DEV, tag=f"d{n} {key}", strides=(ldd, 1) if ldd > C else None).payload
                      for n in "qkv")
    bq = bk = bv = dbk = dbv = None
    if biases:
        bq, bk, bv = (pool.place(b.to(DEV), "bias") for b in case["b3"])
        dbk, dbv = (pool.new((C,), torch.float32, DEV, tag=f"{n} {key}").payload for n in ("dbk", "dbv"))
    table = pool.place(case["table"].to(DEV), "table")
    dout = pool.place(case["dout"].to(DEV), "dout")
    dtable = pool.new((169, heads), torch.float32, DEV, tag=f"dtable {key}").payload
    L = _lib.lib()
    ws = pool.new((L.rgbd_swin_window_attn_bwd_workspace_size(B, H, W, heads),), torch.uint8, DEV, tag=f"ws {key}").payload
    rc = L.rgbd_swin_window_attn_bwd(_CODE[dtype], _p(q), _p(k), _p(v), ldq, _p(bq), _p(bk), _p(bv), _p(table),
                                     _p(dout), C, B, H, W, heads, 7, shift, SCALE, _p(dq), _p(dk), _p(dv), ldd,
                                     _p(dbk), _p(dbv), _p(dtable), _p(ws), _stream(DEV))
    assert rc == 0, (rc, key)
    return dq, dk, dv, dbk, dbv, dtable


def _fractions(got, case, dtype):
    """[(|err| / bar, |err|, name)] of one case."""
    res = []
    for i, (a, w, name) in enumerate(zip(got, case["want"], NAMES)):
        if a is None:
            continue
        assert torch.isfinite(a).all(), (case["key"], name)  # no cell left unwritten, no guard value read
        err = float((a.double().cpu() - w).abs().max())
        wmax = float(w.abs().max())
        bar = 1e-5 * (1 + wmax) if dtype == torch.float32 else 1.5 * case["own"][i] + 1e-3 * wmax
        res.append((err / bar if bar > 0 else (0.0 if err == 0 else float("inf")), err, name))
    return res


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_window_attention_bwd_vs_float64(dtype):
    """The whole grid in swin.py's layout.  Measured on an MI355X over the 90 cases: float32 max |err|
    dq 1.07e-6, dk 1.34e-6, dv 1.10e-6, dbk 8.7e-7, dbv 1.81e-6, dtable 5.37e-6, worst 0.049 of the
    bar (dk at B = 2, 15x20, 1 head, shift 3); bf16 max |err| dq 1.48e-2, dk 1.46e-2, dv 1.56e-2,
    dbk 8.7e-3, dbv 6.0e-3, dtable 4.0e-2, worst 0.91 of the bar (dk at B = 2, 7x7, 3 heads, shift 6,
    where the torch bf16 restatement's own error is smallest)."""
    pool = guard.Pool()
    cases = _cases(dtype)
    outs = [_call(pool, c, dtype, "fused") for c in cases]
    n = pool.check_all()
    worst, where, worst_abs = 0.0, None, {}
    for got, c in zip(outs, cases):
        B, H, W, heads, shift, biases = c["key"]
        for frac, err, name in _fractions(got, c, dtype):
            worst_abs[name] = max(worst_abs.get(name, 0.0), err)
            if frac > worst:
                worst, where = frac, (c["key"], name)
        if biases and H % 7 == 0 and W % 7 == 0:
            assert not got[3].any() and not got[4].any(), f"{c['key']}: dbk / dbv not exactly zero without padding"
    print(f"swin window attention backward {dtype}: {len(outs)} cases, {n} guarded buffers clean, worst |err| / bar "
          f"{worst:.3g} at ((B, H, W, heads, shift, biases), gradient) = {where}; max |err| per gradient "
          + ", ".join(f"{k} {v:.3g}" for k, v in worst_abs.items()))
    assert worst <= 1.0, f"{where}: |err| is {worst:.3g} x the bar"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("layout", ["separate", "padded"])
def test_window_attention_bwd_layouts(dtype, layout):
    """ldq = ldd = C and ldd > C: the same bars and the same bits as the fused layout, gap columns
    and guards untouched."""
    pool = guard.Pool()
    cases = _cases(dtype)
    outs = [_call(pool, c, dtype, layout) for c in cases]
    base = [_call(pool, c, dtype, "fused") for c in cases]
    pool.check_all()
    for got, b, c in zip(outs, base, cases):
        for frac, _, name in _fractions(got, c, dtype):
            assert frac <= 1.0, f"{c['key']} {name}: |err| is {frac:.3g} x the bar"
        for a, e, name in zip(got, b, NAMES):
            assert (a is None and e is None) or torch.equal(a, e), f"{c['key']} {name}: differs from the fused layout"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_window_attention_bwd_is_bitwise_reproducible(dtype):
    """Two calls on the same inputs (fresh NaN-filled outputs and workspaces) agree bitwise: the
    reductions over images and windows run in a fixed order, without float atomics."""
    pool = guard.Pool()
    cases = _cases(dtype)[::3]
    one = [_call(pool, c, dtype, "fused") for c in cases]
    two = [_call(pool, c, dtype, "fused") for c in cases]
    pool.check_all()
    for a, b, c in zip(one, two, cases):
        for x, y, name in zip(a, b, NAMES):
            assert (x is None and y is None) or torch.equal(x, y), (c["key"], name)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_wrapper_and_function_allocate_what_the_kernel_needs(dtype):
    """swin.WindowAttentionFunction's backward under guarded allocation: its output buffers and
    workspace stay inside their guards and hold the bits of the direct call; the [3C] bias gradient
    has a zero q part."""
    from rgbd_amd import swin
    pool = guard.Pool()
    for c in _cases(dtype)[::11]:
        B, H, W, heads, shift, biases = c["key"]
        C = 32 * heads
        direct = _call(pool, c, dtype, "fused")
        qkv = c["qkv"].to(DEV).requires_grad_()
        b = None if c["b3"] is None else c["b3"].reshape(-1).to(DEV).requires_grad_()
        table = c["table"].to(DEV).requires_grad_()
        with guard.guarded_allocations() as sweep:
            out = swin.WindowAttentionFunction.apply(qkv, b, table, B, H, W, heads, shift, SCALE)
            out.backward(c["dout"].to(DEV))
            assert sweep.check_all() >= 5
        assert torch.equal(qkv.grad, torch.cat(direct[:3], 1)), c["key"]
        assert torch.equal(table.grad, direct[5]), c["key"]
        if biases:
            assert not b.grad[:C].any()
            assert torch.equal(b.grad[C:2 * C], direct[3]) and torch.equal(b.grad[2 * C:], direct[4]), c["key"]
    pool.check_all()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gelu_and_its_gradient_vs_float64(dtype):
    """rgbd_gelu / rgbd_gelu_bwd on a length with a tail (3 blocks + 5) inside guards, against
    float64 erf GELU and its autograd gradient.  The arithmetic is float32 with one rounding to the
    operand dtype: 2e-6 * (1 + max) in float32, 2^-8 relative to the max in bf16."""
    from rgbd_amd import dense
    n = 3 * 2048 + 5
    g = torch.Generator().manual_seed(5)
    u = (torch.randn((n,), generator=g) * 2).to(dtype)
    dm = torch.randn((n,), generator=g).to(dtype)
    u64 = u.double().requires_grad_()
    m64 = torch.nn.functional.gelu(u64)
    m64.backward(dm.double())
    with guard.guarded_allocations() as sweep:
        ud, dd = sweep.place(u.to(DEV)), sweep.place(dm.to(DEV))
        m = dense.gelu(ud)
        du = dense.gelu_bwd(ud, dd)
        assert sweep.check_all() == 4
    for got, want, name in ((m, m64.detach(), "gelu"), (du, u64.grad, "gelu_bwd")):
        err = float((got.double().cpu() - want).abs().max())
        bar = 2e-6 * (1 + float(want.abs().max())) if dtype == torch.float32 else 2.0 ** -8 * float(want.abs().max())
        print(f"{name} {dtype}: max |err| {err:.3g}, bar {bar:.3g}")
        assert torch.isfinite(got).all() and err <= bar, name
