"""Global-norm gradient clipping on the HIP optimizer step (csrc/adamw.hip: rgbd_grad_sumsq_multi,
rgbd_grad_norm_finalize, rgbd_adamw_multi_scaled, rgbd_scale_multi; rgbd_amd.optim.HipAdamW(
max_grad_norm=...), clip_grad_norm_; rgbd_amd.trainer.HipClipTrainer) against float64 and against
torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(fused=True).

The tensor list is tests/test_gpu_adamw.py's (more tensors than one AdamW table, numel not a
multiple of 4, one element, one tensor of many chunks) plus a zero-element tensor, a gradient that
is a view starting 4 bytes into its storage (the 16-byte path must be declined) and a parameter
whose grad is None.

Error bound of the norm (NORM_RTOL).  The kernel squares and sums in double from the element on: a
float32 square is exact in double (48 <= 53 bits), and n additions in double err by at most
n * 2^-53 relative (3e6 * 1.1e-16 = 3.3e-10 here, all terms positive).  So the longest serial
float32 chain is k = 0 and no float32 tree stage exists; the only float32 rounding is the final
cast of sqrt(total): 2^-24.  NORM_RTOL = 2^-24 + 1e-9 = 6.06e-8 (issue's ceiling: 1e-5).
Measured: the figures in DESIGN.md §5.14.

Moment bars (test 2): rtol 1e-6 with atol 1e-7 (parameters) / 1e-12 (exp_avg_sq) as in
tests/test_gpu_adamw.py.  exp_avg is a signed sum, so an element can cancel to far below its terms
and needs an absolute term: the two arms' coefficients differ by at most the two norms' float32
errors, <= 4 * 2^-24 = 2.4e-7 relative (ours 2^-24, torch's float32 reduction a few ulp), times the
largest clipped gradient element, 6 sigma / ||g|| <= 6 / 1600 = 3.8e-3 when clipped to norm 1:
9e-10, rounded up to 1e-9."""
import ctypes

import pytest
import torch

import _rgbd_import  # noqa: F401
from checkers import guard

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SHAPES = [(768, 384, 3, 3), (4, 768), (192, 96, 3, 3), (4097,), (1,), (3, 5, 7)] + [(33,)] * 50
EXTRA = [(0,)]          # a zero-element tensor
OFFSET_AT = 3           # the (4097,) gradient is a view 4 bytes into its storage
ALL = SHAPES + EXTRA
NORM_RTOL = 2.0 ** -24 + 1e-9
MAX_NORM = 1.0
_base = {}


def _base_grads(seed):
    """Unit-variance gradients for ALL (CPU, generated once per seed and never modified)."""
    if seed not in _base:
        g = torch.Generator(device="cpu").manual_seed(seed)
        _base[seed] = [torch.randn(s, generator=g) for s in ALL]
    return _base[seed]


def _params(seed=0):
    """Parameters for ALL plus one that never gets a gradient (last)."""
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    return [torch.randn(s, generator=g).to(DEV).requires_grad_() for s in ALL + [(17,)]]


def _clone(params):
    return [p.detach().clone().requires_grad_() for p in params]


def _offset_view(t):
    """t's values in a tensor whose first element sits 4 bytes into a fresh allocation."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _set_grads(params, base, scale, offset=True):
    """params[i].grad = base[i] * scale (fresh tensors); the last parameter keeps grad None."""
    for i, (p, b) in enumerate(zip(params, base)):
        t = (b * scale).to(DEV)
        p.grad = _offset_view(t) if (offset and i == OFFSET_AT) else t
    assert params[-1].grad is None


def _norm64(params):
    return float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params if p.grad is not None)))


def _bits(t):
    return t.detach().contiguous().view(-1).view(torch.uint8)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _close_state(a, b, oa, ob):
    for pa, pb in zip(a, b):
        if pa.grad is None:
            continue
        torch.testing.assert_close(pa, pb, rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(oa.state[pa]["exp_avg"], ob.state[pb]["exp_avg"], rtol=1e-6, atol=1e-9)
        torch.testing.assert_close(oa.state[pa]["exp_avg_sq"], ob.state[pb]["exp_avg_sq"], rtol=1e-6, atol=1e-12)


def test_norm_against_float64():
    """1. opt.grad_norm and clip_grad_norm_'s return against sqrt(sum(g.double()**2)), at norms
    far above, near and below max_norm."""
    from rgbd_amd.optim import HipAdamW, clip_grad_norm_
    base = _base_grads(1)
    a = _params()
    opt = HipAdamW(a, lr=1e-5, max_grad_norm=MAX_NORM)
    worst = 0.0
    for scale in (1.0, 37.0, 6e-4, 1e-4):
        _set_grads(a, base, scale)
        ref = _norm64(a)
        opt.step()
        e_step = abs(float(opt.grad_norm.double()) - ref) / ref
        got = clip_grad_norm_(a, MAX_NORM)
        assert got.shape == () and got.is_cuda and got.dtype == torch.float32
        e_fn = abs(float(got.double()) - ref) / ref
        print(f"scale {scale:g}: float64 norm {ref:.9g}, rel err step {e_step:.3g}, clip_grad_norm_ {e_fn:.3g}")
        worst = max(worst, e_step, e_fn)
        assert e_step <= NORM_RTOL and e_fn <= NORM_RTOL
    print(f"worst relative norm error {worst:.3g} (bound {NORM_RTOL:.3g})")


def test_moments_and_parameters_against_torch():
    """2. Four steps, three that clip (norm >> max_norm) and one that does not (norm 0.17):
    parameters, exp_avg and exp_avg_sq against clip_grad_norm_ + AdamW(fused); p.grad untouched by
    the fused step; the unclipped HipAdamW on the same inputs misses the exp_avg_sq bar."""
    from rgbd_amd.optim import HipAdamW
    base = _base_grads(2)
    a = _params()
    b, c = _clone(a), _clone(a)
    oa = HipAdamW(a, lr=1e-3, weight_decay=0.05, max_grad_norm=MAX_NORM)
    ob = torch.optim.AdamW(b, lr=1e-3, weight_decay=0.05, fused=True)
    oc = HipAdamW(c, lr=1e-3, weight_decay=0.05)
    clipped = []
    for scale in (1.0, 1e-4, 30.0, 0.01):
        for ps in (a, b, c):
            _set_grads(ps, base, scale, offset=ps is not b)
        before = [None if p.grad is None else p.grad.clone() for p in a]
        clipped.append(_norm64(a) > MAX_NORM)
        oa.step()
        torch.nn.utils.clip_grad_norm_(b, MAX_NORM)
        ob.step()
        oc.step()
        for p, g0 in zip(a, before):
            assert g0 is None or _same_bits(p.grad, g0), "the fused step wrote p.grad"
    assert clipped == [True, False, True, True]
    err_m = max(float(((oa.state[pa]["exp_avg"] - ob.state[pb]["exp_avg"]).abs()).max())
                for pa, pb in zip(a, b) if pa.grad is not None and pa.numel())
    rel_v = max(float(((oa.state[pa]["exp_avg_sq"] - ob.state[pb]["exp_avg_sq"]).abs()
                       / ob.state[pb]["exp_avg_sq"].abs().clamp_min(1e-30)).max())
                for pa, pb in zip(a, b) if pa.grad is not None and pa.numel())
    print(f"max |exp_avg - torch| {err_m:.3g}, max rel exp_avg_sq error {rel_v:.3g}")
    _close_state(a, b, oa, ob)
    assert float(oa.state[a[0]]["step"]) == 4.0 and a[-1] not in oa.state
    with pytest.raises(AssertionError):  # not vacuous: without the coefficient the moments are far off
        torch.testing.assert_close(oc.state[c[0]]["exp_avg_sq"], ob.state[b[0]]["exp_avg_sq"], rtol=1e-6, atol=1e-12)


def test_clip_grad_norm_leaves_torchs_gradients():
    """2 (stand-alone form). After clip_grad_norm_, p.grad equals torch's clipped gradients, when it
    clips and when it does not; the return is the pre-clip norm."""
    from rgbd_amd.optim import clip_grad_norm_
    base = _base_grads(2)
    a = _params()
    b = _clone(a)
    for scale in (3.0, 1e-4):
        _set_grads(a, base, scale)
        _set_grads(b, base, scale, offset=False)
        ref = _norm64(a)
        got = clip_grad_norm_(a, MAX_NORM)
        want = torch.nn.utils.clip_grad_norm_(b, MAX_NORM)
        assert abs(float(got.double()) - ref) / ref <= NORM_RTOL
        torch.testing.assert_close(got, want, rtol=1e-6, atol=0)
        for pa, pb in zip(a, b):
            if pb.grad is not None:
                torch.testing.assert_close(pa.grad, pb.grad, rtol=1e-6, atol=0)
        assert a[-1].grad is None


def _with_shadow(max_grad_norm_kw, steps):
    from rgbd_amd.dense import cast_weight
    from rgbd_amd.optim import HipAdamW
    torch.manual_seed(0)
    a = torch.nn.Parameter(torch.randn(1000, 37, device="cuda"))
    b = torch.nn.Parameter(torch.randn(4099, device="cuda"))  # no cast: no shadow
    opt = HipAdamW([a, b], lr=1e-2, **max_grad_norm_kw)
    c0 = cast_weight(a, torch.bfloat16)
    for _ in range(steps):
        a.grad = torch.randn_like(a)
        b.grad = torch.randn_like(b)
        opt.step()
        c = cast_weight(a, torch.bfloat16)
        assert c is c0
        assert torch.equal(c, a.detach().to(torch.bfloat16))
    assert getattr(b, "_rgbd_cast", None) is None
    return [a, b], opt


def test_max_grad_norm_none_is_todays_step():
    """3. max_grad_norm=None: parameters, moments and step count bitwise those of a HipAdamW built
    without the argument, after three steps, one parameter with a bf16 shadow."""
    p0, o0 = _with_shadow({}, 3)
    p1, o1 = _with_shadow(dict(max_grad_norm=None), 3)
    assert o1.grad_norm is None
    for x, y in zip(p0, p1):
        assert _same_bits(x, y)
        for k in ("exp_avg", "exp_avg_sq", "step"):
            assert _same_bits(o0.state[x][k], o1.state[y][k]), k
    assert float(o1.state[p1[0]]["step"]) == 3.0


def test_clipped_step_writes_the_bf16_shadow():
    """4. After clipped steps cast_weight returns the same tensor, bitwise p.to(bfloat16) (checked
    inside _with_shadow), and the step did clip."""
    _, opt = _with_shadow(dict(max_grad_norm=MAX_NORM), 2)
    assert float(opt.grad_norm) > 100 * MAX_NORM  # randn over 41 099 elements: about 203


def test_capture_and_replay():
    """5. One eager clipped step, then opt.step() captured with the gradients in static buffers
    and replayed three times on new gradients of very different norm (one below max_norm): the
    parameters and moments follow the torch arm stepped eagerly, and opt.grad_norm after each
    replay is that replay's float64 norm (a norm or coefficient baked in on the host would not)."""
    from rgbd_amd.optim import HipAdamW
    base = _base_grads(3)
    a = _params()
    b = _clone(a)
    oa = HipAdamW(a, lr=1e-3, weight_decay=0.01, max_grad_norm=MAX_NORM)
    ob = torch.optim.AdamW(b, lr=1e-3, weight_decay=0.01, fused=True)

    def torch_step():
        torch.nn.utils.clip_grad_norm_(b, MAX_NORM)
        ob.step()

    _set_grads(a, base, 1.0)
    _set_grads(b, base, 1.0, offset=False)
    oa.step()  # state, norm buffer allocated outside the capture
    torch_step()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            oa.step()
    torch.cuda.current_stream().wait_stream(s)
    for scale in (50.0, 2e-4, 0.3):
        for p, t in zip(a, base):
            p.grad.copy_((t * scale).to(DEV))  # into the static buffers the graph reads
        _set_grads(b, base, scale, offset=False)
        ref = _norm64(a)
        graph.replay()
        torch_step()
        torch.cuda.synchronize()
        got = float(oa.grad_norm.double())
        print(f"replay scale {scale:g}: grad_norm {got:.9g}, float64 {ref:.9g}")
        assert abs(got - ref) / ref <= NORM_RTOL
    _close_state(a, b, oa, ob)
    assert float(oa.state[a[0]]["step"]) == 4.0


def test_reproducible():
    """6. The norm of the same gradients on two streams (a fresh workspace each) is bitwise equal,
    and a clipped step from identical state gives bitwise equal parameters and moments."""
    from rgbd_amd.optim import HipAdamW, clip_grad_norm_
    base = _base_grads(4)
    a = _params()
    _set_grads(a, base, 2.5)
    before = [None if p.grad is None else p.grad.clone() for p in a]
    norms = []
    for _ in range(2):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            norms.append(clip_grad_norm_(a, float("inf")))  # coefficient exactly 1: gradients unchanged
        torch.cuda.current_stream().wait_stream(s)
    assert _same_bits(norms[0], norms[1])
    for p, g0 in zip(a, before):
        assert g0 is None or _same_bits(p.grad, g0)
    b = _clone(a)
    for p, q in zip(a, b):
        q.grad = None if p.grad is None else p.grad.clone()
    oa = HipAdamW(a, lr=1e-3, max_grad_norm=MAX_NORM)
    ob = HipAdamW(b, lr=1e-3, max_grad_norm=MAX_NORM)
    oa.step()
    ob.step()
    assert _same_bits(oa.grad_norm, ob.grad_norm) and _same_bits(oa.grad_norm, norms[0])
    for p, q in zip(a, b):
        assert _same_bits(p, q)
        if p.grad is not None:
            assert _same_bits(oa.state[p]["exp_avg"], ob.state[q]["exp_avg"])
            assert _same_bits(oa.state[p]["exp_avg_sq"], ob.state[q]["exp_avg_sq"])


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_non_finite_gradients_follow_torch(bad):
    """7. One NaN / one +inf gradient element: grad_norm and the gradients clip_grad_norm_ leaves
    equal torch's (NaN everywhere / zeros with one NaN).  Ordinary values to the kernels."""
    from rgbd_amd.optim import HipAdamW, clip_grad_norm_
    base = _base_grads(5)
    a = _params()
    b, c = _clone(a), _clone(a)
    for ps in (a, b, c):
        _set_grads(ps, base, 1.0, offset=ps is not b)
        ps[2].grad.view(-1)[12345] = bad
    got = clip_grad_norm_(a, MAX_NORM)
    want = torch.nn.utils.clip_grad_norm_(b, MAX_NORM)
    torch.testing.assert_close(got, want, rtol=1e-6, atol=0, equal_nan=True)
    for pa, pb in zip(a, b):
        if pb.grad is not None:
            torch.testing.assert_close(pa.grad, pb.grad, rtol=1e-6, atol=0, equal_nan=True)
    opt = HipAdamW(c, lr=1e-3, max_grad_norm=MAX_NORM)
    opt.step()
    torch.testing.assert_close(opt.grad_norm, want, rtol=1e-6, atol=0, equal_nan=True)


def _guarded_round(params, grads):
    """A clipped HipAdamW step, then clip_grad_norm_, on the given tensors: everything compared."""
    from rgbd_amd.optim import HipAdamW, clip_grad_norm_
    ps = [p.detach().requires_grad_() for p in params]
    for p, g in zip(ps, grads):
        p.grad = g
    opt = HipAdamW(ps, lr=1e-3, weight_decay=0.01, max_grad_norm=MAX_NORM)
    opt.step()
    norm_step = opt.grad_norm.clone()
    norm_fn = clip_grad_norm_(ps, 0.5)
    out = [norm_step, norm_fn]
    for p in ps:
        out += [p.detach(), p.grad, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]]
    return out


def test_guard_bands():
    """8. Norm + finalise + scaled step, then the in-place scale, with the parameters, gradients,
    moments, the two-float output and the partial workspace (exactly the queried size) between
    0xFF guards: every guard byte intact and all results bitwise those of the unguarded run."""
    from rgbd_amd import _lib
    base = _base_grads(6)
    params = [p.detach() for p in _params()[:-1]]
    grads = [(t * 3.0).to(DEV) for t in base]
    grads[OFFSET_AT] = _offset_view(grads[OFFSET_AT])
    with guard.guarded_allocations() as sw:
        gp = [sw.place(p, tag="param") for p in params]
        gg = [sw.place(g, tag="grad") for g in grads]
        # the misaligned gradient: still 4 bytes off a 16-byte boundary inside its guarded buffer
        # (the element in front of it stays 0xFF, a NaN)
        off = sw.new((grads[OFFSET_AT].numel() + 1,), torch.float32, DEV, tag="grad+4")
        gg[OFFSET_AT] = off.payload[1:].view(grads[OFFSET_AT].shape)
        gg[OFFSET_AT].copy_(grads[OFFSET_AT])
        assert gg[OFFSET_AT].data_ptr() % 16 == 4
        got = _guarded_round(gp, gg)
        n = sw.check_all()
        assert sw.passed_through == 0
        ws = {k[1]: v for k, v in sw.workspaces().items()}
    want_ws = 0
    for i in range(0, len(grads), 128):  # one query per table of 128, as the wrapper fills the array
        run = [g.numel() for g in grads[i:i + 128]]
        want_ws += _lib.lib().rgbd_grad_sumsq_workspace_size(len(run), (ctypes.c_longlong * len(run))(*run))
    assert want_ws == 8 * sum((g.numel() + 4095) // 4096 for g in grads) > 256
    assert ws["grad_norm"].numel() == want_ws, "the partial workspace is not exactly the queried size"
    want = _guarded_round([p.clone() for p in params], [g.clone() if i != OFFSET_AT else _offset_view(g)
                                                        for i, g in enumerate(grads)])
    assert len(got) == len(want)
    for i, (x, y) in enumerate(zip(got, want)):
        assert _same_bits(x, y), f"result {i} differs from the unguarded run"
    print(f"{n} guarded buffers clean, {len(got)} results bitwise equal, workspace {want_ws} bytes")


def test_trainer_hook(tmp_path):
    """9. HipClipTrainer over a tiny nn.Linear with gradients set by hand: _clip_grad_norm returns
    the pre-clip norm and leaves torch's clipped gradients."""
    from transformers import TrainingArguments
    from rgbd_amd.trainer import HipClipTrainer
    torch.manual_seed(0)
    model = torch.nn.Linear(37, 5).to(DEV)
    twin = torch.nn.Linear(37, 5).to(DEV)
    for p, q in zip(model.parameters(), twin.parameters()):
        p.grad = torch.randn_like(p)
        q.grad = p.grad.clone()
    args = TrainingArguments(output_dir=str(tmp_path), max_grad_norm=1.0, report_to=[])
    trainer = HipClipTrainer(model=model, args=args)
    ref = _norm64(list(model.parameters()))
    assert ref > 1.0
    got = trainer._clip_grad_norm(model)
    want = torch.nn.utils.clip_grad_norm_(twin.parameters(), args.max_grad_norm)
    assert abs(float(got.double()) - ref) / ref <= NORM_RTOL
    torch.testing.assert_close(got, want, rtol=1e-6, atol=0)
    for p, q in zip(model.parameters(), twin.parameters()):
        torch.testing.assert_close(p.grad, q.grad, rtol=1e-6, atol=0)
