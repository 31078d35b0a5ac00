"""Deterministic mode on the GPU: the atomic-free MSDA value gradient (csrc/msda.hip) and
point-sample gradient (csrc/point_loss.hip), and the whole drop-in model with the switch on.

Every case is checked five ways:
1. bitwise against tests/checkers/ordered_scatter.py (the documented summation order in numpy
   float32) fed the kernel's own emitted keys and coefficients — the test that pins the order;
2. the other gradients (MSDA: gloc, gattw) bitwise equal to the default path's;
3. against the default (float-atomic) path, which sums the same float32 terms in another order:
   per element |det - atomic| <= (2 n + 2) 2^-24 A, n the case's longest segment, A the same
   backward run on |gout| with |attw| (the sequential-sum error bound, once for each side);
4. against the library reference (HF's multi_scale_deformable_attention / grid_sample backward)
   with the bars of tests/test_gpu_msda.py (1e-4 float32, 2e-2 bf16) and
   tests/test_gpu_point_loss.py (1e-5);
5. three runs give torch.equal results.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from transformers.models.mask2former.modeling_mask2former import multi_scale_deformable_attention as hf_msda

from checkers import guard
from checkers import ordered_scatter as osc
from rgbd_amd import deform_attn, determinism, ops, point_loss
from test_gpu_guard_bands import _model, _same_bits, _sweep
from test_gpu_msda import _encoder_locations, _inputs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32, BF16 = torch.float32, torch.bfloat16
U = 2.0 ** -24

ENC = (2, [(30, 40), (15, 20), (8, 10)], 8, 32, 4, 1580)
MSDA_CASES = {
    "ragged64": ((2, [(7, 9), (4, 5), (2, 3)], 4, 64, 3, 50), "random", 0.0, F32),
    "single16": ((1, [(16, 12)], 2, 16, 2, 33), "random", 0.0, F32),
    "enc_j0_f32": (ENC, "encoder", 0.0, F32),
    "enc_j0_bf16": (ENC, "encoder", 0.0, BF16),
    "enc_j0.3_f32": (ENC, "encoder", 0.3, F32),
    "enc_j0.3_bf16": (ENC, "encoder", 0.3, BF16),
    # every location within 1e-3 of (0.5, 0.5): 4 cells per level receive everything, about
    # Q * P = 600 > 2 * CH taps per segment, so the chunked order runs
    "collapsed": ((1, [(6, 8), (3, 4)], 2, 32, 2, 300), "collapsed", 0.0, F32),
}
FULL = [k for k in MSDA_CASES if k != "collapsed"]


def _msda_inputs(name):
    (B, shapes, NH, D, P, Q), kind, jitter, dt = MSDA_CASES[name]
    L = len(shapes)
    if kind == "random":
        value, loc, attw = _inputs(B, shapes, NH, D, P, Q, dtype=dt)
        g = torch.Generator(device=DEV).manual_seed(9)
    else:
        g = torch.Generator(device=DEV).manual_seed(5)
        S = sum(h * w for h, w in shapes)
        value = torch.randn((B, S, NH, D), generator=g, device=DEV).to(dt)
        if kind == "encoder":
            loc = _encoder_locations(B, shapes, NH, P, g, jitter)
        else:
            loc = 0.5 + (torch.rand((B, Q, NH, L, P, 2), generator=g, device=DEV) - 0.5) * 2e-3
        attw = torch.softmax(torch.randn((B, Q, NH, L * P), generator=g, device=DEV), -1).view(B, Q, NH, L, P)
    go = torch.randn((B, Q, NH * D), generator=g, device=DEV)
    return value, shapes, loc.contiguous(), attw, go


@functools.lru_cache(maxsize=None)
def _msda(name):
    """One case's inputs, deterministic stages, default-path result and restatement, computed once."""
    value, shapes, loc, attw, go = _msda_inputs(name)
    B, S, NH, D = value.shape
    Q, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    st = ops.msda_backward_stages(value, shapes, loc, attw, go)
    atomic = ops.msda_backward(value, shapes, loc, attw, go)
    torch.cuda.synchronize()
    # the restatement: go rows per tap i = ((((b NH + h) Q + q) L + l) P + p) 4 + e
    i = np.arange(B * NH * Q * L * P * 4, dtype=np.int64)
    bhq = i // (L * P * 4)
    bh, q = bhq // Q, bhq % Q
    gon = go.to(value.dtype).float().view(B, Q, NH, D).cpu().numpy()
    rows = gon[bh // NH, q, bh % NH]
    want = osc.ordered_scatter(st["sorted_keys"].cpu().numpy(), st["sorted_idx"].cpu().numpy(),
                               st["coef"].cpu().numpy(), B * NH * S, rows=rows)
    want = torch.from_numpy(want.reshape(B, NH, S, D).transpose(0, 2, 1, 3).copy())
    n = int(osc.segment_lengths(st["sorted_keys"].cpu().numpy(), B * NH * S).max())
    return dict(inputs=(value, shapes, loc, attw, go), st=st, atomic=atomic, want=want, n=n)


@pytest.mark.parametrize("name", list(MSDA_CASES))
def test_msda_bitwise_equal_to_restatement(name):
    c = _msda(name)
    value, shapes, loc = c["inputs"][:3]
    B, S, NH, D = value.shape
    keys = c["st"]["keys"]
    sentinel = B * NH * S
    assert int(keys.min()) >= 0 and int(keys.max()) <= sentinel
    sk, si = c["st"]["sorted_keys"], c["st"]["sorted_idx"]
    assert bool((sk[1:] >= sk[:-1]).all()) and bool(((sk[1:] > sk[:-1]) | (si[1:] > si[:-1])).all()), "not a stable sort"
    got = c["st"]["gv"].cpu()
    print(f"{name}: {keys.numel()} taps, {int((keys == sentinel).sum())} padding, longest segment {c['n']}")
    if name == "collapsed":
        assert c["n"] > 2 * osc.CH
    assert _same_bits(got, c["want"]), f"max |gpu - restatement| = {float((got - c['want']).abs().max()):.3g}"


@pytest.mark.parametrize("name", FULL)
def test_msda_gloc_gattw_bitwise_default(name):
    c = _msda(name)
    assert _same_bits(c["st"]["gl"], c["atomic"][1]) and _same_bits(c["st"]["ga"], c["atomic"][2])


@pytest.mark.parametrize("name", list(MSDA_CASES))
def test_msda_value_gradient_against_atomic_path(name):
    c = _msda(name)
    value, shapes, loc, attw, go = c["inputs"]
    A = ops.msda_backward(value, shapes, loc, attw.abs(), go.to(value.dtype).abs())[0].double()
    bound = (2 * c["n"] + 2) * U * A
    diff = (c["st"]["gv"].double() - c["atomic"][0].double()).abs()
    ratio = float((diff / bound.clamp_min(1e-300)).max())
    print(f"{name}: longest segment {c['n']}, max |det - atomic| / bound = {ratio:.4f}, "
          f"max |det - atomic| = {float(diff.max()):.3g}")
    assert bool((diff <= bound).all()), ratio


@pytest.mark.parametrize("name", FULL)
def test_msda_against_hf_backward(name):
    c = _msda(name)
    value, shapes, loc, attw, go = c["inputs"]
    vr, lr, ar = (t.clone().float().requires_grad_(True) for t in (value, loc, attw))
    (hf_msda(vr, shapes, lr, ar) * go.to(value.dtype).float()).sum().backward()
    tol = 1e-4 if value.dtype == F32 else 2e-2
    for a, b, what in ((c["st"]["gv"], vr.grad, "value"), (c["st"]["gl"], lr.grad, "loc"), (c["st"]["ga"], ar.grad, "attw")):
        err = float((a.float() - b).abs().max()) / (float(b.abs().max()) + 1e-12)
        print(f"{name} {what}: {err:.3g}")
        assert err < tol, (what, err)


@pytest.mark.parametrize("name", list(MSDA_CASES))
def test_msda_three_runs_equal(name):
    c = _msda(name)
    value, shapes, loc, attw, go = c["inputs"]
    for _ in range(3):
        got = ops.msda_backward(value, shapes, loc, attw, go, deterministic=True)
        for a, b in zip(got, (c["st"]["gv"], c["st"]["gl"], c["st"]["ga"])):
            assert torch.equal(a, b)


def test_msda_autograd_runs_backward_in_the_forwards_mode():
    """The switch is read in forward and kept on ctx: forward inside the context and backward
    outside it (and the other way round) use the forward's mode."""
    c = _msda("enc_j0.3_f32")
    value, shapes, loc, attw, go = c["inputs"]
    assert not torch.equal(c["st"]["gv"], c["atomic"][0]), "the case does not tell the two modes apart"
    v = value.clone().requires_grad_(True)
    with determinism.deterministic():
        out = deform_attn.multi_scale_deformable_attention(v, shapes, loc, attw)
    out.backward(go)
    assert torch.equal(v.grad, c["st"]["gv"])
    v = value.clone().requires_grad_(True)
    with determinism.deterministic(False):
        out = deform_attn.multi_scale_deformable_attention(v, shapes, loc, attw)
    with determinism.deterministic():
        out.backward(go)
    bound = (2 * c["n"] + 2) * U * ops.msda_backward(value, shapes, loc, attw.abs(), go.abs())[0]
    assert bool(((v.grad - c["atomic"][0]).abs() <= bound).all())


def test_msda_all_outside_writes_exact_zeros():
    """loc = 2.0: every tap is padding.  The output buffers come NaN-filled (0xFF guard payloads);
    the gather must write +0 into every element of gvalue without a memset."""
    (B, shapes, NH, D, P, Q), _, _, _ = MSDA_CASES["ragged64"]
    value, loc, attw = _inputs(B, shapes, NH, D, P, Q)
    loc = torch.full_like(loc, 2.0)
    go = torch.randn((B, Q, NH * D), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    with guard.guarded_allocations() as sw:
        probe = ops.torch.empty((4,), dtype=F32, device=DEV)
        assert bool(torch.isnan(probe).all()), "the harness no longer poisons torch.empty"
        gv, gl, ga = ops.msda_backward(value, shapes, loc, attw, go, deterministic=True)
        sw.check_all()
    assert gv.shape == value.shape and bool((gv.view(torch.int32) == 0).all()), "gvalue is not +0 everywhere"
    assert bool((gl == 0).all()) and bool((ga == 0).all())


@pytest.mark.parametrize("images_per_group", [1, 2], ids=["1+1+1", "2+1"])
def test_msda_batch_split_changes_no_bit(monkeypatch, images_per_group):
    (_, shapes, NH, D, P, Q), _, _, _ = MSDA_CASES["ragged64"]
    B, L = 3, len(shapes)
    value, loc, attw = _inputs(B, shapes, NH, D, P, Q, seed=4)
    go = torch.randn((B, Q, NH * D), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    whole = ops.msda_backward(value, shapes, loc, attw, go, deterministic=True)
    per_image = NH * Q * L * P * 4
    monkeypatch.setattr(ops, "MSDA_DET_MAX_TAPS", images_per_group * per_image + per_image // 2)
    assert ops._msda_det_group(B, value.shape[1], NH, Q, L, P) == images_per_group
    split = ops.msda_backward(value, shapes, loc, attw, go, deterministic=True)
    for a, b in zip(split, whole):
        assert _same_bits(a, b)


def test_msda_deterministic_backward_is_capturable():
    """One torch.cuda.graph capture of the three stages (no host synchronisation, nothing read
    back), replayed twice: each replay bitwise the eager result."""
    c = _msda("ragged64")
    value, shapes, loc, attw, go = c["inputs"]
    eager = ops.msda_backward(value, shapes, loc, attw, go, deterministic=True)  # also the warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ops.msda_backward(value, shapes, loc, attw, go, deterministic=True)
    for _ in range(2):
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(captured, eager):
            assert _same_bits(a, b)


def test_msda_guard_bands():
    value, shapes, loc, attw, go = _msda("ragged64")["inputs"]
    _sweep(lambda v, l, a, g: ops.msda_backward(v, shapes, l, a, g, deterministic=True), value, loc, attw, go)
    value, shapes, loc, attw, go = _msda("enc_j0.3_bf16")["inputs"]
    _sweep(lambda v, l, a, g: ops.msda_backward(v, shapes, l, a, g, deterministic=True), value, loc, attw, go)


# ------------------------------------------------------------------ point sample
POINT_CASES = {"5x5_6x7_37": (5, 5, 6, 7, 37), "6x3_13x9_300": (6, 3, 13, 9, 300), "edges_copies": (4, 2, 5, 6, 64)}


def _point_inputs(name):
    N, G, h, w, P = POINT_CASES[name]
    g = torch.Generator(device=DEV).manual_seed(N * 7 + P)
    maps = torch.randn((N, h, w), generator=g, device=DEV)
    coords = torch.rand((G, P, 2), generator=g, device=DEV)
    if name == "edges_copies":  # 50 copies of one point, and points at exactly 0 and 1
        coords[:, :50] = torch.tensor([0.37, 0.61], device=DEV)
        coords[:, 50:54] = torch.tensor([[0.0, 0.0], [1.0, 1.0], [0.0, 1.0], [1.0, 0.0]], device=DEV)
    go = torch.randn((N, P), generator=g, device=DEV)
    return maps, coords, go


def _point_atomic(maps, coords, go):
    m = maps.clone().requires_grad_(True)
    with determinism.deterministic(False):
        point_loss.point_sample(m, coords).backward(go)
    return m.grad


@functools.lru_cache(maxsize=None)
def _point(name):
    maps, coords, go = _point_inputs(name)
    N, h, w = maps.shape
    st = point_loss.point_sample_backward_stages(go, coords, h, w)
    atomic = _point_atomic(maps, coords, go)
    torch.cuda.synchronize()
    sk = st["sorted_keys"].cpu().numpy()
    want = osc.ordered_scatter(sk, st["sorted_idx"].cpu().numpy(), st["coef"].cpu().numpy(), N * h * w)
    n = int(osc.segment_lengths(sk, N * h * w).max())
    return dict(inputs=(maps, coords, go), st=st, atomic=atomic, want=torch.from_numpy(want).view(N, h, w), n=n)


@pytest.mark.parametrize("name", list(POINT_CASES))
def test_point_bitwise_equal_to_restatement(name):
    c = _point(name)
    N, h, w = c["inputs"][0].shape
    keys = c["st"]["keys"]
    assert int(keys.min()) >= 0 and int(keys.max()) <= N * h * w
    print(f"{name}: {keys.numel()} taps, {int((keys == N * h * w).sum())} outside, longest segment {c['n']}")
    if name == "edges_copies":
        assert c["n"] >= 50
    assert _same_bits(c["st"]["gmaps"].cpu(), c["want"])


@pytest.mark.parametrize("name", list(POINT_CASES))
def test_point_gradient_against_atomic_path(name):
    c = _point(name)
    maps, coords, go = c["inputs"]
    A = _point_atomic(maps, coords, go.abs()).double()
    bound = (2 * c["n"] + 2) * U * A
    diff = (c["st"]["gmaps"].double() - c["atomic"].double()).abs()
    ratio = float((diff / bound.clamp_min(1e-300)).max())
    print(f"{name}: longest segment {c['n']}, max |det - atomic| / bound = {ratio:.4f}")
    assert bool((diff <= bound).all()), ratio


@pytest.mark.parametrize("name", list(POINT_CASES))
def test_point_against_grid_sample_backward(name):
    c = _point(name)
    maps, coords, go = c["inputs"]
    N, G = maps.shape[0], coords.shape[0]
    mref = maps.clone().requires_grad_(True)
    ref_c = coords.repeat_interleave(N // G, dim=0)
    F.grid_sample(mref[:, None], 2.0 * ref_c[:, :, None] - 1.0, align_corners=False)[:, 0, :, 0].backward(go)
    err = float((c["st"]["gmaps"] - mref.grad).abs().max() / (mref.grad.abs().max() + 1e-12))
    print(f"{name}: {err:.3g}")
    assert err <= 1e-5


@pytest.mark.parametrize("name", list(POINT_CASES))
def test_point_three_runs_equal_through_autograd(name):
    c = _point(name)
    maps, coords, go = c["inputs"]
    for _ in range(3):
        m = maps.clone().requires_grad_(True)
        with determinism.deterministic():
            out = point_loss.point_sample(m, coords)
        out.backward(go)  # outside the context: the forward's mode holds
        assert torch.equal(m.grad, c["st"]["gmaps"])


def test_point_guard_bands():
    for name in POINT_CASES:
        maps, coords, go = _point(name)["inputs"]
        h, w = maps.shape[1:]
        _sweep(lambda g, c: point_loss.point_sample_backward_stages(g, c, h, w)["gmaps"], go, coords)


# ------------------------------------------------------------------ whole model
@pytest.mark.parametrize("amp", [False, True], ids=["f32", "bf16_autocast"])
def test_whole_model_train_step_is_bitwise_reproducible(amp):
    """standard_config(48), 320x240, B = 2, the switch on: two training steps from the same state,
    seeds and inputs give the same loss bits and torch.equal gradients for every parameter, and a
    step under the guard-band harness gives them too."""
    import golden_inputs as gi
    m, state = _model()
    m.set_compute_dtype(BF16 if amp else F32)
    rp = m.model.pixel_level_module.ratio_predictor
    H, W, B = 240, 320, 2
    pv0 = torch.from_numpy(gi.pixel_values(6, B, H, W)).to(DEV)
    masks, classes = gi.labels(6, B, H, W)
    ml0 = [torch.from_numpy(x).to(DEV) for x in masks]
    cl0 = [torch.from_numpy(c).to(DEV) for c in classes]

    def step(pv, ml, cl):
        m.load_state_dict(state)
        m.zero_grad(set_to_none=True)
        rp._rgbd_dropout_seed = 0x5EED
        rp._rgbd_dropout_ctr = torch.zeros((1,), dtype=torch.int64, device=DEV)
        torch.manual_seed(1234)
        with determinism.deterministic():
            with torch.autocast("cuda", dtype=BF16, enabled=amp):
                out = m(pixel_values=pv, mask_labels=ml, class_labels=cl)
            out.loss.backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
        assert grads and all(torch.isfinite(g).all() for g in grads.values())
        return out.loss.detach().clone(), grads

    la, ga = step(pv0, ml0, cl0)
    lb, gb = step(pv0, ml0, cl0)
    with guard.guarded_allocations() as sw:
        lg, gg = step(sw.place(pv0, "pixel_values"), [sw.place(x, "mask_labels") for x in ml0],
                      [sw.place(c, "class_labels") for c in cl0])
        n = sw.check_all()
    print(f"whole model {'bf16 autocast' if amp else 'float32'} B={B}: loss {float(la)!r} / {float(lb)!r} / guarded "
          f"{float(lg)!r}; {len(ga)} gradients, {n} guarded buffers clean")
    for what, (l2, g2) in (("second run", (lb, gb)), ("guarded run", (lg, gg))):
        bad = [k for k in ga if not torch.equal(ga[k], g2[k])]
        assert _same_bits(la, l2), f"{what}: loss {float(l2)!r} vs {float(la)!r}"
        assert ga.keys() == g2.keys() and not bad, f"{what}: {len(bad)} of {len(ga)} gradients differ, first {bad[:5]}"
