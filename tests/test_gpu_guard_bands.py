"""No kernel writes outside the tensors and the workspace bytes its caller was told to provide,
and nothing read beyond an input reaches an output.

The write-side twin of tests/test_gpu_workspace_poison.py.  Outputs come from ``torch.empty`` /
``torch.zeros`` and scratch from ``ops._workspace`` (a cache that only grows), so a store past the
end of either lands in allocator slack, a neighbouring tensor or the tail of a workspace an
earlier, larger call left behind: no fault and no changed value.  Here whole paths run under
tests/checkers/guard.py: every buffer the wrappers allocate, every workspace (new, and exactly
the size the wrapper asked the ``*_size`` function for) and every test input sits between 0xFF
guard bands (NaN in float32 and bf16).  Each sweep asserts

(a) every guard byte is still 0xFF, and
(b) the results are bitwise those of the same call without the harness — so no output cell was
    left unwritten and no guard value was read.  Where a kernel sums with float atomics (the whole
    model's MSDA / point-sample backward) bitwise is replaced as that test says.

1. the hot-path training step and the ratio predictor's eval forward (ragged shapes, three
   precision modes);  2. the dense family through dense.py / conv.py / ops.py;  3. one training
   step of the whole drop-in model;  4. direct C-ABI calls for the layouts include/rgbd_hip.h
   promises but the wrappers never produce (ldc / ldr / lda / ldb > extent, sc > M ldc, a split-K
   workspace of exactly rgbd_gemm_workspace_size bytes, colsum with ld > N), each against float64.
"""
import copy
import ctypes

import pytest
import torch

from checkers import guard
from test_gpu_dense import BF16_TOL, F32_TOL, _ref, _rel
from test_gpu_workspace_poison import _load, _state

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32, BF16 = torch.float32, torch.bfloat16
DT_IDS = ["f32", "bf16"]


def _flat(out):
    if isinstance(out, torch.Tensor):
        return [out]
    return [t for o in out for t in _flat(o)]


def _same_bits(a, b):
    """Bitwise, NaNs included (torch.equal calls a NaN unequal to itself)."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(-1).view(torch.uint8),
                                                                     b.contiguous().view(-1).view(torch.uint8))


def _sweep(fn, *inputs):
    """fn(*inputs) with every tensor input copied between guards and every allocation of the
    package guarded, then plainly: guards clean, results bitwise equal.  Returns the number of
    guarded buffers checked."""
    with guard.guarded_allocations() as sw:
        placed = [sw.place(t) if isinstance(t, torch.Tensor) else t for t in inputs]
        got = _flat(fn(*placed))
        n = sw.check_all()
        assert sw.passed_through == 0
    want = _flat(fn(*inputs))
    assert len(got) == len(want) and n > len([t for t in inputs if isinstance(t, torch.Tensor)])
    for i, (a, b) in enumerate(zip(got, want)):
        assert _same_bits(a, b), f"output {i} differs from the unguarded call"
    print(f"{n} guarded buffers clean, {len(got)} results bitwise equal")
    return n


def _randn(g, shape, dt=F32, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(DEV, dt)


# ------------------------------------------------------------------ 1. hot path
HOT_SHAPES = [(90, 125, 2), (97, 131, 3), (64, 96, 1)]


def _hot_parts(ctx, mode):
    import bench
    from rgbd_amd import ops
    if mode != "bf16_f32io":
        return bench.make_parts(ctx, 1)[0]
    from rgbd_amd.hot_path import hot_path, prepare

    def fb():
        pv = ops.assemble_pixel_values(ctx["depth_u8"], ctx["rgb_u8"])
        prep = prepare(pv, ctx["colors"], BF16, dsam_modules=ctx["dsams"], interface_dtype=F32)
        ratio = ctx["rp"](pv[:, 3:6])
        feats = hot_path(pv, ratio, ctx["colors"], ctx["dsams"], ctx["dg"], dtype=BF16, prepared=prep,
                         interface_dtype=F32)
        torch.autograd.backward(feats, ctx["gouts"])
        return feats
    return fb


@pytest.mark.parametrize("mode", ["f32", "bf16", "bf16_f32io"])
@pytest.mark.parametrize("H,W,B", HOT_SHAPES, ids=[f"{h}x{w}_b{b}" for h, w, b in HOT_SHAPES])
def test_hot_path_train_step_and_eval_ratio(H, W, B, mode):
    """K1 assembly, the ratio predictor (train: batch-statistics BatchNorms and dropout; eval), the
    decomposition, the DSAM cascade and the DGGM, forward and backward.  97x131, B = 3 leaves the
    linear 128-pixel and the 8x16 DSAM tiles both ragged with several split-K chunks.  The context
    is entered before the first call, so the pack caches, plans and run workspaces are guarded too."""
    import bench
    from rgbd_amd import ops
    args = bench.parse(["--height", str(H), "--width", str(W), "--batch", str(B), "--dtype",
                        "fp32" if mode == "f32" else "bf16"])
    ctx = bench.build(args, DEV)
    if mode == "bf16_f32io":  # bf16 compute, float32 colour maps, cp1 and outputs
        ctx["colors"] = [c.float() for c in ctx["colors"]]
        ctx["gouts"] = [g.float() for g in ctx["gouts"]]
    state = _state(ctx)
    seed = 0x5EED

    def run(c):
        fb = _hot_parts(c, mode)
        _load(c, state, seed)
        feats = fb()
        c["rp"].eval()
        with torch.no_grad():
            r_eval = c["rp"](ops.assemble_pixel_values(c["depth_u8"], c["rgb_u8"])[:, 3:6])
        c["rp"].train()
        torch.cuda.synchronize()
        out = [f.detach().clone() for f in feats] + [r_eval.clone()]
        out += [p.grad.detach().clone() for m in c["dsams"] + [c["dg"]] for p in m.parameters()]
        out += [b.detach().clone() for b in c["rp"].buffers()]
        return out

    with guard.guarded_allocations() as sw:
        cg = dict(ctx)  # the same modules, the inputs between guards
        for k in ("depth_u8", "rgb_u8"):
            cg[k] = sw.place(ctx[k], k)
        for k in ("colors", "gouts"):
            cg[k] = [sw.place(t, k) for t in ctx[k]]
        got = run(cg)
        n = sw.check_all()
        n_ws = len(sw.workspaces())
        assert sw.passed_through == 0
    want = run(ctx)
    print(f"hot path {H}x{W} B={B} {mode}: {n} guarded buffers clean ({n_ws} workspaces)")
    assert n_ws > 0 and n > 20
    assert all(torch.isfinite(t).all() for t in got[:5])
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if not _same_bits(a, b)]
    assert len(got) == len(want) and not bad, f"tensors {bad} of {len(want)} differ from the unguarded run"


# ------------------------------------------------------------------ 2. dense family
@pytest.mark.parametrize("dt", [F32, BF16], ids=DT_IDS)
@pytest.mark.parametrize("a_t,b_t", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(37, 130, 72), (3, 5, 7)])
def test_gemm_layouts(dt, a_t, b_t, M, N, K):
    from rgbd_amd import dense
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    A = _randn(g, (K, M) if a_t else (M, K), dt)
    B = _randn(g, (K, N) if b_t else (N, K), dt)
    bias, R = _randn(g, (N,)), _randn(g, (M, N), dt)
    _sweep(lambda A, B: dense.gemm(A, B, a_t, b_t, M, N, K), A, B)
    _sweep(lambda A, B, bias, R: dense.gemm(A, B, a_t, b_t, M, N, K, bias=bias, act=dense.ACT_RELU, R=R), A, B, bias, R)


@pytest.mark.parametrize("c_f32", [0, 1, 2])
@pytest.mark.parametrize("act", [0, 1, 2, 3], ids=["none", "relu", "gelu", "relu_grad"])
def test_gemm_lds_dma(act, c_f32):
    """The LDS-DMA kernel (bf16, M >= 1024) with ragged M / N / K: 1029 = 8 x 128 + 5 rows,
    264 = 2 x 128 + 8 columns, K = 200 (zero lines past K)."""
    from rgbd_amd import dense
    M, N, K = 1029, 264, 200
    g = torch.Generator().manual_seed(act)
    A, B = _randn(g, (M, K), BF16), _randn(g, (N, K), BF16)
    bias = None if act == 3 else _randn(g, (N,))
    R = _randn(g, (M, N), F32 if c_f32 == 1 else BF16) if act in (0, 3) else None
    _sweep(lambda A, B, bias, R: dense.gemm(A, B, 0, 0, M, N, K, bias=bias, act=act, R=R, c_f32=c_f32), A, B, bias, R)


@pytest.mark.parametrize("c_f32", [True, False], ids=["f32_out", "bf16_out"])
def test_gemm_lds_dma_weight_gradient(c_f32):
    from rgbd_amd import dense
    N, K, M = 136, 200, 1100
    g = torch.Generator().manual_seed(N + K + M)
    gy, x = _randn(g, (M, N), BF16), _randn(g, (M, K), BF16)
    _sweep(lambda gy, x: dense.gemm(gy, x, 1, 1, N, K, M, c_f32=c_f32), gy, x)


@pytest.mark.parametrize("dt", [F32, BF16], ids=DT_IDS)
@pytest.mark.parametrize("batch,M,N,K", [(1, 100, 72, 8192), (3, 64, 130, 4096)])
def test_gemm_split_k_epilogue(dt, batch, M, N, K):
    """Split-K partial slabs in a workspace of exactly rgbd_gemm_workspace_size bytes."""
    from rgbd_amd import dense
    assert dense._splits(M, N, K) > 1
    g = torch.Generator().manual_seed(9)
    A, B = _randn(g, (batch, M, K), dt), _randn(g, (batch, N, K), dt)
    bias, R = _randn(g, (N,)), _randn(g, (batch, M, N), dt)
    _sweep(lambda A, B, bias, R: dense.gemm(A, B, 0, 0, M, N, K, bias=bias, act=dense.ACT_RELU, R=R, batch=batch,
                                            sa=M * K, sb=N * K, sr=M * N), A, B, bias, R)


@pytest.mark.parametrize("dt", [F32, BF16], ids=DT_IDS)
@pytest.mark.parametrize("rows,N", [(7, 1000), (1234, 77)])
def test_colsum(dt, rows, N):
    from rgbd_amd import dense
    y = _randn(torch.Generator().manual_seed(rows), (rows, N), dt)
    _sweep(dense.colsum, y)
    _sweep(dense.colsum, y)  # a second workspace, zeroed anew: the tickets' contract


@pytest.mark.parametrize("dt", [F32, BF16], ids=DT_IDS)
# C = 62 / 1002 (no multiple of 4): the one-wave-per-row kernels
@pytest.mark.parametrize("C,rows", [(60, 777), (1000, 333), (96, 333), (62, 37), (1002, 37)])
def test_layer_norm_fwd_bwd(dt, C, rows):
    from rgbd_amd import dense
    g = torch.Generator().manual_seed(C)
    ln = dense.HipLayerNorm(C, eps=1e-5).to(DEV)
    with torch.no_grad():
        ln.weight.copy_(torch.randn(C, generator=g))
        ln.bias.copy_(torch.randn(C, generator=g))
    x, gy = _randn(g, (rows, C), dt, 3.0), _randn(g, (rows, C), dt)

    def fn(x, gy):
        x = x.detach().requires_grad_()
        y = dense.layer_norm(x, ln)
        return [y.detach()] + list(torch.autograd.grad(y, [x, ln.weight, ln.bias], gy))
    _sweep(fn, x, gy)


@pytest.mark.parametrize("clamp", [False, True], ids=["plain", "clamp"])
@pytest.mark.parametrize("xdt,rdt", [(F32, F32), (F32, BF16), (BF16, BF16)], ids=["f32+f32", "f32+bf16", "bf16+bf16"])
def test_add_layer_norm_fwd_bwd(xdt, rdt, clamp):
    from rgbd_amd import dense
    C, rows = 96, 333
    g = torch.Generator().manual_seed(C + rows)
    ln = dense.HipLayerNorm(C, eps=1e-5).to(DEV)
    with torch.no_grad():
        w = torch.randn(C, generator=g)
        if clamp:
            w[7] = 1e38  # channel 7 overflows and is clamped (tests/test_gpu_dense.py)
        ln.weight.copy_(w)
        ln.bias.copy_(torch.randn(C, generator=g))
    x, r = _randn(g, (rows, C), xdt, 3.0), _randn(g, (rows, C), rdt)
    gy = _randn(g, (rows, C), torch.promote_types(xdt, rdt))

    def fn(x, r, gy):
        x, r = x.detach().requires_grad_(), r.detach().requires_grad_()
        y = dense.add_layer_norm(x, r, ln, clamp=clamp)
        return [y.detach()] + list(torch.autograd.grad(y, [x, r, ln.weight, ln.bias], gy))
    _sweep(fn, x, r, gy)


def test_group_norm_fwd_bwd():
    from rgbd_amd import dense
    shape = (1, 64, 7, 9)
    g = torch.Generator().manual_seed(7)
    gn = dense.HipGroupNorm(32, 64).to(DEV)
    with torch.no_grad():
        gn.weight.copy_(torch.randn(64, generator=g))
        gn.bias.copy_(torch.randn(64, generator=g))
    x, gy = _randn(g, shape, F32, 2.0), _randn(g, shape)

    def fn(x, gy):
        x = x.detach().requires_grad_()
        y = gn(x)
        return [y.detach()] + list(torch.autograd.grad(y, [x, gn.weight, gn.bias], gy))
    _sweep(fn, x, gy)


@pytest.mark.parametrize("dt", [F32, BF16], ids=DT_IDS)
@pytest.mark.parametrize("k,C,H,W", [(3, 5, 7, 13), (4, 3, 16, 24)])
def test_im2col(dt, k, C, H, W):
    from rgbd_amd import conv
    x = _randn(torch.Generator().manual_seed(k), (2, C, H, W), dt)
    _sweep(lambda x: conv._im2col(x, k), x)
    col = conv._im2col(x, k).float()
    want = torch.nn.functional.unfold(x.float(), k, padding=1 if k == 3 else 0, stride=1 if k == 3 else 4)
    assert torch.equal(col, want)


NHWC_SHAPES = [(3, 40, 7, 9), (1, 8, 1, 1), (2, 136, 33, 65)]


@pytest.mark.parametrize("shape", NHWC_SHAPES, ids=["3x40x7x9", "1x8x1x1", "2x136x33x65"])
def test_nchw_to_nhwc_family(shape):
    """The chunked NHWC transposes: the single-tensor kernel in both dtypes, the bf16 multi launch
    and the float32 multi launch with both output dtypes; each also equal to torch's permute."""
    from rgbd_amd import ops
    g = torch.Generator().manual_seed(shape[1])
    xf, xb = _randn(g, shape), _randn(g, shape, BF16)
    small = _randn(g, (1, 8, 1, 1))
    _sweep(ops.nchw_to_nhwc, xf)
    _sweep(ops.nchw_to_nhwc, xb)
    _sweep(lambda a, b: ops.nchw_to_nhwc_multi([a, b, a]), xb, small.bfloat16())
    _sweep(lambda a, b: ops.nchw_to_nhwc_multi_f32([a, b, a, b], [BF16, F32, F32, BF16]), xf, small)
    assert torch.equal(ops.nchw_to_nhwc(xf), xf.permute(0, 2, 3, 1).contiguous())
    a, b = ops.nchw_to_nhwc_multi_f32([xf, xf], [BF16, F32])
    assert torch.equal(a, xf.bfloat16().permute(0, 2, 3, 1).contiguous()) and torch.equal(b, xf.permute(0, 2, 3, 1).contiguous())
    assert torch.equal(ops.nchw_to_nhwc_multi([xb])[0], xb.permute(0, 2, 3, 1).contiguous())


def test_dggm_single_forms_and_scalar_assemble():
    """What the hot-path sweep does not call: the single-scale DGGM forms (one-scale launches of
    the multi-scale kernels; the backward's workspace is exactly rgbd_dggm_fuse_bwd_workspace_size)
    at h*w % 8 == 0, % 4 == 0 and odd, C ragged against the 32- and 8-channel blocks, and K1 alone
    at W % 4 != 0 (the scalar path; its partials live in rgbd_assemble_workspace_size bytes)."""
    from rgbd_amd import ops
    g = torch.Generator().manual_seed(5)
    depth = torch.randint(0, 256, (2, 9, 13), generator=g, dtype=torch.uint8).to(DEV)
    rgb = torch.randint(0, 256, (2, 9, 13, 3), generator=g, dtype=torch.uint8).to(DEV)
    _sweep(ops.assemble_pixel_values, depth, rgb)
    pv = ops.assemble_pixel_values(depth, rgb)
    for dt in (F32, BF16):
        for C, h, w in [(40, 4, 6), (33, 3, 4), (8, 3, 5)]:
            color, cp1, dout = (_randn(g, (2, C, h, w), dt) for _ in range(3))
            wt, bs = _randn(g, (C, 3, 1, 1)), _randn(g, (C,))
            _sweep(ops.dggm_fuse_fwd, cp1, color, pv, wt, bs)
            _sweep(lambda c, p, w_, b_: ops.dggm_fuse_fwd(None, c, p, w_, b_), color, pv, wt, bs)
            _sweep(ops.dggm_fuse_bwd, dout, pv, wt, bs)


def test_dsam_legs_with_wrapper_made_plans():
    """bf16 DSAM legs called without ``plan=``: the wrapper plans the leg alone (ops.dsam_plan) and
    sizes the workspace for the run part only (rgbd_dsam_run_workspace_size).  97x131, B = 3
    (pyramid 25x33, 13x17, 7x9): the linear 128-pixel tiles and the 8x16 tiles are both ragged and
    a tile spans several chunks, the smallest shapes at which the partial-tile carve can go wrong.
    Plans, partial tiles, channel sums and outputs all sit between guards."""
    from rgbd_amd import ops, synthetic
    B, H, W = 3, 97, 131
    planes, _, _ = synthetic.make_batch(7, B, H, W)
    d3 = torch.from_numpy(planes[:, 3:6]).to(DEV)
    sizes = [(25, 33), (13, 17), (7, 9)]
    codes, info = ops.edsam_decompose(d3, torch.linspace(0.05, 0.45, B, device=DEV), sizes)
    g = torch.Generator().manual_seed(5)
    packs = []
    for ci, co in [(96, 192), (192, 384)]:
        cw, pw = _randn(g, (4, co, ci, 3, 3), scale=0.03), _randn(g, (co, ci, 3, 3), scale=0.03)
        packs.append(ops.dsam_pack(cw, pw, BF16))
    b4 = _randn(g, (4, 192), scale=0.1)
    x0 = _randn(g, (B, 25, 33, 96), BF16)
    res0, gy0 = _randn(g, (B, 13, 17, 192), BF16), _randn(g, (B, 13, 17, 192), BF16, 0.1)
    gy1, gin1 = _randn(g, (B, 7, 9, 384), BF16, 0.1), _randn(g, (B, 13, 17, 192), BF16)
    _sweep(lambda x, c, i, wf, b, r: ops.dsam_fwd_nhwc(x, c, i, wf, b, residual_nhwc=r),
           x0, codes[0], info, packs[0][0], b4, res0)
    _sweep(lambda gy, c, wb, gin: ops.dsam_bwd_data(gy, c, wb, None, want_nhwc=True, want_nchw=False, gin_nhwc=gin)[1],
           gy1, codes[1], packs[1][1], gin1)
    _sweep(lambda gy, x, c, i: ops.dsam_bwd_weight(None, x, c, i, gout_nhwc=gy), gy0, x0, codes[0], info)
    _sweep(lambda x, c, i, wf, b, r: ops.dsam_fwd(x, c, i, wf, b, residual=r, want_nhwc=True),
           x0, codes[0], info, packs[0][0], b4, res0.permute(0, 3, 1, 2).contiguous())


# ------------------------------------------------------------------ 3. whole model
_MODEL = []


def _model():
    if not _MODEL:
        from rgbd_amd import init as winit
        from rgbd_amd.config import standard_config
        from rgbd_amd.custom_model import CustomMask2FormerForUniversalSegmentation
        torch.manual_seed(0)
        m = CustomMask2FormerForUniversalSegmentation(standard_config(48), version="0.4.0")
        winit.init_deterministic(m)
        m = m.to(DEV).train()
        _MODEL.extend([m, copy.deepcopy(m.state_dict())])
    return _MODEL


@pytest.mark.parametrize("amp", [False, True], ids=["f32", "bf16_autocast"])
def test_whole_model_train_step(amp):
    """One training step (forward with labels, loss, backward) of the whole drop-in model at
    320x240, B = 1: the only place the MSDA, masked-attention, mask-predictor, point-loss / top-k,
    LSAP and Swin kernels run on real shapes together.  Guards clean, loss finite, and the loss
    within 4x the difference of two unguarded runs (the float-atomic scatters of the backward are
    the only run-to-run noise, as tests/test_gpu_ddp_model.py)."""
    import golden_inputs as gi
    m, state = _model()
    m.set_compute_dtype(BF16 if amp else F32)
    rp = m.model.pixel_level_module.ratio_predictor
    H, W = 240, 320
    pv0 = torch.from_numpy(gi.pixel_values(6, 1, H, W)).to(DEV)
    masks, classes = gi.labels(6, 1, H, W)
    ml0 = [torch.from_numpy(x).to(DEV) for x in masks]
    cl0 = [torch.from_numpy(c).to(DEV) for c in classes]

    def step(pv, ml, cl):
        m.load_state_dict(state)
        m.zero_grad(set_to_none=True)
        rp._rgbd_dropout_seed = 0x5EED
        rp._rgbd_dropout_ctr = torch.zeros((1,), dtype=torch.int64, device=DEV)
        torch.manual_seed(1234)
        with torch.autocast("cuda", dtype=BF16, enabled=amp):
            out = m(pixel_values=pv, mask_labels=ml, class_labels=cl)
        out.loss.backward()
        torch.cuda.synchronize()
        grads = [p.grad for p in m.parameters() if p.grad is not None]
        assert grads and all(torch.isfinite(g).all() for g in grads)
        return float(out.loss.detach().double())

    with guard.guarded_allocations() as sw:
        got = step(sw.place(pv0, "pixel_values"), [sw.place(x, "mask_labels") for x in ml0],
                   [sw.place(c, "class_labels") for c in cl0])
        n = sw.check_all()
        n_ws = len(sw.workspaces())
    a, b = step(pv0, ml0, cl0), step(pv0, ml0, cl0)
    print(f"whole model {'bf16 autocast' if amp else 'float32'}: {n} guarded buffers clean ({n_ws} workspaces, "
          f"{sw.passed_through} requests passed through); loss guarded {got!r}, unguarded {a!r} / {b!r}")
    assert n > 500 and n_ws > 0
    assert got == got and abs(got) != float("inf"), "loss not finite"
    assert abs(got - a) <= 4 * abs(a - b), f"guarded loss {got!r} vs unguarded {a!r} (run-to-run {abs(a - b):.3g})"


# ------------------------------------------------------------------ 4. direct C-ABI layouts
def _lib():
    from rgbd_amd import _lib as L
    return L.lib()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _put(pool, t, strides, tag):
    """t copied into a guarded buffer with the given element strides (gaps stay 0xFF = NaN)."""
    g = pool.new(t.shape, t.dtype, DEV, tag=tag, strides=strides)
    g.payload.copy_(t)
    return g.payload


def _gemm_cabi(dt, a_t, b_t, M, N, K, batch=1, lda=None, ldb=None, ldc=None, ldr=None, sa=None, sb=None, sc=None,
               sr=None, bias=True, act=0, with_r=True, c_f32=0, splits=1, seed=0):
    """rgbd_gemm on strided guarded operands; returns (C payload view [batch, M, N], float64
    reference).  Every leading dimension / batch stride defaults to the dense one."""
    from rgbd_amd.dense import _CODE
    L = _lib()
    g = torch.Generator().manual_seed(seed + M + N + K)
    ar, ac = (K, M) if a_t else (M, K)
    br, bc = (K, N) if b_t else (N, K)
    lda, ldb, ldc, ldr = lda or ac, ldb or bc, ldc or N, ldr or N
    sa, sb, sc, sr = sa or ar * lda, sb or br * ldb, sc or M * ldc, sr or M * ldr
    c_dt = F32 if (c_f32 or dt == F32) else dt
    r_dt = dt if c_f32 == 2 else c_dt
    A, B = _randn(g, (batch, ar, ac), dt), _randn(g, (batch, br, bc), dt)
    bias_t = _randn(g, (N,)) if bias else None
    R = _randn(g, (batch, M, N), r_dt) if with_r else None
    pool = guard.Pool()
    Ag, Bg = _put(pool, A, (sa, lda, 1), "A"), _put(pool, B, (sb, ldb, 1), "B")
    Rg = None if R is None else _put(pool, R, (sr, ldr, 1), "R")
    bg = None if bias_t is None else pool.place(bias_t, "bias")
    C = pool.new((batch, M, N), c_dt, DEV, tag=f"C ldc={ldc} sc={sc}", strides=(sc, ldc, 1))
    ws = None
    if splits > 1:
        nb = L.rgbd_gemm_workspace_size(M, N, batch, splits)
        assert nb == batch * splits * M * N * 4
        ws = pool.new((nb,), torch.uint8, DEV, tag="split-K workspace").payload  # exactly that, 0xFF-filled
    rc = L.rgbd_gemm(_CODE[dt], a_t, b_t, M, N, K, _p(Ag), lda, sa, _p(Bg), ldb, sb, _p(bg), act, _p(Rg), ldr, sr,
                     _p(C.payload), ldc, sc, c_f32, batch, splits, _p(ws), _stream())
    assert rc == 0, rc
    pool.check_all()
    assert torch.isfinite(C.payload).all()  # every cell written, no gap / guard NaN consumed
    ref = _ref(A, B, a_t, b_t, bias_t, act, R)
    return C.payload, ref


def _tol(dt):
    return F32_TOL if dt == F32 else BF16_TOL


@pytest.mark.parametrize("c_f32", [0, 1, 2])
@pytest.mark.parametrize("dt", [F32, BF16], ids=DT_IDS)
@pytest.mark.parametrize("N,ldc", [(128, 136), (130, 131)], ids=["vector_store", "scalar_store"])
def test_cabi_gemm_ldc_larger_than_n(dt, N, ldc, c_f32):
    for a_t, b_t in [(0, 0), (0, 1), (1, 1)]:
        C, ref = _gemm_cabi(dt, a_t, b_t, 37, N, 72, ldc=ldc, c_f32=c_f32, act=1)
        assert C.dtype == (BF16 if (dt == BF16 and c_f32 == 0) else F32)
        assert _rel(C, ref) < _tol(dt), (a_t, b_t)


@pytest.mark.parametrize("dt", [F32, BF16], ids=DT_IDS)
@pytest.mark.parametrize("pad", [8, 3], ids=["pad8_vector", "pad3_scalar"])
def test_cabi_gemm_lda_ldb_ldr_larger_than_extent(dt, pad):
    M, N, K = 37, 130, 72
    for a_t, b_t in [(0, 0), (0, 1), (1, 0), (1, 1)]:
        C, ref = _gemm_cabi(dt, a_t, b_t, M, N, K, lda=(M if a_t else K) + pad, ldb=(N if b_t else K) + pad,
                            ldr=N + pad + 3, ldc=N + pad)
        assert _rel(C, ref) < _tol(dt), (a_t, b_t)
        C, ref = _gemm_cabi(dt, a_t, b_t, M, N, K, lda=(M if a_t else K) + pad, ldb=(N if b_t else K) + pad,
                            ldr=N + pad, act=3, bias=False)
        assert _rel(C, ref) < _tol(dt), (a_t, b_t, "relu_grad")


@pytest.mark.parametrize("dt", [F32, BF16], ids=DT_IDS)
def test_cabi_gemm_batched_sc_larger_than_m_ldc(dt):
    M, N, K = 37, 130, 72
    for ldc, extra in [(131, 5), (136, 64)]:
        C, ref = _gemm_cabi(dt, 0, 0, M, N, K, batch=3, ldc=ldc, sc=M * ldc + extra, sa=M * K + 8, sb=N * K + 16,
                            ldr=N + 2, sr=M * (N + 2) + 7)
        assert _rel(C, ref) < _tol(dt), (ldc, extra)


@pytest.mark.parametrize("c_f32", [0, 1, 2])
def test_cabi_gemm_lds_kernel_ldc(c_f32):
    """The LDS-DMA kernel (bf16, 1029 x 264 x 200) storing into ldc = 272."""
    for act, with_r in [(0, True), (1, False)]:
        C, ref = _gemm_cabi(BF16, 0, 0, 1029, 264, 200, ldc=272, ldr=280, c_f32=c_f32, act=act, with_r=with_r)
        assert _rel(C, ref) < BF16_TOL, act


@pytest.mark.parametrize("dt", [F32, BF16], ids=DT_IDS)
def test_cabi_gemm_split_k_ldc_exact_workspace(dt):
    """Split-K at (100, 72, 8192) into ldc = 80: float32 partials [batch * splits][M][N] in a
    workspace of exactly rgbd_gemm_workspace_size bytes, summed in split order, then the epilogue."""
    from rgbd_amd import dense
    M, N, K = 100, 72, 8192
    splits = dense._splits(M, N, K)
    assert splits > 1
    C, ref = _gemm_cabi(dt, 0, 0, M, N, K, ldc=80, ldr=88, act=1, splits=splits)
    assert _rel(C, ref) < _tol(dt)


@pytest.mark.parametrize("dt", [F32, BF16], ids=DT_IDS)
@pytest.mark.parametrize("rows,N,ld", [(1234, 77, 80), (1234, 77, 83), (7, 1000, 1008), (300, 256, 264)])
def test_cabi_colsum_ld_larger_than_n(dt, rows, N, ld):
    from rgbd_amd.dense import _CODE
    L = _lib()
    y = _randn(torch.Generator().manual_seed(rows + ld), (rows, N), dt)
    pool = guard.Pool()
    yg = _put(pool, y, (ld, 1), "y")
    out = pool.new((N,), F32, DEV, tag="colsum out")
    ws = pool.new((L.rgbd_colsum_workspace_size(rows, N),), torch.uint8, DEV, zero=True, tag="colsum workspace")
    for _ in range(2):  # the second call finds the tickets rearmed
        assert L.rgbd_colsum(_CODE[dt], _p(yg), rows, N, ld, _p(out.payload), _p(ws.payload), _stream()) == 0
        pool.check_all()
        assert _rel(out.payload, y.double().sum(0)) < 1e-5
