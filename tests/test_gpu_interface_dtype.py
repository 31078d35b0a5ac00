"""The float32-interface bf16 mode of the hot path on the GPU (compute dtype bfloat16, interface
dtype float32: DESIGN.md §5.11): colour maps in, cp1 and features out in float32, bf16 only as the
DSAM operands.  Bitwise checks of the new layout kernel and DSAM epilogue against torch and
against the plain bf16 entry points, the float32 NHWC-cp1 path of the DGGM pass the mode relies
on, the three precision modes of the hot path side by side against the oracle, the plain bf16
mode untouched, the mode inside a captured training step, and the whole model at G5."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
from oracle import hot_path as hot_o
from rgbd_amd import init as winit, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
BF16, F32 = torch.bfloat16, torch.float32
# tests/test_gpu_parity.py BF16_REL: max-abs error / max-abs value, bf16 operands with f32 accumulation
BF16_REL = 3e-2
DSAM_CH = [(96, 192), (192, 384), (384, 768)]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------ 1. layout kernel
LAYOUT_SHAPES = [(2, 96, 120, 160), (3, 40, 7, 8), (1, 8, 5, 5), (2, 768, 15, 20)]


def _layout_input(shape, seed):
    """Finite float32 values; among them exact ties between two bf16 neighbours (low half
    0x8000, even and odd bf16 mantissas, both signs), +0 and -0, float32 subnormals (below the
    smallest normal bf16, 2^-126) and the largest finite values that round to infinity or not."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(shape, generator=g, device=DEV)
    flat = x.view(-1).view(torch.int32)
    n = flat.numel()
    idx = torch.randperm(n, generator=g, device=DEV)
    q = max(n // 8, 1)
    ties = (flat[idx[:q]] & ~0xFFFF) | 0x8000                               # exact ties
    flat[idx[:q]] = ties
    sub = torch.randint(0, 0x00800000, (q,), generator=g, device=DEV, dtype=torch.int32)
    sign = torch.randint(0, 2, (q,), generator=g, device=DEV, dtype=torch.int32) << 31
    flat[idx[q:2 * q]] = sub | sign                                          # subnormals, both signs
    special = torch.tensor([0, -0x80000000, 0x00000001, 0x00008000, 0x00018000, 0x007F8000, 0x7F7F7FFF, 0x7F7F8000,
                            0x3F808000, 0x3F818000], dtype=torch.int64, device=DEV).to(torch.int32)
    k = min(special.numel(), n - 2 * q)
    flat[idx[2 * q:2 * q + k]] = special[:k]
    assert torch.isfinite(x).all()
    return x


def _layout_check(xs, dts):
    for x, dt, y in zip(xs, dts, ops.nchw_to_nhwc_multi_f32(xs, dts)):
        ref = x.to(dt).permute(0, 2, 3, 1).contiguous()
        assert y.dtype == dt and _same_bits(y, ref), (tuple(x.shape), dt)


def test_layout_f32_source_bitwise():
    xs = [_layout_input(s, 40 + i) for i, s in enumerate(LAYOUT_SHAPES)]
    _layout_check(xs, [BF16, F32, BF16, F32])        # four to a launch, mixed destinations
    _layout_check(xs, [F32, BF16, F32, BF16])
    _layout_check(xs[::-1], [BF16, BF16, BF16, F32])
    for x in xs:                                      # singly
        _layout_check([x], [BF16])
        _layout_check([x], [F32])
    with pytest.raises(ops._lib.RgbdHipError):       # C % 8 != 0
        ops.nchw_to_nhwc_multi_f32([torch.zeros((1, 12, 5, 5), device=DEV)], [BF16])
    with pytest.raises(ValueError):
        ops.nchw_to_nhwc_multi_f32([torch.zeros((1, 8, 5, 5), device=DEV, dtype=BF16)], [BF16])


# ------------------------------------------------------------------ 2. DSAM epilogue
@pytest.fixture(scope="module")
def dsam_setup():
    """Per image shape: region codes / info of the three DSAM input resolutions; per DSAM: packed
    bf16 filters for the codes present and the four biases."""
    from rgbd_amd.modules import DSAModule
    cache = {}

    def get(H, W, B):
        if (H, W, B) not in cache:
            sizes = gi.swin_sizes(H, W)
            pv = torch.from_numpy(gi.pixel_values(21, B, H, W)).to(DEV)
            codes, info = ops.edsam_decompose(pv[:, 3:6].contiguous(), torch.linspace(0.05, 0.45, B, device=DEV),
                                              sizes[:3])
            masks = ops.dsam_code_masks(codes)
            per = []
            for k, (ci, co) in enumerate(DSAM_CH):
                m = DSAModule(ci, co)
                winit.init_deterministic(m, prefix=f"f32io.dsam{k}.")
                conv_w = torch.stack([m.conv_layers[i].weight.detach() for i in range(4)]).to(DEV)
                bias4 = torch.stack([m.conv_layers[i].bias.detach() for i in range(4)]).to(DEV)
                wf, _ = ops.dsam_pack(conv_w, m.rgb_projection.weight.detach().to(DEV), BF16,
                                      code_mask=masks[k:k + 1], want_bwd=False)
                per.append((wf, bias4))
            cache[(H, W, B)] = (sizes, codes, info, per)
        return cache[(H, W, B)]
    return get


@pytest.mark.parametrize("planned", [False, True], ids=["unplanned", "planned"])
@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("H,W,B", [(97, 131, 3), (240, 320, 2)])
def test_dsam_f32io_epilogue_bitwise(dsam_setup, H, W, B, k, planned):
    """rgbd_dsam_fwd_nhwc's float32 interface on the three real DSAMs: 97x131, B = 3 (ragged tiles,
    several split-K chunks) and 240x320, B = 2."""
    sizes, codes, info, per = dsam_setup(H, W, B)
    (h, w), (ci, co) = sizes[k], DSAM_CH[k]
    ho, wo = sizes[k + 1]
    wf, bias4 = per[k]
    code = codes[k]
    g = torch.Generator(device=DEV).manual_seed(900 + 10 * k + H)
    x = torch.randn((B, h, w, ci), generator=g, device=DEV).bfloat16()
    r = torch.randn((B, ho, wo, co), generator=g, device=DEV)
    r16 = r.bfloat16()

    def plan():
        return ops.dsam_plan([(ops.LEG_FWD, code, ci, co)])[0] if planned else None

    def new(res):
        return ops.dsam_fwd_nhwc_f32io(x, code, info, wf, bias4, residual_f32_nhwc=res, plan=plan())

    def old(res16):
        return ops.dsam_fwd_nhwc(x, code, info, wf, bias4, residual_nhwc=res16, plan=plan())
    before = old(r16)
    o16, o32 = new(r)
    assert o16.dtype == BF16 and o32.dtype == F32 and o16.shape == o32.shape == (B, ho, wo, co)
    assert _same_bits(o16, o32.to(BF16)), "(a) the bf16 output is the one rounding of the float32 output"
    b16, b32 = new(r16.float())
    assert _same_bits(b16, before), "(b) bf16-representable residual: today's bf16 result"
    assert _same_bits(b16, b32.to(BF16))
    z16, v = new(torch.zeros_like(r))
    assert torch.equal(o32, r + v), "(c) out_f32 = r + v, one float32 add"
    n16, n32 = new(None)
    assert torch.equal(n32, v), "(c) a zero residual leaves v"
    assert _same_bits(n32.to(BF16), old(None)), "(d) no residual: today's no-residual result"
    assert _same_bits(n16, n32.to(BF16)) and _same_bits(z16, v.to(BF16))
    only16, none32 = ops.dsam_fwd_nhwc_f32io(x, code, info, wf, bias4, residual_f32_nhwc=r, want_f32=False, plan=plan())
    none16, only32 = ops.dsam_fwd_nhwc_f32io(x, code, info, wf, bias4, residual_f32_nhwc=r, want_bf16=False, plan=plan())
    assert none32 is None and none16 is None and _same_bits(only16, o16) and _same_bits(only32, o32)
    assert _same_bits(old(r16), before), "(e) today's entry point unchanged after the new one (shared workspace)"


# ------------------------------------------------------------------ 3. DGGM, float32 NHWC cp1
@pytest.mark.parametrize("shape", [(2, 96, 120, 160), (3, 192, 13, 17), (2, 384, 7, 9)])
def test_dggm_f32_cp1_nhwc_equals_nchw(shape):
    """rgbd_dggm_fuse_fwd_multi (RGBD_F32) with cp1 in NHWC gives bitwise the NCHW-cp1
    result: the path the mode's outputs take (shapes of test_dggm_cp1_nhwc_equals_nchw)."""
    B, C, h, w = shape
    pv = torch.from_numpy(gi.pixel_values(13, B, 4 * h, 4 * w)).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(9)
    color = torch.randn((B, C, h, w), generator=g, device=DEV)
    cp1 = torch.randn((B, C, h, w), generator=g, device=DEV)
    wt = torch.randn((C, 3, 1, 1), generator=g, device=DEV)
    bs = torch.randn((C,), generator=g, device=DEV)
    ref = ops.dggm_fuse_fwd_multi([cp1], [color], pv, [wt], [bs])[0]
    got = ops.dggm_fuse_fwd_multi([ops.nchw_to_nhwc(cp1)], [color], pv, [wt], [bs], cp1_nhwc=(0,))[0]
    assert got.dtype == F32 and _same_bits(got, ref)


# ------------------------------------------------------------------ 4 / 5. hot path, three modes
def _hot_modules():
    from rgbd_amd.modules import DSAModule, DepthGradientInjectionResidual
    pre = "model.pixel_level_module."
    dsams = []
    for k, (ci, co) in enumerate(DSAM_CH):
        m = DSAModule(ci, co)
        winit.init_deterministic(m, prefix=f"{pre}dsam{k}.")
        dsams.append(m.to(DEV))
    dg = DepthGradientInjectionResidual([96, 192, 384, 768], 3)
    winit.init_deterministic(dg, prefix=f"{pre}depth_gradient_injection.")
    return dsams, dg.to(DEV)


@pytest.fixture(scope="module")
def hp_runs():
    """Inputs, modules, ratios and oracle of test_hot_path_fused_vs_oracle (240x320, B = 2); one
    forward + backward per mode, in the order plain bf16, new mode, plain bf16 again, new mode
    without the side stream, float32; the oracle once."""
    from rgbd_amd.hot_path import hot_path
    H, W, B = 240, 320, 2
    pv = torch.from_numpy(gi.pixel_values(7, B, H, W))
    ratios = torch.tensor([[0.2], [0.07]], dtype=F32)
    sizes = gi.swin_sizes(H, W)
    colors = [torch.from_numpy(gi.feature(f"hp.c{k}", (B, c, *sizes[k]))) for k, c in enumerate([96, 192, 384, 768])]
    gouts = [torch.from_numpy(gi.feature(f"hp.g{k}", tuple(c.shape))) for k, c in enumerate(colors)]
    dsams, dg = _hot_modules()
    named = {}
    for k, m in enumerate(dsams):
        for n, p in m.named_parameters():
            named[f"dsam{k}.{n}"] = p
    for n, p in dg.named_parameters():
        named[f"depth_gradient_injection.{n}"] = p
    pvd, rd, cd = pv.to(DEV), ratios.to(DEV), [c.to(DEV) for c in colors]

    def run(dtype, interface, **kw):
        for p in named.values():
            p.grad = None
        outs = hot_path(pvd, rd, cd, dsams, dg, dtype=dtype, interface_dtype=interface, check_status=True, **kw)
        gdt = F32 if interface is not None else dtype
        torch.autograd.backward(outs, [g.to(DEV).to(gdt) for g in gouts])
        torch.cuda.synchronize()
        return [o.detach().clone() for o in outs], {n: p.grad.detach().clone() for n, p in named.items()}
    runs = {"bf16": run(BF16, None), "new": run(BF16, F32), "bf16_again": run(BF16, None),
            "new_serial": run(BF16, F32, overlap=False), "f32": run(F32, None), "f32_if": run(F32, F32)}
    sd = {}
    for k, m in enumerate(dsams):
        for kk, v in m.state_dict().items():
            sd[f"dsam{k}.{kk}"] = v.detach().cpu().clone().requires_grad_(True)
    for kk, v in dg.state_dict().items():
        sd[f"depth_gradient_injection.{kk}"] = v.detach().cpu().clone().requires_grad_(True)
    ref, _, _ = hot_o.hot_path_forward(colors, pv, sd, ratios=ratios)
    torch.autograd.backward(ref, gouts)
    return runs, [r.detach() for r in ref], {n: sd[n].grad for n in named}


def _feature_errors(outs, ref):
    res = []
    for o, e in zip(outs, ref):
        d = o.float().cpu() - e
        res.append((float(d.abs().max() / e.abs().max()), float(d.square().mean().sqrt())))
    return res


def test_hot_path_three_modes_vs_oracle(hp_runs):
    runs, ref, ref_grads = hp_runs
    new_o, new_g = runs["new"]
    f32_o, f32_g = runs["f32"]
    errs = {m: _feature_errors(runs[m][0], ref) for m in ("f32", "bf16", "new")}
    for m, e in errs.items():
        print(f"hot path {m:>4}: " + "  ".join(f"f{k} max-rel {a:.3g} rms {b:.3g}" for k, (a, b) in enumerate(e)))
    assert all(o.dtype == F32 for o in new_o)
    assert all(o.dtype == BF16 for o in runs["bf16"][0])
    assert _same_bits(new_o[0], f32_o[0]), "feature 0 takes no bf16 operand: the float32 mode's bits"
    for k in (1, 2, 3):
        assert errs["new"][k][1] <= errs["bf16"][k][1], f"feature {k}: rms {errs['new'][k][1]} > plain bf16's"
    for k in range(4):
        assert errs["new"][k][0] < BF16_REL, f"feature {k}"
    for n, e in ref_grads.items():
        scale = max(float(e.abs().max()), 1e-6)
        err = float((new_g[n].float().cpu() - e).abs().max()) / scale
        if n.startswith("dsam"):
            assert err < BF16_REL, f"{n}: rel err {err}"
        else:  # they depend only on G, pixel_values and the DGGM weights
            assert _same_bits(new_g[n], f32_g[n]), f"{n}: not the float32 mode's bits"
    # interface float32 with compute float32 is the float32 mode
    for a, b in zip(runs["f32_if"][0], f32_o):
        assert _same_bits(a, b)
    for n in f32_g:
        assert _same_bits(runs["f32_if"][1][n], f32_g[n]), n


def test_plain_bf16_untouched_and_serial_schedule(hp_runs):
    runs, _, _ = hp_runs
    for a, b in zip(runs["bf16"][0], runs["bf16_again"][0]):
        assert _same_bits(a, b)
    for n, g in runs["bf16"][1].items():
        assert _same_bits(g, runs["bf16_again"][1][n]), n
    for a, b in zip(runs["new"][0], runs["new_serial"][0]):
        assert _same_bits(a, b)
    for n, g in runs["new"][1].items():
        assert _same_bits(g, runs["new_serial"][1][n]), n


def test_prepared_for_another_interface_is_refused():
    from rgbd_amd.hot_path import hot_path, prepare
    H, W, B = 64, 96, 1
    pv = torch.from_numpy(gi.pixel_values(11, B, H, W)).to(DEV)
    sizes = gi.swin_sizes(H, W)
    colors = [torch.from_numpy(gi.feature(f"pi.c{k}", (B, c, *sizes[k]))).to(DEV)
              for k, c in enumerate([96, 192, 384, 768])]
    dsams, dg = _hot_modules()
    ratio = torch.tensor([[0.2]], device=DEV)
    for made, asked in ((None, F32), (F32, None)):
        prep = prepare(pv, colors, BF16, interface_dtype=made)
        with pytest.raises(ValueError, match="interface"):
            hot_path(pv, ratio, colors, dsams, dg, dtype=BF16, prepared=prep, interface_dtype=asked)
        prep.join()
    prep = prepare(pv, colors, BF16, interface_dtype=F32, dsam_modules=dsams)
    with torch.no_grad():
        a = hot_path(pv, ratio, colors, dsams, dg, dtype=BF16, prepared=prep, interface_dtype=F32)
        b = hot_path(pv, ratio, colors, dsams, dg, dtype=BF16, interface_dtype=F32)
    for x, y in zip(a, b):
        assert x.dtype == F32 and _same_bits(x, y)


# ------------------------------------------------------------------ 6. capturable
def _train_ctx():
    """bench.build's modules and frames at 90x125, B = 2, with float32 colour maps and upstream
    gradients, and the same dropout stream in every arm."""
    import bench
    ctx = bench.build(bench.parse(["--height", "90", "--width", "125", "--batch", "2"]), DEV)
    assert ctx["dtype"] == BF16
    g = torch.Generator(device=DEV).manual_seed(77)
    ctx["colors"] = [torch.randn(c.shape, generator=g, device=DEV) for c in ctx["colors"]]
    ctx["gouts"] = [torch.randn(c.shape, generator=g, device=DEV) * 1e-2 for c in ctx["colors"]]
    ctx["rp"]._rgbd_dropout_ctr = torch.zeros((1,), dtype=torch.int64, device=DEV)
    ctx["rp"]._rgbd_dropout_seed = 0x5EED1234
    return ctx


def _train_parts(ctx):
    from rgbd_amd.hot_path import hot_path, prepare
    from rgbd_amd.optim import HF_TRAINER_ADAMW, HipAdamW
    params = [p for m in ctx["dsams"] + [ctx["dg"]] for p in m.parameters()]
    opt = HipAdamW(params, **HF_TRAINER_ADAMW)

    def fb():
        pv = ops.assemble_pixel_values(ctx["depth_u8"], ctx["rgb_u8"])
        prep = prepare(pv, ctx["colors"], BF16, dsam_modules=ctx["dsams"], interface_dtype=F32)
        ratio = ctx["rp"](pv[:, 3:6])
        feats = hot_path(pv, ratio, ctx["colors"], ctx["dsams"], ctx["dg"], dtype=BF16, prepared=prep,
                         interface_dtype=F32)
        torch.autograd.backward(feats, ctx["gouts"])
        return feats
    return fb, opt, params


def test_new_mode_captured_step_equals_eager_steps():
    """Two eager steps plus two replays of the captured step leave bitwise the parameters of four
    eager steps (after tests/test_gpu_train_graph.py::test_captured_step_equals_eager_steps)."""
    from rgbd_amd.train_graph import CapturedTrainStep
    a, b = _train_ctx(), _train_ctx()
    fa, oa, pa = _train_parts(a)
    for _ in range(4):
        fa()
        oa.step()
        oa.zero_grad(set_to_none=True)
    fb, ob, pb = _train_parts(b)
    step = CapturedTrainStep(fb, ob, warmup=2)
    for _ in range(2):
        outs = step()
    torch.cuda.synchronize()
    assert int(a["rp"]._rgbd_dropout_ctr.item()) == 4 == int(b["rp"]._rgbd_dropout_ctr.item())
    for i, (x, y) in enumerate(zip(pa, pb)):
        assert _same_bits(x.detach(), y.detach()), f"parameter {i} differs after 4 steps"
    assert len(outs) == 4 and all(o.dtype == F32 and torch.isfinite(o).all() for o in outs)


# ------------------------------------------------------------------ 7. whole model, G5
def _full_model():
    from rgbd_amd.config import standard_config
    from rgbd_amd.custom_model import CustomMask2FormerForUniversalSegmentation
    m = CustomMask2FormerForUniversalSegmentation(standard_config(48), version="0.4.0")
    winit.init_deterministic(m)
    return m.to(DEV)


def test_full_model_mask_logits_new_mode_below_plain_bf16(golden):
    """G5 (320x240, B = 1) with the reference's attention masks forced (arithmetic only): the new
    mode's max relative mask-logit error is strictly below the plain bf16 mode's on the same
    model, and within the bench line's bound."""
    import bench
    ref = golden("g5_model")["mask_logits"]
    refm = bench.ReferenceMasks("g5")
    m = _full_model().eval()
    pv = torch.from_numpy(gi.pixel_values(1, 1, 240, 320)).to(DEV)
    err = {}
    for name, interface in (("bf16", None), ("new", F32)):
        m.set_compute_dtype(BF16, interface=interface)
        rec = []
        h = refm.attach(m, True, rec)
        try:
            with torch.no_grad():
                out = m(pixel_values=pv)
        finally:
            h.remove()
        err[name] = float(np.abs(out.masks_queries_logits.float().cpu().numpy() - ref).max() / np.abs(ref).max())
    print(f"G5 mask-logit max-rel-err, reference masks forced: plain bf16 {err['bf16']:.3g}, "
          f"float32 interface {err['new']:.3g}")
    assert err["new"] < err["bf16"]
    assert err["new"] < bench.BF16_LOGIT_REL_TOL
