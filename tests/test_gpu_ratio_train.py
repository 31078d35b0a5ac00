"""The ratio predictor (K4, csrc/ratio.hip) in train mode against float64, stage by stage, with the
dropout masks replayed (tests/checkers/ratio_dropout.py; the rule is in include/rgbd_hip.h above
`rgbd_ratio_forward`).  Everything after feature_extractor.5's batch statistics is pinned here:

a. tail conv 256->512 + BatchNorm + ReLU + global average pool (`rgbd_ratio_feat_offset`) from the
   GPU's own pooled features (`rgbd_ratio_pooled_offset`): batch statistics in train mode, running
   statistics in eval mode, and the running-statistics update;
b. fc_layers[0:3] (`rgbd_ratio_hidden_offset`) from the GPU's feat, with the replayed keep mask;
c. fc_layers[3:] and the range map from the GPU's hidden layer, with the replayed keep mask and a
   last layer rescaled so that the logits span about [-2, 2];
d. the whole forward from the depth planes against the float64 module tree with the same masks;
e. the device counter: eval leaves it, train adds one, 64-bit, both train routes.

Tolerance of a float32 stage against float64 on that stage's own input as the GPU left it:
|got - ref| <= 2e-6 * (1 + max|ref|) (tests/test_gpu_masked_attention.py's form).  The tail is
float32 in both compute dtypes, so (a)-(c) hold for bfloat16 unchanged.  Each reference-side
self-check (the other kind of statistics, a flipped mask bit, the excluded-unit cap) is asserted.
Measured errors: DESIGN.md §5.10.1."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_inputs as gi
from checkers import ratio_dropout as rd
from oracle import ratio as ratio_o
from rgbd_amd import init as winit

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRE = "model.pixel_level_module.ratio_predictor."
SEED = 0x5EED
EPS = 1e-5
MOMENTUM = 0.1
CASES = [(1, 64, 96), (3, 90, 125), (11, 64, 96), (32, 32, 32)]
DTYPES = [torch.float32, torch.bfloat16]
IDS = {torch.float32: "f32", torch.bfloat16: "bf16"}


def run_stats():
    """feature_extractor.5's running statistics before the forward: per channel, unrelated to the
    batch's (whose means span +-0.5 with deviations around 0.15), so that "batch" and "running"
    give different answers, and of that size, so that eval mode's ReLU passes part of the map
    (with mean 0.5 / var 4 it would pass nothing: feat = 0)."""
    g = torch.Generator().manual_seed(5)
    return torch.randn(512, generator=g) * 0.25, torch.rand(512, generator=g) * 0.06 + 0.01


def tol32(ref):
    """float32 kernel against float64 arithmetic on the same input."""
    return 2e-6 * (1.0 + float(ref.abs().max()))


# ---------------------------------------------------------------- float64 restatements
def ref_feat(pooled, p, training, run_mean, run_var):
    """feature_extractor[4:8] + global average pool from pooled [B,256,4,4] (float64).
    Returns feat [B,512], the batch mean and the biased batch variance [512]."""
    y = F.conv2d(pooled, p["feature_extractor.4.weight"], p["feature_extractor.4.bias"], padding=1)
    mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
    m, v = (mean, var) if training else (run_mean, run_var)
    z = (y - m[None, :, None, None]) / torch.sqrt(v[None, :, None, None] + EPS)
    z = z * p["feature_extractor.5.weight"][None, :, None, None] + p["feature_extractor.5.bias"][None, :, None, None]
    return torch.relu(z).mean((2, 3)), mean, var


def ref_hidden(feat, p, keep1, training):
    """fc_layers[0:3] from feat [B,512] (float64): (pre-activation, h1)."""
    pre = feat @ p["fc_layers.0.weight"].T + p["fc_layers.0.bias"]
    h = torch.relu(pre)
    if training:
        h = h * torch.from_numpy(keep1).double() / (1.0 - rd.P1)
    return pre, h


def ref_head(h1, p, keep2, training):
    """fc_layers[3:] + range map from h1 [B,128] (float64): (fc_layers.3 pre-activation, logit [B], ratio [B])."""
    pre = h1 @ p["fc_layers.3.weight"].T + p["fc_layers.3.bias"]
    h = torch.relu(pre)
    if training:
        h = h * torch.from_numpy(keep2).double() / (1.0 - rd.P2)
    h = torch.relu(h @ p["fc_layers.6.weight"].T + p["fc_layers.6.bias"])
    z = (h @ p["fc_layers.8.weight"].T + p["fc_layers.8.bias"]).reshape(-1)
    return pre, z, 0.01 + (0.5 - 0.01) * torch.sigmoid(z)


# ---------------------------------------------------------------- running the kernels
def _module(dtype):
    from rgbd_amd.modules import EnhancedDepthImageRatioPredictor
    m = EnhancedDepthImageRatioPredictor(3)
    winit.init_deterministic(m, prefix=PRE)
    m.compute_dtype = dtype
    bn = m.feature_extractor[5]
    mean, var = run_stats()
    bn.running_mean.copy_(mean)
    bn.running_var.copy_(var)
    return m


def _params64(m):
    return {k: v.detach().cpu().double() for k, v in m.state_dict().items()}


def _set_counter(m, value):
    v = value if value < 2 ** 63 else value - 2 ** 64
    m._rgbd_dropout_seed = SEED
    m._rgbd_dropout_ctr = torch.full((1,), v, dtype=torch.int64, device=DEV)


def _counter(m):
    return int(m._rgbd_dropout_ctr.cpu()) % 2 ** 64


def _forward(m, x):
    """One forward; returns the ratio and the workspace's pooled / feat / h1 (float64, CPU; h1 also
    as its float32 bits)."""
    from rgbd_amd import _lib, ops
    B, _, H, W = x.shape
    with torch.no_grad():
        ratio = m(x)
    torch.cuda.synchronize()
    L = _lib.lib()
    code = 1 if m.compute_dtype == torch.bfloat16 else 0
    ws = ops._workspace(x.device, L.rgbd_ratio_workspace_size(code, B, H, W), "ratio")

    def rd32(off, n):
        return ws[off:off + 4 * n].view(torch.float32).clone().cpu()
    pooled = rd32(L.rgbd_ratio_pooled_offset(code, B, H, W), B * 256 * 16).reshape(B, 256, 4, 4)
    feat = rd32(L.rgbd_ratio_feat_offset(code, B, H, W), B * 512).reshape(B, 512)
    h1 = rd32(L.rgbd_ratio_hidden_offset(code, B, H, W), B * 128).reshape(B, 128)
    assert ratio.shape == (B, 1) and ratio.dtype == torch.float32
    return dict(ratio=ratio.reshape(-1).cpu().double(), pooled=pooled.double(), feat=feat.double(), h1=h1.double(),
                h1_bits=h1.view(torch.int32))


def _depth(B, H, W):
    return torch.from_numpy(gi.pixel_values(8, B, H, W)[:, 3:6].copy())


@functools.lru_cache(maxsize=None)
def _run(B, H, W, dtype, training):
    """The case's forward (counter 0), then, in train mode, a second one (counter 0 again) with
    fc_layers.8 rescaled so that the float64 logits computed from the first forward's h1 span
    [-2, 2] over the batch (one image: the logit becomes +-2).  Cached: the tests share it and
    leave it unchanged."""
    depth = _depth(B, H, W)
    m_cpu = _module(dtype).train(training)
    m = copy.deepcopy(m_cpu).to(DEV)
    p = _params64(m)
    _set_counter(m, 0)
    x = depth.to(DEV)
    out = dict(_forward(m, x), p=p, depth=depth, m_cpu=m_cpu, counter_after=_counter(m),
               stats_after={k: v.detach().cpu().double() for k, v in m.state_dict().items() if "running" in k})
    out["keep"] = rd.keep_masks(SEED, 0, B)
    if training:
        _, z, _ = ref_head(out["h1"], p, out["keep"][1], True)
        if B > 1:
            a = 4.0 / float(z.max() - z.min())
            c = -a * float(z.mean())
        else:
            a, c = 2.0 / abs(float(z[0])), 0.0
        with torch.no_grad():
            m.fc_layers[8].weight.mul_(a)
            m.fc_layers[8].bias.mul_(a).add_(c)
        _set_counter(m, 0)
        out["spread"] = dict(_forward(m, x), p=_params64(m), a=a, c=c)
    return out


def _params(fn):
    return pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)(pytest.mark.parametrize("B,H,W", CASES)(fn))


# ---------------------------------------------------------------- a. tail conv + BN + ReLU + GAP
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@_params
def test_tail_conv_bn_relu_gap(B, H, W, dtype, training):
    r = _run(B, H, W, dtype, training)
    p = r["p"]
    rm0, rv0 = (t.double() for t in run_stats())
    ref, mean, var = ref_feat(r["pooled"], p, training, rm0, rv0)
    other, _, _ = ref_feat(r["pooled"], p, not training, rm0, rv0)
    tol = tol32(ref)
    err = float((r["feat"] - ref).abs().max())
    gap = float((other - ref).abs().max())
    print(f"feat {B}x{H}x{W} {IDS[dtype]} train={training}: max|d| {err:.3g} (tol {tol:.3g}, max|ref| "
          f"{float(ref.abs().max()):.3g}); the other kind of statistics is {gap:.3g} away")
    assert gap > 100 * tol      # batch and running statistics give different answers here
    live = float((ref > 100 * tol).float().mean())
    # the features are not mostly 0; with running statistics the ReLU also stops whole channels
    # (with batch statistics every channel's map straddles 0, so nearly every mean is positive)
    assert live >= 0.2 and (training or live <= 0.9), live
    assert err <= tol
    got_rm = r["stats_after"]["feature_extractor.5.running_mean"]
    got_rv = r["stats_after"]["feature_extractor.5.running_var"]
    if training:
        n = B * 16
        want_rm = (1 - MOMENTUM) * rm0 + MOMENTUM * mean
        want_rv = (1 - MOMENTUM) * rv0 + MOMENTUM * var * n / (n - 1)
        e_rm, e_rv = float((got_rm - want_rm).abs().max()), float((got_rv - want_rv).abs().max())
        print(f"  running_mean max|d| {e_rm:.3g} (tol {tol32(want_rm):.3g}), running_var max|d| {e_rv:.3g} "
              f"(tol {tol32(want_rv):.3g})")
        assert e_rm <= tol32(want_rm)
        assert e_rv <= tol32(want_rv)
    else:
        assert torch.equal(got_rm, rm0) and torch.equal(got_rv, rv0)


# ---------------------------------------------------------------- b. fc1 + dropout
def check_hidden(r, p, keep1, training, tag):
    """h1 against float64 from the GPU's feat with the given keep mask; returns the units whose
    zero / non-zero state the reference decides (|pre-activation| beyond the tolerance)."""
    pre, ref = ref_hidden(r["feat"], p, keep1, training)
    tol = tol32(ref)
    decided = (pre.abs() > tol).numpy()
    assert (~decided).mean() <= 0.01, f"{tag}: {int((~decided).sum())} units within {tol:.3g} of 0"
    err = float((r["h1"] - ref).abs().max())
    print(f"h1 {tag}: max|d| {err:.3g} (tol {tol:.3g}, max|ref| {float(ref.abs().max()):.3g}); "
          f"{int((~keep1).sum())} of {keep1.size} dropped, {int((~decided).sum())} undecided")
    assert err <= tol, tag
    bits = r["h1_bits"].numpy()
    got = r["h1"].numpy()
    assert (bits[~keep1] == 0).all(), f"{tag}: a dropped unit is not +0.0"
    active = keep1 & decided & (pre.numpy() > 0)
    assert (got[active] != 0).all(), f"{tag}: a kept active unit is zero"
    assert (bits[decided & (pre.numpy() < 0)] == 0).all(), f"{tag}: ReLU left a negative unit"
    return decided


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@_params
def test_fc1_dropout(B, H, W, dtype, training):
    r = _run(B, H, W, dtype, training)
    keep1 = r["keep"][0] if training else np.ones((B, 128), bool)
    if training:
        assert 0 < (~keep1).sum() < keep1.size
    check_hidden(r, r["p"], keep1, training, f"{B}x{H}x{W} {IDS[dtype]} train={training}")


# ---------------------------------------------------------------- c. head
@_params
def test_head_with_spread_logits(B, H, W, dtype):
    r = _run(B, H, W, dtype, True)
    s, keep2 = r["spread"], r["keep"][1]
    p = s["p"]
    pre, z, ref = ref_head(s["h1"], p, keep2, True)
    tol = 0.1225 * 2e-6 * (1.0 + float(z.abs().max())) + 2.0 ** -23
    err = float((s["ratio"] - ref).abs().max())
    print(f"head {B}x{H}x{W} {IDS[dtype]}: logits {float(z.min()):.3f}..{float(z.max()):.3f} (a = {s['a']:.4g}), "
          f"ratio max|d| {err:.3g} (tol {tol:.3g})")
    assert float(z.abs().max()) <= 4.0 and (B == 1 or float(z.max() - z.min()) > 2.0)
    # a single wrong bit of keep2 must show: flip sampled active units in the reference
    active = np.argwhere(keep2 & (pre.numpy() > 0))
    assert len(active) >= 16
    pick = active[np.random.default_rng(0).choice(len(active), 16, replace=False)]
    moved = []
    for b, o in pick:
        k = keep2.copy()
        k[b, o] = False
        moved.append(float((ref_head(s["h1"], p, k, True)[2] - ref).abs().max()))
    print(f"  one flipped keep2 bit moves the ratio by {min(moved):.3g}..{max(moved):.3g}")
    assert sum(d >= 10 * tol for d in moved) >= 0.9 * len(moved)
    assert err <= tol


# ---------------------------------------------------------------- d. end to end
@_params
def test_train_ratio_end_to_end(B, H, W, dtype):
    """float32: within max(4 x the float32 CPU module's own error against float64, the project's
    eval tolerance rtol 1e-5 / atol 1e-6).  bfloat16: the stated bf16 tolerance on the ratio, atol
    5e-3 (tests/test_gpu_model.py)."""
    r = _run(B, H, W, dtype, True)
    m32 = copy.deepcopy(r["m_cpu"]).train()
    m64 = copy.deepcopy(r["m_cpu"]).double().train()
    with torch.no_grad():
        ref = ratio_o.ratio_forward_modules(m64, r["depth"].double(), dropout_keep=r["keep"]).reshape(-1)
        cpu32 = ratio_o.ratio_forward_modules(m32, r["depth"], dropout_keep=r["keep"]).reshape(-1).double()
    assert ref.dtype == torch.float64
    err = (r["ratio"] - ref).abs()
    own = float((cpu32 - ref).abs().max())
    print(f"ratio {B}x{H}x{W} {IDS[dtype]}: max|hip - f64| {float(err.max()):.3g}; float32 CPU module vs f64 {own:.3g}; "
          f"eval-tolerance bound {float((1e-6 + 1e-5 * ref.abs()).min()):.3g}")
    if dtype == torch.float32:
        assert bool((err <= torch.clamp_min(1e-6 + 1e-5 * ref.abs(), 4 * own)).all())
    else:
        assert float(err.max()) <= 5e-3
    assert r["counter_after"] == 1


# ---------------------------------------------------------------- e. counter semantics
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_dropout_counter(dtype):
    B, H, W = 3, 64, 96
    x = _depth(B, H, W).to(DEV)
    m = _module(dtype).to(DEV)
    p = _params64(m)
    tag = f"{B}x{H}x{W} {IDS[dtype]}"
    _set_counter(m, 0)
    m.eval()
    r = _forward(m, x)
    assert _counter(m) == 0                      # eval leaves the counter
    check_hidden(r, p, np.ones((B, 128), bool), False, tag + " eval")
    m.train()
    first = None
    for start in (0, 1, 2 ** 40 + 5, 2 ** 40 + 6, 2 ** 64 - 1):
        if _counter(m) != start:
            _set_counter(m, start)
        r = _forward(m, x)
        assert _counter(m) == (start + 1) % 2 ** 64, start   # each train forward adds exactly 1
        keep1 = rd.keep_masks(SEED, start, B)[0]
        decided = check_hidden(r, p, keep1, True, f"{tag} counter {start}")
        if first is None:
            first = (r, decided, keep1)
    assert not np.array_equal(first[2], rd.keep_masks(SEED, 1, B)[0])
    m.eval()
    _forward(m, x)
    assert _counter(m) == 0                      # 2^64 - 1 wrapped to 0; eval left it
    # the phase-2 train route draws the same masks at the same counter
    m.train()
    m.train_route = "phase2"
    _set_counter(m, 0)
    r2 = _forward(m, x)
    assert _counter(m) == 1
    d2 = check_hidden(r2, p, first[2], True, tag + " phase2 counter 0")
    both = first[1] & d2
    assert ((r2["h1_bits"].numpy() == 0) == (first[0]["h1_bits"].numpy() == 0))[both].all()
