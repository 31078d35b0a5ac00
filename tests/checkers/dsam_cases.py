"""Shapes, region-code maps, seeded inputs and error constants shared by tests/test_dsam_cases.py
(CPU: the table reaches every kernel variant), tests/test_dsam_ref.py (CPU: pins the float64
checker of checkers/dsam_ref.py, measures the constants) and tests/test_gpu_dsam_parity.py (K5
against it).

Inputs: x and residual ~ N(0,1), gy and gin ~ 0.1 N(0,1), filters ~ 0.05 N(0,1), biases
~ 0.1 N(0,1) pushed to |b| >= 0.02 (a wrong bias prefix then moves an output by 2^10 bounds or
more).  n_masks of an image is (4 g + 3) % 5 with g the image's index counted through the table
(case A holds images 0-1, B 2-4, ...): with at most three images per case, a count restarted at
every case would only ever give 3, 2, 1; counted through, cases A to F meet all of 0..4 (the
float32 legs run A to G).

Error constants of the bounds |hip - ref64| <= K * 2^-24 * A (A, S: sum of the magnitudes of an
element's summands, checkers/dsam_ref.py): 8 times the largest such ratio that torch's own CPU
float32 evaluation of the same expression on the same operands reaches against the checker
(``cpu_float32_ratios``: float32 conv2d / conv_transpose2d / im2col-einsum, merged by code on the
bf16-quantised filters for the bf16 legs, the literal five-convolution formula for the float32
legs), over every case and code map below.  The factor 8 pays for the kernels' different
summation order (MFMA k-blocks, per-code steps, split-K chunk partials summed in chunk order):
reordering n random-sign terms moves the rounding error by a small factor, not by n.  The
rigorous ceiling would be the number of summands (9 Cin + 6 forward, 9 Cout + 1 dX, B ho wo dW).
tests/test_dsam_ref.py measures the ratios again and asserts that the constants cover 8 times
them.  ``cpu_float32_ratios`` runs torch on ONE thread (the blocking of its CPU kernels, hence
their summation order, follows the thread count: dX reads 6.35 at eight threads).  Measured so
with the torch build the suite runs on (largest over the five code maps):

    forward  bf16-merged 1.05 (F1 fifteen)  float32 literal 1.91 (A zero)
    dX       bf16-merged 2.95 (D fifteen)   float32 literal 5.76 (B zero)
    dconv    bf16 3.10 (B const0)           float32 5.52 (B rand)
    dproj    bf16 2.94 (E)                  float32 5.22 (D)
    db       bf16 0.11 (C)                  float32 0.93 (F2)

torch's transposed convolution (col2im) is three times further from float64 than its forward,
so the rule is applied per leg and the forward keeps the tighter constant:
K5_F = 8 * 1.91 -> 16 (forward, both precisions and interfaces), K5_X = 8 * 5.76 -> 47 (dX),
K5_B = 8 * 5.52 -> 45 (dW and db).  All are below the smallest ceiling they meet (78 summands in
the forward of case G1, 217 in its dX) except K5_B at the one-row maps of case F (1 and 10
summands per dW element): ``k_of`` caps every constant at the case's number of summands."""
import functools

import torch

K5_F = 16
K5_X = 47
K5_B = 45
EPS = 2.0 ** -24

# name -> (B, Cin, Cout, h, w)
BF16_CASES = {
    "A": (2, 32, 32, 15, 31),
    "B": (3, 64, 160, 30, 33),
    "C": (1, 96, 224, 29, 32),
    "D": (2, 128, 256, 9, 13),
    "E": (2, 192, 192, 16, 32),
    "F1": (1, 32, 64, 1, 1),
    "F2": (2, 32, 32, 1, 9),
}
F32_ONLY_CASES = {
    "G1": (2, 8, 24, 7, 9),
    "G2": (2, 40, 72, 13, 18),
}
CASES = {**BF16_CASES, **F32_ONLY_CASES}
MAPS = ("rand", "zero", "fifteen", "scene", "const0")


def first_image(name):
    """Index of the case's image 0 counted through the table (the bf16 cases, then the float32-only ones)."""
    g = 0
    for n, s in CASES.items():
        if n == name:
            return g
        g += s[0]
    raise KeyError(name)


def n_masks_of(name):
    g0 = first_image(name)
    return [(4 * (g0 + b) + 3) % 5 for b in range(CASES[name][0])]


# ---------------------------------------------------------------- the kernels' plan arithmetic
# Python restatement of ld_kc / ld_linear / ld_plan (csrc/dsam_lds.hip) and wg_fm / wg_plan
# (csrc/dsam_wgrad.hip): which instantiation and tiling a shape lands on.
LD_BM, LD_BN, WPX = 128, 192, 64


def ld_kc(C):
    return 3 if C % 96 == 0 else (2 if C % 64 == 0 else 1)


def ld_linear(Hc, Wc):
    blk = ((Hc + 7) // 8 * 8) * ((Wc + 15) // 16 * 16)
    return Hc * Wc * 100 < 85 * blk


def wg_fm(Cout):
    return 6 if Cout % 192 == 0 else (4 if Cout % 128 == 0 else 2)


def class_sizes(h, w):
    """(Hc, Wc) of the four dX parity classes (py, px) = (cls >> 1, cls & 1) of an h x w input grid."""
    return [((h - (c >> 1) + 1) >> 1, (w - (c & 1) + 1) >> 1) for c in range(4)]


def conv_variant(kind, B, Cin, Cout, h, w):
    """kind 'fwd' / 'dx' -> dict(kc, ncg, ntn, n_last, linear, exact, crosses): the implicit GEMM's
    channel count C and column count N, the grid the 128-row tiles cover (the largest parity class for
    dX), whether 8x16 blocks tile it exactly, and whether a linear tile spans two images."""
    ho, wo = (h + 1) // 2, (w + 1) // 2
    C, N = (Cin, Cout) if kind == "fwd" else (Cout, Cin)
    Hc, Wc = (ho, wo) if kind == "fwd" else ((h + 1) // 2, (w + 1) // 2)
    kc = ld_kc(C)
    lin = ld_linear(Hc, Wc)
    return dict(kc=kc, ncg=C // (32 * kc), ntn=-(-N // LD_BN), n_last=N - (-(-N // LD_BN) - 1) * LD_BN, linear=lin,
                exact=(not lin) and Hc % 8 == 0 and Wc % 16 == 0,
                crosses=lin and B > 1 and (Hc * Wc) % LD_BM != 0, classes=class_sizes(h, w) if kind == "dx" else None)


def wgrad_variant(B, Cin, Cout, h, w):
    hwo = ((h + 1) // 2) * ((w + 1) // 2)
    fm = wg_fm(Cout)
    return dict(fm=fm, nunit=-(-hwo // WPX), unit_tail=hwo % WPX, ntile_kk=-(-9 * Cin // 128), kk_tail=9 * Cin % 128,
                ntile_o=-(-Cout // (32 * fm)), o_tail=Cout % (32 * fm))


# ---------------------------------------------------------------- region-code maps
def code_map(name, kind):
    """int64 [B,h,w].  rand: every pixel uniform over the 16 codes; zero / fifteen: one code
    everywhere (projection only / all four masks: the packing mask has one bit); scene: code 1 with
    a rectangle of code 3, one of code 12 and a two-pixel border of code 5; const0: image 0 all
    code 6, the other images random."""
    B, _, _, h, w = CASES[name]
    g = torch.Generator().manual_seed(1000 + 17 * list(CASES).index(name) + MAPS.index(kind))
    if kind in ("rand", "const0"):
        c = torch.randint(0, 16, (B, h, w), generator=g)
        if kind == "const0":
            c[0] = 6
        return c
    if kind == "zero":
        return torch.zeros((B, h, w), dtype=torch.int64)
    if kind == "fifteen":
        return torch.full((B, h, w), 15, dtype=torch.int64)
    assert kind == "scene"
    c = torch.ones((B, h, w), dtype=torch.int64)
    c[:, h // 6:h // 2 + 1, w // 8:w // 2] = 3
    c[:, h // 3:h - h // 5, w // 2 - 1:w - w // 6] = 12
    c[:, :2], c[:, -2:], c[:, :, :2], c[:, :, -2:] = 5, 5, 5, 5
    return c


# ---------------------------------------------------------------- inputs and references
@functools.lru_cache(maxsize=None)
def inputs(name, bf16):
    """Shared, do not modify.  NCHW float32 tensors (rounded to bf16 values when ``bf16``; filters
    and biases stay float32, as the modules keep them): x, gin [B,Ci,h,w]; residual, gy
    [B,Co,ho,wo]; conv_w [4,Co,Ci,3,3]; proj_w [Co,Ci,3,3]; bias4 [4,Co]; n_masks."""
    B, Ci, Co, h, w = CASES[name]
    ho, wo = (h + 1) // 2, (w + 1) // 2
    g = torch.Generator().manual_seed(5000 + list(CASES).index(name))
    rnd = lambda *s: torch.randn(s, generator=g)
    q = (lambda t: t.bfloat16().float()) if bf16 else (lambda t: t)
    x, res = q(rnd(B, Ci, h, w)), q(rnd(B, Co, ho, wo))
    gy, gin = q(0.1 * rnd(B, Co, ho, wo)), q(0.1 * rnd(B, Ci, h, w))
    conv_w, proj_w = 0.05 * rnd(4, Co, Ci, 3, 3), 0.05 * rnd(Co, Ci, 3, 3)
    b = 0.1 * rnd(4, Co)
    bias4 = torch.where(b >= 0, b.clamp_min(0.02), b.clamp_max(-0.02))
    return dict(x=x, residual=res, gy=gy, gin=gin, conv_w=conv_w, proj_w=proj_w, bias4=bias4,
                n_masks=n_masks_of(name))


@functools.lru_cache(maxsize=None)
def reference(name, kind, bf16):
    """Shared, do not modify.  (inputs, code, refs): refs maps y / dx / dconv / dproj / dbias to
    (float64 value, magnitude), merged by code on the quantised filters when ``bf16``, literal
    otherwise; y includes the residual and dx the incoming gradient gin."""
    from checkers import dsam_ref as R
    i = inputs(name, bf16)
    code = code_map(name, kind)
    if bf16:
        wq = R.merged_filters(i["conv_w"], i["proj_w"])
        y = R.fwd_merged(i["x"], code, i["n_masks"], wq, i["bias4"], i["residual"])
        dx = R.dx_merged(i["gy"], code, wq, i["gin"])
    else:
        y = R.fwd_literal(i["x"], code, i["n_masks"], i["conv_w"], i["proj_w"], i["bias4"], i["residual"])
        dx = R.dx_literal(i["gy"], code, i["conv_w"], i["proj_w"], i["gin"])
    return i, code, dict(y=y, dx=dx, **R.dw_ref(i["x"], i["gy"], code, i["n_masks"]))


def cpu_float32_ratios(name, kind, bf16):
    """torch's CPU float32 evaluation of the reference's own expression on the same operands,
    against the reference with K = 1: dict leg -> largest |f32 - ref| / (EPS * A).  The yardstick
    K5_F and K5_B come from; nothing of the HIP kernels enters."""
    i, code, ref = reference(name, kind, bf16)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # the summation order of torch's CPU kernels depends on the thread count
    try:
        return _cpu_float32_ratios(name, i, code, ref, bf16)
    finally:
        torch.set_num_threads(threads)


def _cpu_float32_ratios(name, i, code, ref, bf16):
    import torch.nn.functional as F
    from checkers import dsam_ref as R
    B, Ci, Co, h, w = CASES[name]
    x, gy = i["x"], i["gy"]
    conv = lambda t, wt: F.conv2d(t, wt, stride=2, padding=1)
    convt = lambda t, wt: F.conv_transpose2d(t, wt, stride=2, padding=1,
                                             output_padding=(h - (2 * gy.shape[2] - 1), w - (2 * gy.shape[3] - 1)))
    z = torch.zeros((Co,))
    bias = torch.stack([i["bias4"][:n].sum(0) if n > 0 else z for n in i["n_masks"]])[:, :, None, None]
    if bf16:
        wq = R.merged_filters(i["conv_w"], i["proj_w"]).float()
        ks = code.unique().tolist()
        y = sum(conv(x * (code == k)[:, None].float(), wq[k]) for k in ks)
        dx = sum((code == k)[:, None].float() * convt(gy, wq[k]) for k in ks)
    else:
        bit = lambda n: ((code >> n) & 1)[:, None].float()
        y = conv(x, i["proj_w"]) + sum(conv(x * bit(n), i["conv_w"][n]) for n in range(4))
        dx = convt(gy, i["proj_w"]) + sum(bit(n) * convt(gy, i["conv_w"][n]) for n in range(4))
    y, dx = i["residual"] + (y + bias), i["gin"] + dx
    cw = i["conv_w"].clone().requires_grad_(True)
    pw = i["proj_w"].clone().requires_grad_(True)
    b4 = i["bias4"].clone().requires_grad_(True)
    out = conv(x, pw) + sum(conv(x * ((code >> n) & 1)[:, None].float(), cw[n]) for n in range(4))
    out = out + torch.stack([b4[:n].sum(0) if n > 0 else b4[:1].sum(0) * 0 for n in i["n_masks"]])[:, :, None, None]
    out.backward(gy)
    got = dict(y=y, dx=dx, dconv=cw.grad, dproj=pw.grad, dbias=b4.grad)
    return {leg: R.compare(got[leg], ref[leg][0], ref[leg][1], 1.0)[0] for leg in got}


def summands(name):
    """The rigorous ceiling of each constant: the number of summands of one output element."""
    B, Ci, Co, h, w = CASES[name]
    n = B * ((h + 1) // 2) * ((w + 1) // 2)
    return dict(y=9 * Ci + 6, dx=9 * Co + 1, dconv=n, dproj=n, dbias=n)


def k_of(name, leg):
    """The constant of leg y / dx / dconv / dproj / dbias at case ``name``."""
    return min(dict(y=K5_F, dx=K5_X).get(leg, K5_B), summands(name)[leg])

