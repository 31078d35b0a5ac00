"""float64 restatement of the K5 DSAM legs (forward, dX, dW/db) and the element-wise comparator
of tests/test_gpu_dsam_parity.py.  CPU, plain torch.

DSAModule.forward (custom_model.py:682-699) is

    y = sum_{i<4} Conv3x3s2_i(x * m_i) + sum_{i<n_masks[b]} b_i + Proj3x3s2(x) (+ residual),

m_i = bit i of the region code of the SOURCE pixel.  The float32 legs compute that formula with
the float32 filters (``*_literal``).  The bfloat16 forward / dX regroup it by code k: a source pixel
of code k meets the merged filter Wq_k = bf16(proj + sum_{i in k} conv_i), summed in float32 with
proj first and conv_0..3 ascending and rounded once (``merged_filters``; the packed layout is
pinned bit for bit by test_pack_codes_layout_bit_exact), so their reference is on Wq_k
(``*_merged``).  dW/db have no filter quantisation: one reference for both precisions.

Every reference returns (value, A): A is the same expression with every operand replaced by its
absolute value, the sum of the magnitudes of the summands of each output element.
All tensors are NCHW float64; ``code`` is an integer [B,h,w] map, ``n_masks`` a length-B sequence."""
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
BF16_REL = 2.0 ** -8  # one round-to-nearest of a result to bf16 (8 significant bits)


def bf16(t):
    """float32 tensor rounded to bfloat16 (round to nearest even), back as float32."""
    return t.float().bfloat16().float()


def merged_filters(conv_w, proj_w, each_add=False):
    """[16,Co,Ci,3,3] float64: Wq_k = bf16(proj + sum_{i in k} conv_i), float32 sums in ascending
    order, one rounding at the end.  ``each_add`` rounds after every addition (a mutant)."""
    out = []
    for k in range(16):
        t = bf16(proj_w) if each_add else proj_w.float().clone()
        for i in range(4):
            if (k >> i) & 1:
                t = t + conv_w[i].float()
                if each_add:
                    t = bf16(t)
        out.append(bf16(t).double())
    return torch.stack(out)


def bias_prefix(bias4, n_masks):
    """[B,Co]: sum_{i < n_masks[b]} b_i, and the same of |b_i|."""
    b = bias4.double()
    z = torch.zeros_like(b[0])
    s = torch.stack([b[:int(n)].sum(0) if n > 0 else z for n in n_masks])
    a = torch.stack([b[:int(n)].abs().sum(0) if n > 0 else z for n in n_masks])
    return s, a


def _conv(x, w):
    return F.conv2d(x, w, stride=2, padding=1)


def _convt(gy, w, h, w_):
    ho, wo = gy.shape[2:]
    return F.conv_transpose2d(gy, w, stride=2, padding=1, output_padding=(h - (2 * ho - 1), w_ - (2 * wo - 1)))


def fwd_merged(x, code, n_masks, wq, bias4, residual=None):
    x = x.double()
    y = a = 0.0
    for k in code.unique().tolist():
        m = (code == k)[:, None].double()
        y = y + _conv(x * m, wq[k])
        a = a + _conv(x.abs() * m, wq[k].abs())
    s, sa = bias_prefix(bias4, n_masks)
    y, a = y + s[:, :, None, None], a + sa[:, :, None, None]
    if residual is not None:
        y, a = y + residual.double(), a + residual.double().abs()
    return y, a


def fwd_literal(x, code, n_masks, conv_w, proj_w, bias4, residual=None):
    x, cw, pw = x.double(), conv_w.double(), proj_w.double()
    y, a = _conv(x, pw), _conv(x.abs(), pw.abs())
    for i in range(4):
        m = ((code >> i) & 1)[:, None].double()
        y = y + _conv(x * m, cw[i])
        a = a + _conv(x.abs() * m, cw[i].abs())
    s, sa = bias_prefix(bias4, n_masks)
    y, a = y + s[:, :, None, None], a + sa[:, :, None, None]
    if residual is not None:
        y, a = y + residual.double(), a + residual.double().abs()
    return y, a


def dx_merged(gy, code, wq, gin=None):
    gy = gy.double()
    _, h, w = code.shape
    d = a = 0.0
    for k in code.unique().tolist():
        m = (code == k)[:, None].double()  # the code of the destination pixel
        d = d + m * _convt(gy, wq[k], h, w)
        a = a + m * _convt(gy.abs(), wq[k].abs(), h, w)
    if gin is not None:
        d, a = d + gin.double(), a + gin.double().abs()
    return d, a


def dx_literal(gy, code, conv_w, proj_w, gin=None):
    gy, cw, pw = gy.double(), conv_w.double(), proj_w.double()
    _, h, w = code.shape
    d, a = _convt(gy, pw, h, w), _convt(gy.abs(), pw.abs(), h, w)
    for i in range(4):
        m = ((code >> i) & 1)[:, None].double()
        d = d + m * _convt(gy, cw[i], h, w)
        a = a + m * _convt(gy.abs(), cw[i].abs(), h, w)
    if gin is not None:
        d, a = d + gin.double(), a + gin.double().abs()
    return d, a


def _dw_one(xm, gy):
    """d/dW of sum conv2d(xm, W) * gy: im2col rows of xm against gy.  -> [Co,Ci,3,3]"""
    Ci = xm.shape[1]
    cols = F.unfold(xm, 3, stride=2, padding=1)  # [B, Ci*9, ho*wo]
    return torch.einsum("bol,bkl->ok", gy.flatten(2), cols).reshape(gy.shape[1], Ci, 3, 3)


def dw_ref(x, gy, code, n_masks):
    """-> dict dconv [4,Co,Ci,3,3], dproj [Co,Ci,3,3], dbias [4,Co], each a pair (value, S)."""
    x, gy = x.double(), gy.double()
    xa, ga = x.abs(), gy.abs()
    dc, sc = [], []
    for i in range(4):
        m = ((code >> i) & 1)[:, None].double()
        dc.append(_dw_one(x * m, gy))
        sc.append(_dw_one(xa * m, ga))
    nm = torch.as_tensor([int(n) for n in n_masks])
    db, sb = [], []
    for i in range(4):
        live = (nm > i).double()[:, None]
        db.append((gy.sum((2, 3)) * live).sum(0))
        sb.append((ga.sum((2, 3)) * live).sum(0))
    return dict(dconv=(torch.stack(dc), torch.stack(sc)), dproj=(_dw_one(x, gy), _dw_one(xa, ga)),
                dbias=(torch.stack(db), torch.stack(sb)))


def compare(got, ref, A, K, rel=0.0):
    """Element-wise |got - ref| <= rel * |ref| + K * EPS * A over every element.
    -> (largest error / bound, share of elements over the bound).  Where the bound is zero (no
    live summand) the value must be exactly zero: any error there counts as an infinite ratio."""
    got, ref, A = got.detach().double().cpu(), ref.double(), A.double()
    assert got.shape == ref.shape == A.shape, (got.shape, ref.shape, A.shape)
    assert bool(torch.isfinite(got).all()), "non-finite output"
    err = (got - ref).abs()
    bound = rel * ref.abs() + K * EPS * A
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300),
                        torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max()), float((ratio > 1).double().mean())
