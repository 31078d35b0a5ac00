"""Float64 restatement of K2, the DGGM gated fusion (csrc/dggm.hip, rgbd_dggm_fuse_fwd / _bwd):

    out = (cp1 +) color + ReLU(W . (bilinear(grad) * nearest(mask)) + b),   dW, db

Only the source indices and the bilinear weight are float32, computed op for op the way torch's
float32 upsample kernels do (float64 F.interpolate computes the scale in double and may pick
other cells):

    bilinear (align_corners=False): scale = f32(in) / f32(out)
                                    s  = max(scale * (dst + 0.5f) - 0.5f, 0)   one rounding per op
                                    i0 = int(s), i1 = i0 + (i0 < in - 1), l1 = s - i0
    nearest (legacy floor):         min(floor(f32(dst) * scale), in - 1)

Everything after them is float64 on the widened inputs.  Next to the values the checker returns
the per-element sums of magnitudes that a float32 evaluation's rounding error scales with, and
the set of elements whose pre-activation is so close to zero that a float32 evaluation may
legitimately take the other ReLU branch.  Plain numpy / torch; nothing of the package is imported.
"""
import numpy as np
import torch

F32 = np.float32
NEAR_REL = 1e-5  # |pre| <= NEAR_REL * A_pre: about ten float32 rounding bounds of a 4-term sum


def bilinear_index(n_in, n_out, fma=False):
    """-> (i0, i1, l1): int64, int64, float32 arrays of length n_out.

    ``fma``: round scale * (dst + 0.5f) - 0.5f once, as a compiler that contracts it into a fused
    multiply-add does (the float64 product of two float32 is exact).  Both roundings are float32
    evaluations of the same expression; they differ by at most one ulp of the product, which is
    2^-17 of a source pixel at coordinate 64..128 and goes into the weight l1 in full."""
    scale = F32(n_in) / F32(n_out)
    dst = np.arange(n_out, dtype=F32) + F32(0.5)
    if fma:
        s = (np.float64(scale) * dst.astype(np.float64) - 0.5).astype(F32)
    else:
        s = scale * dst - F32(0.5)
    s = np.maximum(s, F32(0))
    assert s.dtype == F32
    i0 = s.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = s - i0.astype(F32)
    return i0, i1, l1


def nearest_index(n_in, n_out):
    scale = F32(n_in) / F32(n_out)
    s = np.floor(np.arange(n_out, dtype=F32) * scale)
    assert s.dtype == F32
    return np.minimum(s.astype(np.int64), n_in - 1)


def gate(grad, mask, h, w, fma=False):
    """g[b, k, y, x] = bilinear(grad[b, k]) * mask[b, 0, nearest]; float64 [B, 3, h, w]."""
    grad = torch.as_tensor(grad).double()
    mask = torch.as_tensor(mask).double()
    H, W = grad.shape[-2:]
    y0, y1, ly1 = bilinear_index(H, h, fma)
    x0, x1, lx1 = bilinear_index(W, w, fma)
    ly1 = torch.from_numpy(ly1.astype(np.float64))[:, None]
    lx1 = torch.from_numpy(lx1.astype(np.float64))[None, :]
    ly0, lx0 = 1.0 - ly1, 1.0 - lx1
    y0, y1, x0, x1 = (torch.from_numpy(a) for a in (y0, y1, x0, x1))

    def tap(yi, xi):
        return grad[:, :, yi[:, None], xi[None, :]]

    bil = ly0 * (lx0 * tap(y0, x0) + lx1 * tap(y0, x1)) + ly1 * (lx0 * tap(y1, x0) + lx1 * tap(y1, x1))
    ny = torch.from_numpy(nearest_index(H, h))
    nx = torch.from_numpy(nearest_index(W, w))
    return bil * mask[:, :, ny[:, None], nx[None, :]]


def dggm_ref(grad, mask, color, weight, bias, cp1=None, dout=None, keep=None, fma=False):
    """grad [B,3,H,W], mask [B,1,H,W], color / cp1 / dout [B,C,h,w], weight [C,3(,1,1)], bias [C].

    -> dict of float64 tensors:
         out, pre [B,C,h,w]; A_pre = |b| + sum_k |w_k||g_k|; A_out = |cp1| + |color| + A_pre;
         near = |pre| <= NEAR_REL * A_pre (bool)
       and with ``dout``:
         db [C], dw [C,3] and S_db, S_dw, the sums of the absolute summands of each entry.
    ``keep`` (bool, broadcastable to [B,1,h,w]) restricts the dW/db sums to those pixels;
    ``fma`` as in bilinear_index."""
    color = torch.as_tensor(color).double()
    B, C, h, w = color.shape
    wt = torch.as_tensor(weight).double().reshape(C, 3)
    bs = torch.as_tensor(bias).double().reshape(C)
    g = gate(grad, mask, h, w, fma)                                      # [B,3,h,w]
    pre = bs[None, :, None, None] + torch.einsum("ck,bkyx->bcyx", wt, g)
    a_pre = bs.abs()[None, :, None, None] + torch.einsum("ck,bkyx->bcyx", wt.abs(), g.abs())
    out = color + pre.clamp_min(0.0)
    a_out = color.abs() + a_pre
    if cp1 is not None:
        cp1 = torch.as_tensor(cp1).double()
        out = cp1 + out
        a_out = cp1.abs() + a_out
    r = dict(out=out, pre=pre, A_pre=a_pre, A_out=a_out, near=pre.abs() <= NEAR_REL * a_pre, gate=g)
    if dout is not None:
        d = torch.as_tensor(dout).double() * (pre > 0)
        if keep is not None:
            d = d * torch.as_tensor(keep).reshape(-1, 1, h, w).double()
        r["db"] = d.sum(dim=(0, 2, 3))
        r["S_db"] = d.abs().sum(dim=(0, 2, 3))
        r["dw"] = torch.einsum("bcyx,bkyx->ck", d, g)
        r["S_dw"] = torch.einsum("bcyx,bkyx->ck", d.abs(), g.abs())
    return r


def ratio(err, bound):
    """max of err / bound over the entries with bound > 0; an entry with bound == 0 must have
    err == 0 (inf otherwise)."""
    err, bound = torch.as_tensor(err).double().abs(), torch.as_tensor(bound).double()
    pos = bound > 0
    if bool((err[~pos] > 0).any()):
        return float("inf")
    return float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
