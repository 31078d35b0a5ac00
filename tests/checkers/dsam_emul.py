"""The arithmetic of the bf16 K5 legs emulated in torch float32 on the CPU, tap by tap and code by
code on the quantised operands, with the mutations tests/test_dsam_ref.py must see rejected by
the comparator of checkers/dsam_ref.py.  Nothing here runs on the GPU or reads a HIP result.

``mutant`` (one at most):
  bias_prefix    forward: the bias prefix of one image (the first with n_masks > 0) is n_masks - 1
  each_add       forward: the merged filter is rounded to bf16 after every addition (dX accepts it
                 too; the tests judge it on the forward's float32 output, see test_dsam_ref)
  code_dst       forward: every tap takes the region code of the output pixel's centre source
  code_src       dX: the code of the gradient pixel's centre source, not of the destination pixel
  right_edge     forward: a tap one column past the right edge reads the next row's first pixel
  prev_image     forward, linear tiles: the rows of a 128-row tile that lie past an image boundary
                 take the n_masks of the image the tile started in
  drop_unit      dW: the last, ragged 64-pixel unit of the last image is left out
  drop_kk        dW: the last 9 Cin % 128 columns kk = tap * Cin + c are left out
  db_all         db: summed over all images regardless of n_masks
"""
import torch
import torch.nn.functional as F

from checkers import dsam_cases as cases
from checkers import dsam_ref as R


def _wq(i, mutant):
    return R.merged_filters(i["conv_w"], i["proj_w"], each_add=mutant == "each_add").float()


def fwd(name, i, code, mutant=None):
    """float32 [B,Co,ho,wo]: residual + (acc + bias prefix), before the bf16 rounding of the output."""
    B, Ci, Co, h, w = cases.CASES[name]
    ho, wo = (h + 1) // 2, (w + 1) // 2
    wq = _wq(i, mutant)
    P = B * h * w
    xf = torch.cat([i["x"].permute(0, 2, 3, 1).reshape(P, Ci), torch.zeros((1, Ci))])
    cf = torch.cat([code.reshape(P), torch.zeros((1,), dtype=code.dtype)])
    bb = torch.arange(B)[:, None, None]
    oy, ox = torch.arange(ho)[None, :, None], torch.arange(wo)[None, None, :]
    centre = code[bb, 2 * oy, 2 * ox]
    acc = torch.zeros((B, Co, ho, wo))
    for ky in range(3):
        for kx in range(3):
            iy, ix = 2 * oy - 1 + ky, 2 * ox - 1 + kx
            rows = (iy >= 0) & (iy < h)
            inb = rows & (ix >= 0) & (ix < w)
            if mutant == "right_edge":
                inb = rows & (ix >= 0) & (ix <= w)
            idx = ((bb * h + iy) * w + ix).expand(B, ho, wo)
            idx = torch.where(inb.expand(B, ho, wo) & (idx < P), idx, torch.full_like(idx, P))
            xs = xf[idx]  # [B,ho,wo,Ci]
            cs = centre if mutant == "code_dst" else cf[idx]
            live = idx < P
            for k in cs[live].unique().tolist():
                m = ((cs == k) & live)[..., None].float()
                acc = acc + torch.einsum("bhwc,oc->bohw", xs * m, wq[k][:, :, ky, kx])
    n = torch.tensor(i["n_masks"])[:, None, None].expand(B, ho, wo).clone()
    if mutant == "bias_prefix":
        b0 = next(b for b, v in enumerate(i["n_masks"]) if v > 0)
        n[b0] -= 1
    if mutant == "prev_image" and cases.conv_variant("fwd", *cases.CASES[name])["linear"]:
        m = torch.arange(B * ho * wo)
        n = torch.tensor(i["n_masks"])[(m // cases.LD_BM * cases.LD_BM) // (ho * wo)].reshape(B, ho, wo)
    pre = torch.cat([torch.zeros((1, Co)), torch.cumsum(i["bias4"], 0)])  # float32, ascending
    return i["residual"] + (acc + pre[n].permute(0, 3, 1, 2))


def dx(name, i, code, mutant=None):
    """float32 [B,Ci,h,w]: gin + acc, before the bf16 rounding of the output."""
    B, Ci, Co, h, w = cases.CASES[name]
    ho, wo = (h + 1) // 2, (w + 1) // 2
    wq = _wq(i, mutant)
    Q = B * ho * wo
    gf = torch.cat([i["gy"].permute(0, 2, 3, 1).reshape(Q, Co), torch.zeros((1, Co))])
    bb = torch.arange(B)[:, None, None]
    yy, xx = torch.arange(h)[None, :, None], torch.arange(w)[None, None, :]
    acc = torch.zeros((B, Ci, h, w))
    for ky in range(3):
        for kx in range(3):
            ny, nx = yy + 1 - ky, xx + 1 - kx
            ok = (ny % 2 == 0) & (ny >= 0) & (ny // 2 < ho) & (nx % 2 == 0) & (nx >= 0) & (nx // 2 < wo)
            oy, ox = (ny // 2).clamp(0, ho - 1), (nx // 2).clamp(0, wo - 1)
            idx = torch.where(ok, (bb * ho + oy) * wo + ox, torch.tensor(Q)).expand(B, h, w)
            g = gf[idx]  # [B,h,w,Co]
            cs = code[bb, 2 * oy, 2 * ox] if mutant == "code_src" else code
            live = idx < Q
            for k in cs[live].unique().tolist():
                m = ((cs == k) & live)[..., None].float()
                acc = acc + torch.einsum("bhwo,oc->bchw", g * m, wq[k][:, :, ky, kx])
    return i["gin"] + acc


def dw(name, i, code, mutant=None):
    """float32 dict dconv [4,Co,Ci,3,3], dproj [Co,Ci,3,3], dbias [4,Co] from the bf16 x and gy."""
    B, Ci, Co, h, w = cases.CASES[name]
    ho, wo = (h + 1) // 2, (w + 1) // 2
    v = cases.wgrad_variant(*cases.CASES[name])
    gy = i["gy"].clone()
    if mutant == "drop_unit" and v["unit_tail"]:
        gy.view(B, Co, ho * wo)[B - 1, :, (v["nunit"] - 1) * cases.WPX:] = 0
    g2 = gy.flatten(2)

    def one(xm):
        cols = F.unfold(xm, 3, stride=2, padding=1)
        d = torch.einsum("bol,bkl->ok", g2, cols).reshape(Co, Ci, 3, 3)
        if mutant == "drop_kk" and v["kk_tail"]:
            kk = d.permute(0, 2, 3, 1).reshape(Co, 9 * Ci).clone()  # kk = tap * Cin + c
            kk[:, 9 * Ci // 128 * 128:] = 0
            d = kk.reshape(Co, 3, 3, Ci).permute(0, 3, 1, 2)
        return d
    dconv = torch.stack([one(i["x"] * ((code >> b) & 1)[:, None].float()) for b in range(4)])
    nm = torch.tensor(i["n_masks"])
    s = i["gy"].sum((2, 3))  # [B,Co]
    dbias = torch.stack([(s * (torch.ones(B) if mutant == "db_all" else (nm > b).float())[:, None]).sum(0)
                         for b in range(4)])
    return dict(dconv=dconv, dproj=one(i["x"]), dbias=dbias)
