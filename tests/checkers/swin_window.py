"""Float64 restatement of what Hugging Face's ``SwinLayer`` does around its attention core, taking
exactly the arguments of ``rgbd_swin_window_attn`` (csrc/swin_attn.hip): per-token q / k / v rows
of the ORIGINAL ``H x W`` map, the projection biases (a padded position is a zero row, whose
projection is the bias), the relative-position table, the shift and the scale.

tests/test_oracle_swin_window.py pins it against the installed ``SwinLayer`` itself; the GPU test
(tests/test_gpu_swin_window.py) holds the kernel to it.
"""
import torch

WS = 7


def _region(n, shift):
    i = torch.arange(n)
    return (i >= n - WS).long() + (i >= n - shift).long()


def window_attention_ref(q, k, v, bq, bk, bv, table, B, H, W, heads, shift, scale):
    """q / k / v [B*H*W, C] (any float dtype, C = heads * head_dim), bq / bk / bv [C] or None,
    table [169, heads] -> out [B*H*W, C] float64."""
    C = q.shape[1]
    hd = C // heads
    Hp, Wp = -(-H // WS) * WS, -(-W // WS) * WS
    nwy, nwx = Hp // WS, Wp // WS

    def windows(x, bias):
        # 1. the padded Hp x Wp map: the bias row outside H x W
        row = torch.zeros(C, dtype=torch.float64) if bias is None else bias.double().cpu()
        m = row.expand(B, Hp, Wp, C).clone()
        m[:, :H, :W] = x.double().cpu().view(B, H, W, C)
        # 2. roll by -shift
        if shift > 0:
            m = torch.roll(m, shifts=(-shift, -shift), dims=(1, 2))
        # 3. 7x7 windows per head: [B, nwy, nwx, heads, 49, hd]
        m = m.view(B, nwy, WS, nwx, WS, heads, hd).permute(0, 1, 3, 5, 2, 4, 6)
        return m.reshape(B, nwy, nwx, heads, WS * WS, hd)

    Q, K, V = windows(q, bq), windows(k, bk), windows(v, bv)
    # 4. S = Q K^T scale + table[(qy - ky + 6) * 13 + (qx - kx + 6)]
    t = torch.arange(WS * WS)
    ty, tx = t // WS, t % WS
    idx = (ty[:, None] - ty[None, :] + WS - 1) * (2 * WS - 1) + (tx[:, None] - tx[None, :] + WS - 1)
    bias = table.double().cpu()[idx.reshape(-1)].view(WS * WS, WS * WS, heads).permute(2, 0, 1)
    S = Q @ K.transpose(-1, -2) * float(scale) + bias
    # 5. -100 between tokens of different shift regions (regions of the padded, rolled map)
    if shift > 0:
        reg = 3 * _region(Hp, shift)[:, None] + _region(Wp, shift)[None, :]        # [Hp, Wp]
        reg = reg.view(nwy, WS, nwx, WS).permute(0, 2, 1, 3).reshape(nwy, nwx, WS * WS)
        differ = reg[:, :, :, None] != reg[:, :, None, :]
        S = S + (-100.0 * differ.double())[None, :, :, None]
    # 6. softmax, P V, un-window, roll back, crop
    O = torch.softmax(S, dim=-1) @ V
    O = O.view(B, nwy, nwx, heads, WS, WS, hd).permute(0, 1, 4, 2, 5, 3, 6).reshape(B, Hp, Wp, C)
    if shift > 0:
        O = torch.roll(O, shifts=(shift, shift), dims=(1, 2))
    return O[:, :H, :W].reshape(B * H * W, C).contiguous()
