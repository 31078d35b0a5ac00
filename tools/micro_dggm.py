"""Micro benchmark of the DGGM fused fwd / bwd entry points at the bench's four scales (B=8,
640x480, bf16), each timed with CUDA events over --iters calls.

Per-scale lines fwd<k> / bwd<k>: the single-scale calls (one-scale launches of the multi-scale
kernels).  Hot-path lines: the calls hot_path.py makes in bf16 mode: fwd012 (scales 0-2 in one
launch, cp1 of scales 1 and 2 NHWC), fwd3 (scale 3, cp1 NHWC) and bwd0123 (all four scales: one
partial launch + one final launch)."""
import argparse, os, sys
_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R]
import torch
import _rgbd_import  # noqa: F401
from rgbd_amd import ops
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
a = ap.parse_args()
dev = torch.device("cuda")
B, H, W = 8, 480, 640
g = torch.Generator(device=dev)
g.manual_seed(0)
pv = torch.rand((B, 10, H, W), generator=g, device=dev)
pv[:, 9] = (pv[:, 9] > 0.3).float()


def timed(name, fn):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(a.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return f"{name} {e0.elapsed_time(e1) / a.iters * 1e3:.1f}us"


cols, cp1s, wts, bss = [], [], [], []
for C, h, w in [(96, 120, 160), (192, 60, 80), (384, 30, 40), (768, 15, 20)]:
    cols.append(torch.randn((B, C, h, w), generator=g, device=dev).bfloat16())
    cp1s.append(torch.randn((B, C, h, w), generator=g, device=dev).bfloat16())
    wts.append(torch.randn((C, 3, 1, 1), generator=g, device=dev))
    bss.append(torch.randn((C,), generator=g, device=dev))
res = []
for k in range(4):
    res.append(timed(f"fwd{k}", lambda: ops.dggm_fuse_fwd(cp1s[k], cols[k], pv, wts[k], bss[k])))
    res.append(timed(f"bwd{k}", lambda: ops.dggm_fuse_bwd(cols[k], pv, wts[k], bss[k])))
print("per scale: " + "  ".join(res))
cp1_hot = [cp1s[0]] + [ops.nchw_to_nhwc(c) for c in cp1s[1:]]  # the DSAM cascade's outputs are NHWC
res = [timed("fwd012", lambda: ops.dggm_fuse_fwd_multi(cp1_hot[0:3], cols[0:3], pv, wts[0:3], bss[0:3], cp1_nhwc=(1, 2))),
       timed("fwd3", lambda: ops.dggm_fuse_fwd_multi(cp1_hot[3:], cols[3:], pv, wts[3:], bss[3:], cp1_nhwc=(0,))),
       timed("bwd0123", lambda: ops.dggm_fuse_bwd_multi(cols, pv, wts, bss))]
print("hot path: " + "  ".join(res))
