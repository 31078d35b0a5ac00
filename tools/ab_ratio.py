"""A/B of two library builds on the ratio predictor (train mode, bench shape), interleaved in one
process so both see the same device and clock state: per round, --iters forwards with each
library; per-kernel times from each library's own HIP-event timing.  Prints medians.

    python tools/ab_ratio.py rgb-d-instance-segmentation_amd/gpurun_ab_old.so --rounds 8

--bytes instead compares the builds' outputs bytewise at small shapes (see compare_bytes); the
exit status is non-zero when anything differs.
"""
import argparse
import ctypes
import os
import statistics
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "tests/golden")]
import torch  # noqa: E402

import _rgbd_import  # noqa: E402,F401
from rgbd_amd import _lib, init as winit, synthetic  # noqa: E402
from rgbd_amd.modules import EnhancedDepthImageRatioPredictor  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("others", nargs="+")
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--per-round", action="store_true", help="also print every round's per-kernel averages (noise estimate)")
ap.add_argument("--bytes", action="store_true",
                help="no timing: rgbd_ratio_forward of every build on the same packed weights, small shapes, both "
                     "dtypes, train and eval; ratio, workspace and BN running statistics compared bytewise")
a = ap.parse_args()

new = _lib.lib()
libs = {"new": new}
for other in a.others:
    h = ctypes.CDLL(os.path.join(_R, other))
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(h, name):
            fn = getattr(h, name)
            fn.restype, fn.argtypes = res, args
    libs[os.path.basename(other)] = h


def compare_bytes():
    """Every build's rgbd_ratio_forward, called directly: the same packed blob and input, and per
    build fresh clones of the BN tensors, a zeroed workspace, a fixed seed and a zero seed counter."""
    from rgbd_amd import ratio as host
    from rgbd_amd.ops import _p, _stream
    shapes = [(2, 64, 128), (2, 64, 96), (32, 32, 32), (3, 90, 125), (1, 64, 96)]
    cases = [(torch.float32, 1, 0), (torch.float32, 0, 0), (torch.bfloat16, 1, 0), (torch.bfloat16, 1, 1),
             (torch.bfloat16, 0, 0)]  # dtype, training, flags (1 = RGBD_RATIO_F_PHASE2)
    mod = EnhancedDepthImageRatioPredictor(3)
    winit.init_deterministic(mod, prefix="model.pixel_level_module.ratio_predictor.")
    mod = mod.cuda()
    dev = torch.device("cuda")
    bn0 = [t.detach().clone() for bn in host._bns(mod) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)]
    bad = 0
    print("dtype train flags shape | build: ratio ws[0:features) [features:pooled) [pooled:feat) [feat:hidden) "
          "[hidden:end) bn_running")
    for dtype, training, flags in cases:
        code = 1 if dtype == torch.bfloat16 else 0
        blob = host._packed(mod, dtype)  # packed once, by the in-tree build
        for B, H, W in shapes:
            planes, _, _ = synthetic.make_batch(3, B, H, W)
            d = torch.from_numpy(planes[:, 3:6].copy()).cuda()
            got = {}
            for tag, L in libs.items():
                n = L.rgbd_ratio_workspace_size(code, B, H, W)
                cuts = [0] + [f(code, B, H, W) for f in (L.rgbd_ratio_features_offset, L.rgbd_ratio_pooled_offset,
                                                          L.rgbd_ratio_feat_offset, L.rgbd_ratio_hidden_offset)] + [n]
                bn = [t.clone() for t in bn0]
                ws = torch.zeros(n, dtype=torch.uint8, device=dev)
                ctr = torch.zeros(1, dtype=torch.int64, device=dev)
                ratio = torch.zeros(B, dtype=torch.float32, device=dev)
                arr = (ctypes.c_void_p * len(bn))(*[t.data_ptr() for t in bn])
                host.check(L.rgbd_ratio_forward(code, training, ctypes.c_float(0.1), ctypes.c_void_p(d.data_ptr()),
                                                d.stride(0), B, H, W, _p(blob), arr, ctypes.c_ulonglong(0x1234567),
                                                _p(ctr), _p(ratio), _p(ws), flags, _stream(dev)), "rgbd_ratio_forward")
                torch.cuda.synchronize()
                parts = [ratio.view(torch.uint8)] + [ws[a0:a1] for a0, a1 in zip(cuts, cuts[1:])]
                parts.append(torch.cat([t.view(torch.uint8) for t in bn[2::4] + bn[3::4]] + [ctr.view(torch.uint8)]))
                got[tag] = (cuts, [p.cpu() for p in parts])
            for tag in libs:
                eq = [got[tag][0] == got["new"][0] and torch.equal(x, y) for x, y in zip(got[tag][1], got["new"][1])]
                bad += eq.count(False)
                print(f"{str(dtype)[6:]} {training} {flags} {B}x{H}x{W} | {tag}:", " ".join("equal" if e else "DIFFER" for e in eq))
    print("bytes: every comparison equal" if not bad else f"bytes: {bad} comparisons DIFFER")
    return bad


if a.bytes:
    sys.exit(1 if compare_bytes() else 0)

m = EnhancedDepthImageRatioPredictor(3)
winit.init_deterministic(m, prefix="model.pixel_level_module.ratio_predictor.")
m.compute_dtype = torch.bfloat16
m = m.cuda().train()
planes, _, _ = synthetic.make_batch(3, 8, 480, 640)
d = torch.from_numpy(planes[:, 3:6].copy()).cuda()
names = ["rp_conv3x3", "rp_chain"]
res = {k: {n: [] for n in names + ["total"]} for k in libs}
for rnd in range(a.rounds + 1):
    for tag, L in libs.items():
        _lib._lib = L
        for _ in range(2):
            m(d)
        torch.cuda.synchronize()
        L.rgbd_timing_enable(1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            m(d)
        e1.record()
        torch.cuda.synchronize()
        cnt = ctypes.c_int(0)
        for n in names:
            ms = L.rgbd_timing_read(n.encode(), ctypes.byref(cnt))
            if rnd:
                res[tag][n].append(ms / max(cnt.value, 1))
        L.rgbd_timing_enable(0)
        if rnd:
            res[tag]["total"].append(e0.elapsed_time(e1) / a.iters)
# same inputs, eval mode (deterministic): every build must give the in-tree build's ratio bitwise
m.eval()
outs = {}
for tag, L in libs.items():
    _lib._lib = L
    outs[tag] = m(d).cpu()
_lib._lib = new
m.train()
if a.per_round:
    for tag in libs:
        for n in names + ["total"]:
            print(tag, n, "rounds:", " ".join(f"{v:.4f}" for v in res[tag][n]))
for tag in libs:
    print(tag, "ratio==new:", bool(torch.equal(outs[tag], outs["new"])), "  ".join(f"{n} {statistics.median(v):.4f} ms (min {min(v):.4f})" for n, v in res[tag].items()))
