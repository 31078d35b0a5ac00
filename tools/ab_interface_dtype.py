"""A/B of the hot path's interface dtype on the bench's captured headline step (B = 8, 640x480,
compute dtype bf16): the plain bf16 mode (bf16 colour maps in, bf16 features out, bf16 upstream
gradients) against the float32-interface mode (float32 colour maps, features and upstream
gradients of the same values' shapes).  One process, one captured graph per
mode, replayed in alternating rounds; prints the median ms per step per mode and the difference.

    python tools/ab_interface_dtype.py [--rounds 8] [--steps 20] [--height 480 --width 640 --batch 8]

bench.make_parts builds the step around rgbd_amd.hot_path.prepare / hot_path, which it looks up
when it is called; for the new mode they are wrapped here to pass interface_dtype=torch.float32
(bench.py itself is not touched)."""
import argparse
import functools
import json
import os
import statistics
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "tests/golden")]
import torch  # noqa: E402

import bench  # noqa: E402
from rgbd_amd import hot_path as hp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--width", type=int, default=640)
ap.add_argument("--batch", type=int, default=8)
a = ap.parse_args()

dev = torch.device("cuda")
args = bench.parse(["--height", str(a.height), "--width", str(a.width), "--batch", str(a.batch)])


def make(interface):
    ctx = bench.build(args, dev)
    if interface is None:
        st = bench.make_step(ctx, 1, graph=True)
    else:
        g = torch.Generator(device=dev).manual_seed(1234)
        ctx["colors"] = [torch.randn(c.shape, generator=g, device=dev) for c in ctx["colors"]]
        ctx["gouts"] = [torch.randn(c.shape, generator=g, device=dev) * 1e-2 for c in ctx["colors"]]
        prepare, hot_path = hp.prepare, hp.hot_path
        hp.prepare = functools.partial(prepare, interface_dtype=interface)
        hp.hot_path = functools.partial(hot_path, interface_dtype=interface)
        try:
            st = bench.make_step(ctx, 1, graph=True)
            for _ in range(3):
                outs = st()  # capture + warm-up with the wrapped functions
        finally:
            hp.prepare, hp.hot_path = prepare, hot_path
        assert all(o.dtype == torch.float32 for o in outs)
    for _ in range(3):
        st()
    torch.cuda.synchronize()
    return st


steps = {"bf16": make(None), "bf16+f32io": make(torch.float32)}
res = {k: [] for k in steps}
for rnd in range(a.rounds):
    for k, st in steps.items():
        res[k].append(1e3 * bench.timed(st, a.steps, 2, 1) / a.steps)
med = {k: statistics.median(v) for k, v in res.items()}
for k, v in res.items():
    print(f"{k:12s}: {med[k]:.4f} ms/step (min {min(v):.4f}, max {max(v):.4f}, {a.rounds} rounds x {a.steps} steps)")
d = med["bf16+f32io"] - med["bf16"]
print(f"float32 interface costs {1e3 * d:+.1f} us/step ({100 * d / med['bf16']:+.2f} %)")
print(json.dumps({"shape": f"{a.width}x{a.height}", "batch": a.batch, "ms_per_step": med, "rounds": res,
                  "delta_us": 1e3 * d, "delta_pct": 100 * d / med["bf16"], "device": torch.cuda.get_device_name(0)}))
