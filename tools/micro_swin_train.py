"""The Swin-T backbone's forward + backward at BASELINE's 640x480, B = 8, in float32 and under
bf16 autocast: the HIP layers with the window-attention backward (rgbd_amd/swin.py with gradients)
against the Hugging Face path on the same weights (``swin.uninstall``: pad, roll, window
partition, eager attention — what the layers ran under gradients before the backward kernel
existed; the nn.Linear / LayerNorm / patch-embedding classes of dense.install stay in both arms).
Both arms in one process, alternating round by round; device time by HIP events after a warm-up
of every (arm, precision); per arm the median and the spread (min .. max) of the rounds, and the
HF / HIP ratio.  Also the window-attention backward kernel alone at the four stage shapes.
Writes profiles/swin_backward/micro_swin_train.json (and prints it); --out DIR to redirect.
--trace runs the HIP bf16 arm alone (for a kernel trace taken in a run of its own)."""
import argparse
import copy
import json
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R]
import torch  # noqa: E402

import _rgbd_import  # noqa: E402,F401
from rgbd_amd import dense, swin  # noqa: E402
from rgbd_amd.config import standard_config  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--hw", type=int, nargs=2, default=(480, 640))
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=os.path.join(_R, "profiles", "swin_backward"))
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()

dev = torch.device("cuda")
from transformers import SwinBackbone  # noqa: E402
torch.manual_seed(3)
hf = SwinBackbone(standard_config(48).backbone_config).to(dev).eval()
with torch.no_grad():
    for m in hf.modules():
        if hasattr(m, "relative_position_bias_table"):
            m.relative_position_bias_table.normal_(0, 0.5)
hip = copy.deepcopy(hf)
dense.install(hf)
dense.install(hip)
assert swin.install(hip) == 12
x = torch.randn((args.batch, 3, *args.hw), device=dev)
arms = {"hip": hip, "hf": hf}


def step(m, amp):
    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        feats = m(x).feature_maps
    sum(f.float().square().mean() for f in feats).backward()


def timed(m, amp):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        step(m, amp)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.reps


if args.trace:
    for _ in range(3):
        step(hip, True)
    torch.cuda.synchronize()
    sys.exit(0)

res = {"batch": args.batch, "hw": list(args.hw), "rounds": args.rounds, "reps": args.reps}
for amp, tag in ((False, "float32"), (True, "bf16_autocast")):
    for m in arms.values():  # warm-up of every shape: allocator, workspaces, weight casts
        step(m, amp)
        step(m, amp)
    torch.cuda.synchronize()
    ts = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, m in arms.items():
            ts[k].append(timed(m, amp))
    r = {}
    for k, v in ts.items():
        v = sorted(v)
        r[k + "_ms"] = {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}
        print(f"{tag:>14} {k:>4}: median {v[len(v) // 2]:8.2f} ms  (min {v[0]:8.2f}, max {v[-1]:8.2f})")
    r["hf_over_hip"] = round(r["hf_ms"]["median"] / r["hip_ms"]["median"], 3)
    print(f"{tag:>14} HF / HIP = {r['hf_over_hip']:.3f}")
    res[tag] = r

# the backward kernel alone (with its reduction kernel) at the four stage shapes, bf16 and float32
kern = {}
for dt, tag in ((torch.bfloat16, "bf16"), (torch.float32, "f32")):
    for (H, W, heads) in ((120, 160, 3), (60, 80, 6), (30, 40, 12), (15, 20, 24)):
        C = 32 * heads
        rows = args.batch * H * W
        qkv = torch.randn((rows, 3 * C), device=dev).to(dt)
        b = torch.randn((3 * C,), device=dev)
        table = torch.randn((169, heads), device=dev)
        g = torch.randn((rows, C), device=dev).to(dt)
        v = []
        for fn in (lambda: swin.window_attention(qkv, b, table, args.batch, H, W, heads, 3, 32 ** -0.5),
                   lambda: swin.window_attention_bwd(qkv, b, table, g, args.batch, H, W, heads, 3, 32 ** -0.5)):
            for _ in range(3):
                fn()
            t = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(5):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                t.append(e0.elapsed_time(e1) / 5 * 1e3)
            v.append(round(sorted(t)[2], 1))
        kern[f"{tag}_{H}x{W}x{heads}"] = {"fwd_us": v[0], "bwd_us": v[1]}
        print(f"window attention {tag} {H}x{W} heads {heads}: forward {v[0]:8.1f} us, backward {v[1]:8.1f} us")
res["kernel"] = kern
os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, "micro_swin_train.json"), "w") as f:
    json.dump({"micro_swin_train": res}, f, indent=1)
    f.write("\n")
print(json.dumps({"micro_swin_train": res}))
