"""Micro benchmark of the clipped optimizer step (csrc/adamw.hip) on two
parameter lists: the hot path's (DSAM0-2 + DGGM, 17.4 M fp32) and the whole drop-in model's
(CustomMask2FormerForUniversalSegmentation v0.4.0, Swin-T, 48 labels: 37.3 M).  Arms, all on the
same parameters and gradients, alternated round by round:
  unclipped     HipAdamW.step()                                          (28 B per parameter)
  torch_clip    torch.nn.utils.clip_grad_norm_(1.0) + HipAdamW.step()    (the only way to clip before)
  fused_clip    HipAdamW(max_grad_norm=1.0).step()                       (32 B per parameter + finalise)
  hip_clip_fn   rgbd_amd.optim.clip_grad_norm_(1.0) + HipAdamW.step()    (the Trainer-hook form)
Each arm is timed eagerly (device events around --steps steps: launch enqueue included) and as a
captured graph replay (device time only).  The gradients are static buffers refilled before each
window with norm sqrt(n) >> 1: fused_clip clips every step, the in-place arms clip the first step
of a window and find norm 1 afterwards (the same launches either way).  One JSON line per
list: median over --rounds of us per step, and what fused_clip adds to unclipped against the
floor of 4 B per parameter at the unclipped arm's own HBM rate."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

import _rgbd_import  # noqa: E402,F401
from rgbd_amd.optim import HF_TRAINER_ADAMW, HipAdamW, clip_grad_norm_  # noqa: E402


def hot_path_params(dev):
    from rgbd_amd.modules import DSAModule, DepthGradientInjectionResidual
    mods = [DSAModule(ci, co).to(dev) for ci, co in [(96, 192), (192, 384), (384, 768)]]
    dg = DepthGradientInjectionResidual([96, 192, 384, 768], 3).to(dev)
    return [p for m in mods + [dg] for p in m.parameters()]


def whole_model_params(dev):
    """The parameters that receive a gradient in a training step (37.3 M of the model's 66.5 M: the
    colour backbone is detached, the ratio predictor takes none), found by one small step set up
    as tools/bench_full_model.py's."""
    import numpy as np
    from rgbd_amd import init as winit, ops, synthetic
    from rgbd_amd.config import standard_config
    from rgbd_amd.custom_model import CustomMask2FormerForUniversalSegmentation
    B, H, W = 2, 240, 320
    scenes = [synthetic.make_scene(synthetic.scene_seed(4, i), H, W) for i in range(B)]
    depth = torch.from_numpy(np.stack([s["depth_u8"] for s in scenes])).to(dev)
    rgb = torch.from_numpy(np.stack([s["rgb_u8"] for s in scenes])).contiguous().to(dev)
    mask_labels = [torch.from_numpy(s["masks"].astype(np.float32)).to(dev) for s in scenes]
    class_labels = [torch.from_numpy(s["classes"]).to(dev) for s in scenes]
    torch.manual_seed(0)
    m = CustomMask2FormerForUniversalSegmentation(standard_config(48), version="0.4.0")
    winit.init_deterministic(m)
    m.set_compute_dtype(torch.bfloat16).to(dev).train()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = m(pixel_values=ops.assemble_pixel_values(depth, rgb), mask_labels=mask_labels, class_labels=class_labels)
    out.loss.backward()
    ps = [p for p in m.parameters() if p.grad is not None]
    for p in m.parameters():
        p.grad = None
    return ps


def make_arms(ps):
    plain = HipAdamW(ps, **HF_TRAINER_ADAMW)
    fused = HipAdamW(ps, **HF_TRAINER_ADAMW, max_grad_norm=1.0)

    def torch_clip():
        torch.nn.utils.clip_grad_norm_(ps, 1.0)
        plain.step()

    def hip_clip_fn():
        clip_grad_norm_(ps, 1.0)
        plain.step()
    return {"unclipped": plain.step, "torch_clip": torch_clip, "fused_clip": fused.step, "hip_clip_fn": hip_clip_fn}


def time_us(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lists", default="hot_path,whole_model")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("micro_grad_clip: needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda")
    for name in args.lists.split(","):
        ps = {"hot_path": hot_path_params, "whole_model": whole_model_params}[name](dev)
        n = sum(p.numel() for p in ps)
        arms = make_arms(ps)

        for p in ps:
            p.grad = torch.empty_like(p)  # static: the captured graphs hold these addresses

        def fresh_grads():  # norm ~ sqrt(n) >> 1 again (the clipping arms shrink p.grad in place)
            for p in ps:
                p.grad.normal_()
        fresh_grads()
        graphs = {}
        for arm, fn in arms.items():
            for _ in range(3):  # state, workspaces, code objects
                fn()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(s):
                fn()  # this stream's workspace, outside the capture
                with torch.cuda.graph(g, stream=s):
                    fn()
            torch.cuda.current_stream().wait_stream(s)
            graphs[arm] = g
        eager = {a: [] for a in arms}
        replay = {a: [] for a in arms}
        for _ in range(args.rounds):
            for arm, fn in arms.items():  # alternate the arms within a round
                fresh_grads()
                eager[arm].append(time_us(fn, args.steps))
                fresh_grads()
                replay[arm].append(time_us(graphs[arm].replay, args.steps))
        res = {"list": name, "tensors": len(ps), "params": n, "steps": args.steps, "rounds": args.rounds}
        for arm in arms:
            res[arm] = {"eager_us": round(statistics.median(eager[arm]), 1),
                        "eager_us_min_max": [round(min(eager[arm]), 1), round(max(eager[arm]), 1)],
                        "graph_us": round(statistics.median(replay[arm]), 1),
                        "graph_us_min_max": [round(min(replay[arm]), 1), round(max(replay[arm]), 1)]}
        base, fused = res["unclipped"]["graph_us"], res["fused_clip"]["graph_us"]
        res["unclipped_graph_TBs"] = round(28 * n / base / 1e6, 2)
        res["fused_adds_graph_us"] = round(fused - base, 1)
        res["floor_4B_per_param_us"] = round(base * 4 / 28, 1)  # at the unclipped arm's own rate
        res["fused_vs_torch_clip"] = {k: round(res["fused_clip"][k] / res["torch_clip"][k], 3)
                                      for k in ("eager_us", "graph_us")}
        print(json.dumps(res), flush=True)
        del arms, graphs, ps
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
