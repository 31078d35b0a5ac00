"""f4b timing: semantic and panoptic post-processing, B = 8 images of Q = 100 queries, C = 48
classes, 160x160 mask logits to 640x640 (tools/micro_postprocess.py times the instance path).

Three arms, each in a fresh process (no arm inherits another's allocator pool or warm caches):
  hf_gpu       the HF methods fed GPU tensors (ATen kernels plus HF's host loop): the fastest path
               without the kernels, the baseline
  device       rgbd_amd.postprocess with keep_on_device=True
  device_host  the same including the copy of the maps to the host (the default)
Per arm and method: HIP-event time per batch (median and spread over --iters calls after
--warmup), and the peak torch.cuda.max_memory_allocated above the inputs.  One JSON line each.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import types

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ("hf_gpu", "device", "device_host")


def _inputs(B, Q, C, h, w):
    import numpy as np
    import torch
    rng = np.random.default_rng(0)
    cl = rng.standard_normal((B, Q, C + 1)).astype(np.float32)
    cl[:, :, C] += 6.0                       # most queries say no-object, as a trained model's do
    for q in range(0, Q, 4):                 # every fourth one is an object
        cl[:, q, q % C] += 12.0
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    ml = np.empty((B, Q, h, w), np.float32)
    for q in range(Q):
        cy, cx, sg = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.05, 0.2) * h
        ml[:, q] = 14 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sg * sg)) - 6
    ml += 0.3 * rng.standard_normal(ml.shape).astype(np.float32)
    return torch.from_numpy(cl).cuda(), torch.from_numpy(ml).cuda()


def _arm(a):
    sys.path[:0] = [_R]
    import torch
    import _rgbd_import  # noqa: F401
    from rgbd_amd import postprocess as pp
    from transformers.models.mask2former.image_processing_pil_mask2former import Mask2FormerImageProcessorPil
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    cl, ml = _inputs(a.batch, 100, 48, a.size, a.size)
    outs = types.SimpleNamespace(class_queries_logits=cl, masks_queries_logits=ml)
    ts = [(a.target, a.target)] * a.batch
    proc = Mask2FormerImageProcessorPil()
    keep = a.arm == "device"
    calls = {
        "semantic": (lambda: proc.post_process_semantic_segmentation(outs, target_sizes=ts)) if a.arm == "hf_gpu" else
                    (lambda: pp.post_process_semantic_segmentation(outs, target_sizes=ts, keep_on_device=keep)),
        "panoptic": (lambda: proc.post_process_panoptic_segmentation(outs, label_ids_to_fuse={0, 4}, target_sizes=ts))
                    if a.arm == "hf_gpu" else
                    (lambda: pp.post_process_panoptic_segmentation(outs, label_ids_to_fuse={0, 4}, target_sizes=ts,
                                                                   keep_on_device=keep)),
    }
    for task, call in calls.items():
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()  # before the warm-up: the workspace a first call keeps counts
        torch.cuda.reset_peak_memory_stats()
        for _ in range(a.warmup):
            res = call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        n_seg = sum(len(r["segments_info"]) for r in res) if task == "panoptic" else None
        print(json.dumps({"arm": a.arm, "task": task, "batch": a.batch, "logits": a.size, "target": a.target,
                          "ms_per_batch_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3),
                          "ms_max": round(max(ms), 3), "iters": a.iters, "warmup": a.warmup,
                          "peak_mem_above_inputs_MB": round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1),
                          "segments": n_seg}), flush=True)
        del res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arm", choices=ARMS, help="run one arm in this process (default: all, one child process each)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=160, help="mask-logit height and width")
    ap.add_argument("--target", type=int, default=640, help="target height and width")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per arm")
    a = ap.parse_args()
    if a.arm:
        return _arm(a)
    for arm in ARMS:
        cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm] + [
            f"--{k}={getattr(a, k)}" for k in ("batch", "size", "target", "iters", "warmup")]
        rc = subprocess.run(cmd, timeout=a.timeout).returncode
        if rc != 0:  # nothing more is started on the GPU after a failed arm
            raise SystemExit(f"arm {arm} ended with status {rc}")


if __name__ == "__main__":
    main()
