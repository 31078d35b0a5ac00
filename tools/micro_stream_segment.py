"""C5 end to end: frames per second of stream.StreamingSegmenter (one graph replay per frame)
against the eager path the package offered before it, in ONE process, the two arms alternated
round by round (the host is shared: a difference is trusted only against the spread of the rounds).

  replay  seg(depth, rgb) -> res.segments(): the host waits for the frame's event and reads the
          pinned tables; map and overlay stay on the device
  replay_track  the same with track=dict(iou_threshold=0.5): contingency against the previous
          frame, greedy match, track assignment and the two state copies inside the graph
          (DESIGN §5.19); its cost per call is reported as the difference of the medians
  eager   data.map_10channel -> model -> postprocess.post_process_instance_segmentation (maps copied
          to the host, its default) -> the reference's overlay loop on the host in numpy

Both take device-resident u8 frames (the camera upload is the same for both and is left out) and end
with the host holding the segments of every frame, so each frame's time includes its synchronise.
Model: the drop-in v0.4.0 model with formula weights, 48 labels, bf16 (the streaming default).

Then rgbd_overlay_blend alone at 1280x720: HIP-event time over a burst of back-to-back launches,
bytes = 10 B per pixel (3 read + 4 read + 3 written), beside the 6.3 TB/s the project takes as
achievable.  B = 1 moves 9.2 MB: a launch-bound size, reported as such.

One JSON line per result; --out also writes them to a file.
"""
import argparse
import json
import os
import statistics
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"640x480_b1": (480, 640, 1, None), "640x480_b8": (480, 640, 8, None),  # name: (H, W, B, model size)
          "c5_1280x720_to_640": (720, 1280, 1, (640, 640))}
ACHIEVABLE_GBS = 6300.0


def _host_overlay(image, result, palette, num_colors, alpha=0.6):
    """predictor.py:1286-1320 with the colour taken from the palette by label (host, numpy)."""
    import numpy as np
    seg = result["segmentation"].numpy()
    over = image.astype(np.float32)
    for s in result["segments_info"]:
        m = seg == s["id"]
        color = palette[s["label_id"] % num_colors]
        for c in range(3):
            over[m, c] = (1 - alpha) * over[m, c] + alpha * color[c]
    return np.clip(over, 0, 255).astype(np.uint8)


def _emit(rec, fh):
    line = json.dumps(rec)
    print(line, flush=True)
    if fh:
        fh.write(line + "\n")
        fh.flush()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=",".join(SHAPES), help="comma-separated subset of " + ", ".join(SHAPES))
    ap.add_argument("--rounds", type=int, default=3, help="alternated rounds per arm")
    ap.add_argument("--frames", type=int, default=8, help="frames per round")
    ap.add_argument("--threshold", type=float, default=0.0, help="0.0 keeps segments with formula weights")
    ap.add_argument("--blend-iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path[:0] = [_R]
    import numpy as np
    import torch
    import _rgbd_import  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    from rgbd_amd import data, init as winit, overlay, postprocess as pp, synthetic
    from rgbd_amd.config import standard_config
    from rgbd_amd.custom_model import CustomMask2FormerForUniversalSegmentation
    from rgbd_amd.stream import StreamingSegmenter
    fh = open(a.out, "w") if a.out else None
    dev = torch.device("cuda", 0)
    _emit({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip}, fh)
    torch.manual_seed(0)
    model = CustomMask2FormerForUniversalSegmentation(standard_config(48), version="0.4.0")
    winit.init_deterministic(model)
    model = model.to(dev).eval()
    palette = overlay.consistent_colors(48)

    for name in a.shapes.split(","):
        H, W, B, size = SHAPES[name]
        scenes = [synthetic.make_scene(synthetic.scene_seed(5, i), H, W) for i in range(B + 2)]
        batches = []
        for k in range(3):  # three different batches, cycled
            pick = [scenes[(k + i) % len(scenes)] for i in range(B)]
            batches.append((torch.from_numpy(np.stack([s["depth_u8"] for s in pick])).to(dev),
                            torch.from_numpy(np.stack([s["rgb_u8"] for s in pick])).contiguous().to(dev)))
        seg = StreamingSegmenter(model, H, W, B=B, size=size, threshold=a.threshold, dtype=torch.bfloat16,
                                 overlay=dict(alpha=0.6, palette=palette, color_by="label")).capture()

        seg_t = StreamingSegmenter(model, H, W, B=B, size=size, threshold=a.threshold, dtype=torch.bfloat16,
                                   overlay=dict(alpha=0.6, palette=palette, color_by="label"),
                                   track=dict(iou_threshold=0.5)).capture()

        host_s = [0.0]

        def replay(depth, rgb):
            return seg(depth, rgb).segments()

        def replay_track(depth, rgb):
            return seg_t(depth, rgb).segments()

        def eager(depth, rgb):
            model.set_compute_dtype(torch.bfloat16)
            with torch.no_grad():
                pv = data.map_10channel(rgb, depth, size=size)["pixel_values"]
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    out = model(pixel_values=pv)
                res = pp.post_process_instance_segmentation(out, threshold=a.threshold, target_sizes=[(H, W)] * B)
            t0 = time.perf_counter()  # the maps are on the host by now: what follows is host time only
            frames = rgb.cpu().numpy()
            over = [_host_overlay(frames[i], res[i], palette, 48) for i in range(B)]
            host_s[0] += time.perf_counter() - t0
            return res, over

        kept = [len(r["segments_info"]) for r in replay(*batches[0])]
        for fn in (replay, replay_track, eager):  # warm every arm on every batch
            for bt in batches:
                fn(*bt)
        fps = {"replay": [], "replay_track": [], "eager": []}
        host_s[0], t_eager = 0.0, 0.0
        for _ in range(a.rounds):
            for arm, fn in (("replay", replay), ("replay_track", replay_track), ("eager", eager)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(a.frames):
                    fn(*batches[i % 3])
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                t_eager += dt if arm == "eager" else 0.0
                fps[arm].append(B * a.frames / dt)
        rec = {"what": "segmenter frames/s, end to end", "shape": name, "H": H, "W": W, "B": B, "size": size,
               "dtype": "bf16", "graph_branches": seg.width, "segments_kept_first_batch": kept,
               "rounds": a.rounds, "frames_per_round": a.frames}
        for arm, v in fps.items():
            rec[arm] = {"fps_median": round(statistics.median(v), 2), "fps_min": round(min(v), 2),
                        "fps_max": round(max(v), 2)}
        rec["eager_host_overlay_share_of_time"] = round(host_s[0] / t_eager, 3)
        rec["replay_over_eager_median"] = round(rec["replay"]["fps_median"] / rec["eager"]["fps_median"], 3)
        rec["track_ms_per_call_median"] = round(
            1e3 * B * (1 / rec["replay_track"]["fps_median"] - 1 / rec["replay"]["fps_median"]), 3)
        _emit(rec, fh)
        del seg, seg_t
        torch.cuda.empty_cache()

    H, W = 720, 1280
    for B in (1, 8):
        g = torch.Generator(device="cpu").manual_seed(B)
        rgb = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
        ids = torch.randint(-1, 100, (B, H // 16, W // 16), generator=g).float()  # 16 x 16 blocks, -1 = none
        segm = ids.repeat_interleave(16, 1).repeat_interleave(16, 2).contiguous().to(dev)
        lut = torch.randint(0, 1 << 24, (B, 100), dtype=torch.int32, generator=g).to(dev)
        out = torch.empty_like(rgb)
        for _ in range(10):
            overlay.blend(rgb, segm, lut, 0.6, out=out)
        torch.cuda.synchronize()
        ms = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.blend_iters):
                overlay.blend(rgb, segm, lut, 0.6, out=out)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / a.blend_iters)
        nbytes = 10 * B * H * W
        med = statistics.median(ms)
        _emit({"what": "rgbd_overlay_blend alone (burst of back-to-back launches, HIP events; includes the launch gaps)",
               "shape": f"{W}x{H}", "B": B, "MB": round(nbytes / 1e6, 2), "us_per_call_median": round(med * 1e3, 2),
               "us_per_call_min": round(min(ms) * 1e3, 2), "GBs_median": round(nbytes / med / 1e6, 1),
               "GBs_best": round(nbytes / min(ms) / 1e6, 1), "achievable_GBs": ACHIEVABLE_GBS,
               "share_of_achievable_median": round(nbytes / med / 1e6 / ACHIEVABLE_GBS, 3),
               "note": "launch-bound size: 9.2 MB per call" if B == 1 else "73.7 MB per call"}, fh)
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
