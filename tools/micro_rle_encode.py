"""Per-call time of the JSON export, the device encoder (csrc/rle_encode.hip, rgbd_amd/export.py)
against the torch path it can replace: maps of 100 segments at 480x640, B = 1 and B = 8, built by
loading the files of tools/micro_json_import.py.

  per_image  export.prediction_to_json per image, whole call — uploads, launches, host reads, host
             string assembly — with export.HIP_RLE_ENCODE on against off (off is the parent
             commit's path: the [N, h, w] stack, nonzero, _to_string)
  batched    export.encode_segments_batch over the B maps against export.encode_masks per image
  kernels    the launch set of rgbd_rle_encode_labels alone on preallocated buffers (no host work,
             no copies), bursts between two HIP events, launch gaps included
  stream     (--stream) StreamingSegmenter replay + segments(), with and without encode=True, at
             240x320 and 480x640 (formula weights, one synthetic scene)

The two arms of a pair are interleaved burst by burst in one process; a burst is timed by two HIP
events (every call ends in a device-to-host copy, so they bracket finished work) and by the host
clock; reported: the median of the bursts and their spread (max - min over the bursts).  Every
result is checked equal between the arms before anything is timed.  One JSON line per result;
--out also writes them to a file.
"""
import argparse
import json
import logging
import os
import statistics
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "tests"), os.path.dirname(os.path.abspath(__file__))]
H, W, N_MASKS = 480, 640, 100


def _emit(rec, fh):
    line = json.dumps(rec)
    print(line, flush=True)
    if fh:
        fh.write(line + "\n")
        fh.flush()


def _pair(torch, arms, iters, bursts=5):
    """arms: name -> callable.  Bursts of ``iters`` calls, the arms taking turns -> name -> stats."""
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in arms}
    wall = {k: [] for k in arms}
    for _ in range(bursts):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3 / iters)
            ev[name].append(e0.elapsed_time(e1) / iters)
    return {k: dict(ms_median=round(statistics.median(ev[k]), 4), ms_min=round(min(ev[k]), 4),
                    ms_spread=round(max(ev[k]) - min(ev[k]), 4), wall_ms_median=round(statistics.median(wall[k]), 4),
                    wall_ms_spread=round(max(wall[k]) - min(wall[k]), 4)) for k in arms}


def _stream(torch, fh, iters):
    from rgbd_amd import init as winit, synthetic
    from rgbd_amd.config import standard_config
    from rgbd_amd.custom_model import CustomMask2FormerForUniversalSegmentation
    from rgbd_amd.stream import StreamingSegmenter
    logging.getLogger("rgbd_amd.export").setLevel(logging.ERROR)  # "empty mask: skipped" once per call and segment
    torch.manual_seed(0)
    model = CustomMask2FormerForUniversalSegmentation(standard_config(48), version="0.4.0")
    winit.init_deterministic(model)
    model = model.to("cuda").eval()
    for h, w in ((240, 320), (480, 640)):
        sc = synthetic.make_scene(synthetic.scene_seed(5, 0), h, w)
        depth = torch.from_numpy(sc["depth_u8"]).cuda()[None]
        rgb = torch.from_numpy(sc["rgb_u8"]).contiguous().cuda()[None]
        segs = {k: StreamingSegmenter(model, h, w, B=1, threshold=0.0, dtype=torch.bfloat16, encode=(k == "encode"))
                for k in ("plain", "encode")}
        for s in segs.values():
            s(depth, rgb).segments()
        kept = len(segs["encode"](depth, rgb).to_json()[0]["masks"])
        arms = {k: (lambda s=s: s(depth, rgb).segments()) for k, s in segs.items()}
        arms["encode+to_json"] = lambda s=segs["encode"]: s(depth, rgb).to_json()
        for k, st in _pair(torch, arms, iters).items():
            _emit(dict(what="stream", arm=k, H=h, W=w, B=1, masks_written=kept, calls_per_burst=iters, **st), fh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--kernel-iters", type=int, default=100)
    ap.add_argument("--stream", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import _rgbd_import  # noqa: F401
    import micro_json_import as mji
    from checkers import rle_encode_cases as rc
    from rgbd_amd import export, json_results as js
    if not torch.cuda.is_available():
        raise SystemExit("micro_rle_encode: no GPU; nothing is measured without one")
    fh = open(args.out, "w") if args.out else None
    rng = np.random.RandomState(20)
    export.HIP_RLE_ENCODE = False
    files = [mji._file(np, torch, export, rng, 0.1) for _ in range(8)]
    preds = js.load_json_predictions(files, (H, W))
    assert all(p is not None for p in preds)

    def per_image(on, sub):
        export.HIP_RLE_ENCODE = on
        return [export.prediction_to_json(p) for p in sub]

    def torch_batch(sub):
        out = []
        for p in sub:
            seg = p["segmentation"]
            ids = torch.tensor([s["id"] for s in p["segments_info"]], dtype=seg.dtype, device=seg.device)
            out.append(export.encode_masks(seg[None] == ids[:, None, None]))
        return out

    for B in (1, 8):
        sub = preds[:B]
        maps = torch.stack([p["segmentation"] for p in sub])
        ids = [[s["id"] for s in p["segments_info"]] for p in sub]
        on, off = per_image(True, sub), per_image(False, sub)
        assert json.dumps(on) == json.dumps(off)
        dev_b, torch_b = export.encode_segments_batch(maps, ids), torch_batch(sub)
        assert [[e[:2] for e in img] for img in dev_b] == [[tuple(e) for e in img] for img in torch_b]
        n_masks = sum(len(i) for i in ids)
        n_chars = sum(len(e[0]["counts"]) for img in dev_b for e in img)
        st = _pair(torch, {"hip": lambda: per_image(True, sub), "torch": lambda: per_image(False, sub)}, args.iters)
        for k, v in st.items():
            _emit(dict(what="per_image", arm=k, B=B, masks=n_masks, chars=n_chars, calls_per_burst=args.iters, **v), fh)
        st = _pair(torch, {"hip": lambda: export.encode_segments_batch(maps, ids), "torch": lambda: torch_batch(sub)},
                   args.iters)
        for k, v in st.items():
            _emit(dict(what="batched", arm=k, B=B, masks=n_masks, chars=n_chars, calls_per_burst=args.iters, **v), fh)
        Q = max(len(i) for i in ids)
        table = np.full((B, Q), -1, np.int32)
        for b, row in enumerate(ids):
            table[b, :len(row)] = row
        t = torch.from_numpy(table).cuda()
        cap = rc.capacity(0, B, B * Q, H, W)
        bufs = rc.raw_encode(0, maps, t, B, B * Q, H, W, *cap)
        from rgbd_amd import _lib
        from rgbd_amd.ops import _p, _stream as _st
        L, dev = _lib.lib(), maps.device

        def launch():
            L.rgbd_rle_encode_labels(_lib.RGBD_I32, _p(maps), B, H, W, 256, _p(t), Q, cap[0], cap[1], _p(bufs["chars"]),
                                     _p(bufs["offsets"]), _p(bufs["info"]), _p(bufs["totals"]), _p(bufs["ws"]),
                                     _st(dev))
        st = _pair(torch, {"kernels": launch}, args.kernel_iters)["kernels"]
        _emit(dict(what="kernels", B=B, masks=B * Q, counts=int(bufs["totals"][0]), chars=int(bufs["totals"][1]),
                   us_median=round(st["ms_median"] * 1e3, 2), us_min=round(st["ms_min"] * 1e3, 2),
                   us_spread=round(st["ms_spread"] * 1e3, 2), calls_per_burst=args.kernel_iters), fh)
    if args.stream:
        _stream(torch, fh, args.iters)


if __name__ == "__main__":
    main()
