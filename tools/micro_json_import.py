"""Per-call time of the JSON import (csrc/rle_decode.hip, rgbd_amd/json_results.py): files of 100
masks at 480x640, B = 1 and B = 8.

  load      json_results.load_json_predictions on parsed dicts, whole call — host packing, the one
            upload, the launch set, the one host read — between two HIP events (the call ends in a
            device-to-host copy, so the events bracket finished work); bursts of calls, median, min
  kernels   the launch set of rgbd_rle_paint alone on the packed input (no host work, no copies),
            bursts between two HIP events, launch gaps included
  checker   tests/checkers/json_import_ref.load_prediction on the same files, host clock, once per
            file — the NumPy statement of the reference's loader (pycocotools is absent)

Masks: ellipses of random centre and radius with a ragged edge (a run per column they cross,
some hundred counts each), ten per cent of them at half size (the resize path).  Every map is
checked equal to the checker's before anything is timed.  One JSON line per result; --out also
writes them to a file.
"""
import argparse
import json
import os
import statistics
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, N_MASKS = 480, 640, 100


def _emit(rec, fh):
    line = json.dumps(rec)
    print(line, flush=True)
    if fh:
        fh.write(line + "\n")
        fh.flush()


def _file(np, torch, export, rng, resized_share):
    masks = []
    for i in range(N_MASKS):
        h, w = (H // 2, W // 2) if i > 0 and rng.rand() < resized_share else (H, W)
        y, x = np.mgrid[:h, :w]
        cy, cx = rng.randint(0, h), rng.randint(0, w)
        ry, rx = rng.randint(h // 20, h // 4), rng.randint(w // 20, w // 4)
        d = ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2
        masks.append((d < 1.0 + 0.15 * rng.rand(h, w)))
    out = []
    for m in masks:  # sizes differ: encode one at a time
        out.append(export.encode_masks(torch.from_numpy(m[None]).cuda())[0][0])
    return {"labels": [int(v) for v in rng.randint(0, 40, N_MASKS)],
            "scores": [float(v) for v in rng.rand(N_MASKS).round(4)], "masks": out}


def _burst(torch, fn, iters, bursts=5):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(bursts):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kernel-iters", type=int, default=200)
    args = ap.parse_args()
    sys.path[:0] = [_R, os.path.join(_R, "tests")]
    import numpy as np
    import torch
    import _rgbd_import  # noqa: F401
    from checkers import json_import_ref as jr
    from rgbd_amd import export, json_results as js
    if not torch.cuda.is_available():
        raise SystemExit("micro_json_import: no GPU; nothing is measured without one")
    fh = open(args.out, "w") if args.out else None
    rng = np.random.RandomState(20)
    files = [_file(np, torch, export, rng, 0.1) for _ in range(8)]
    chars = [sum(len(m["counts"]) for m in f["masks"]) for f in files]
    t_host = []
    want = []
    for f in files:
        t0 = time.perf_counter()
        want.append(jr.load_prediction(f, (H, W)))
        t_host.append(time.perf_counter() - t0)
    got = js.load_json_predictions(files, (H, W))
    for g, w in zip(got, want):
        assert np.array_equal(g["segmentation"].cpu().numpy(), w[0]) and [s["id"] for s in g["segments_info"]] == w[1]
    _emit(dict(what="checker", masks=N_MASKS, H=H, W=W, files=len(files), chars_per_file=chars,
               host_ms_per_file=[round(t * 1e3, 1) for t in t_host],
               host_ms_median=round(statistics.median(t_host) * 1e3, 1)), fh)
    for B in (1, 8):
        sub = files[:B]
        med, mn = _burst(torch, lambda: js.load_json_predictions(sub, (H, W)), args.iters)
        _emit(dict(what="load", B=B, masks_per_file=N_MASKS, ms_median=round(med, 4), ms_min=round(mn, 4),
                   calls_per_burst=args.iters), fh)
        fields = [js._file_masks(f, "file", (H, W)) for f in sub]
        pk = js._Packed(fields, H, W, torch.device("cuda", 0))
        med, mn = _burst(torch, pk.paint, args.kernel_iters)
        _emit(dict(what="kernels", B=B, masks=pk.N, resized=pk.n_resized, chars=pk.n_chars,
                   us_median=round(med * 1e3, 2), us_min=round(mn * 1e3, 2), calls_per_burst=args.kernel_iters), fh)


if __name__ == "__main__":
    main()
