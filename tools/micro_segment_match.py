"""Per-call time of the segment-matching kernels (csrc/segment_match.hip) at 1280x720.

rgbd_label_contingency against two baselines on the same maps:

  bincount  the device composition torch offers: ids of both maps folded into one key,
            torch.bincount(a * (nb + 1) + b) per batch (key arithmetic included: it is part of
            that path); its table is checked equal to the kernel's before anything is timed
  host      the reference's loop (mask2former/predictor.py:95-155, :72-92): one boolean mask per
            segment, logical_and / logical_or over the full frame for every pair, in numpy on
            the host.  Timed once on image 0; for more than ``--host-pairs`` pairs a prefix of
            the prediction rows is timed and the figure scaled, and the record says so.

Two kinds of map: "segments" (a 10 x 10 grid of rectangles with jittered ids — a wave's 256
consecutive cells lie in one or two segments, as in an instance map) and "noise" (an id per
pixel: no two neighbouring lanes share a key, the worst case for the wave pre-reduction).

Timing: bursts of back-to-back calls between two HIP events (launch gaps included), five
bursts, median and minimum.  Bytes = 8 B per pixel read; the table traffic is left out.
Then rgbd_greedy_iou_match and rgbd_match_lut on the tables so made.

One JSON line per result; --out also writes them to a file.
"""
import argparse
import json
import os
import statistics
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 720, 1280
ACHIEVABLE_GBS = 6300.0


def _emit(rec, fh):
    line = json.dumps(rec)
    print(line, flush=True)
    if fh:
        fh.write(line + "\n")
        fh.flush()


def _maps(np, rng, B, n, kind):
    if kind == "noise":
        return rng.randint(-1, n, size=(B, H, W)).astype(np.float32)
    ids = rng.randint(-1, n, size=(B, 10, 10))
    m = np.repeat(np.repeat(ids, H // 10, axis=1), W // 10, axis=2)
    return np.roll(m, rng.randint(0, 40), axis=2).astype(np.float32)


def _burst(torch, fn, iters, bursts=5):
    for _ in range(10):
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


def _host_loop(np, a, b, na, nb, max_pairs):
    """The reference's P x G loop on one image -> (seconds, pairs timed, pairs in all)."""
    pm = [a == i for i in range(na)]
    gm = [b == j for j in range(nb)]
    pm, gm = [m for m in pm if m.sum() > 0], [m for m in gm if m.sum() > 0]
    rows = max(1, min(len(pm), max_pairs // max(len(gm), 1)))
    t0 = time.perf_counter()
    for p in pm[:rows]:
        for g in gm:
            inter = np.logical_and(p, g).sum()
            union = np.logical_or(p, g).sum()
            _ = inter / union if union else 0.0
    return time.perf_counter() - t0, rows * len(gm), len(pm) * len(gm)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host-pairs", type=int, default=2000, help="pairs of the host loop timed per case")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path[:0] = [_R]
    import numpy as np
    import torch
    import _rgbd_import  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    from rgbd_amd import overlay
    fh = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        fh = open(a.out, "w")
    dev = torch.device("cuda", 0)
    _emit({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
           "numpy": np.__version__}, fh)
    rng = np.random.RandomState(0)
    for kind in ("segments", "noise"):
        for na, nb in ((100, 100), (100, 256)):
            for B in (1, 8):
                ha, hb = _maps(np, rng, B, na, kind), _maps(np, rng, B, nb, kind)
                if kind == "segments":  # the second map: the first moved by 7 pixels, so that segments match
                    hb = np.roll(ha, 7, axis=2)
                da, db = torch.from_numpy(ha).to(dev), torch.from_numpy(hb).to(dev)
                T = (na + 1) * (nb + 1)
                counts = torch.empty((B, na + 1, nb + 1), dtype=torch.int32, device=dev)
                off = (torch.arange(B, device=dev) * T).view(B, 1, 1)

                def kernel():
                    overlay.label_contingency(da, db, na, nb, out=counts)

                def bincount():
                    ia = torch.where(da < 0, na, da).long()
                    ib = torch.where(db < 0, nb, db).long()
                    return torch.bincount((ia * (nb + 1) + ib + off).flatten(), minlength=B * T)

                kernel()
                same = bool(torch.equal(counts.flatten().long(), bincount()))
                k_med, k_min = _burst(torch, kernel, a.iters)
                b_med, b_min = _burst(torch, bincount, max(a.iters // 4, 10))
                nbytes = 8 * B * H * W
                rec = {"what": "rgbd_label_contingency per call (burst between HIP events; launch gaps included)",
                       "maps": kind, "shape": f"{W}x{H}", "B": B, "na": na, "nb": nb, "table_KB": round(T * 4 / 1024, 1),
                       "path": "LDS table" if T * 4 <= 163840 else "global table", "MB_read": round(nbytes / 1e6, 2),
                       "kernel_us_median": round(k_med * 1e3, 2), "kernel_us_min": round(k_min * 1e3, 2),
                       "kernel_GBs_median": round(nbytes / k_med / 1e6, 1),
                       "share_of_achievable_median": round(nbytes / k_med / 1e6 / ACHIEVABLE_GBS, 3),
                       "bincount_us_median": round(b_med * 1e3, 2), "bincount_us_min": round(b_min * 1e3, 2),
                       "bincount_over_kernel_median": round(b_med / k_med, 2), "tables_equal": same}
                if B == 1:
                    sec, timed, pairs = _host_loop(np, ha[0], hb[0], na, nb, a.host_pairs)
                    rec.update({"host_loop_s_per_image": round(sec * pairs / timed, 3), "host_pairs_timed": timed,
                                "host_pairs": pairs, "host_scaled": timed != pairs})
                _emit(rec, fh)
                if B == 8 or kind == "noise":
                    continue
                # the per-image stages on this table (Q = 100 against nb ids), B = 1
                a_list = torch.arange(na, dtype=torch.int32, device=dev).repeat(B, 1).contiguous()
                b_list = torch.arange(nb, dtype=torch.int32, device=dev).repeat(B, 1).contiguous()
                outs = overlay.greedy_iou_match(counts, a_list, b_list, H * W, 0.5)
                gt_colors = torch.randint(0, 1 << 24, (B, nb), dtype=torch.int32, device=dev)
                lut = torch.empty((B, na), dtype=torch.int32, device=dev)
                m_med, m_min = _burst(torch, lambda: overlay.greedy_iou_match(counts, a_list, b_list, H * W, 0.5,
                                                                               out=outs), a.iters)
                l_med, l_min = _burst(torch, lambda: overlay.match_lut(counts, a_list, b_list, outs[0], outs[2],
                                                                        gt_colors, out=lut), a.iters)
                _emit({"what": "rgbd_greedy_iou_match and rgbd_match_lut (mode gt) per call, one workgroup per image",
                       "maps": kind, "B": B, "na": na, "nb": nb, "matched": int((outs[0] >= 0).sum()),
                       "match_us_median": round(m_med * 1e3, 2), "match_us_min": round(m_min * 1e3, 2),
                       "lut_us_median": round(l_med * 1e3, 2), "lut_us_min": round(l_min * 1e3, 2)}, fh)
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
