"""Times of the two launches the end-to-end mode adds to the hot path's backward, from a
rocprofv3 kernel trace (csv) of `tools/bench_full_model.py --arms hip:e2e`: the colour-gradient
kernel (k_color_grads) and dsam0's dX leg (the last k_dsam_lds dispatch before each k_color_grads:
the cascade runs dX2, dX1, dX0 on one stream and the colour-gradient launch follows dX0).  The
colour-gradient kernel's traffic is computed from the shapes (bf16: G, D and out of scales 0-2, G
and out of scale 3) and reported as GB/s and as a share of 8 TB/s.

    python tools/e2e_kernel_times.py <kernel_trace.csv> [--batch 8 --height 480 --width 640]"""
import argparse
import csv
import json
import statistics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--skip", type=int, default=2, help="leading steps left out (warm-up)")
    args = ap.parse_args()
    rows = []
    for r in csv.DictReader(open(args.trace)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    cg, dx0, nhwc = [], [], []
    last_ld = last_nhwc = None
    for s, e, name in rows:
        if "k_dsam_lds" in name:
            last_ld = e - s
        elif "k_nchw_to_nhwc_multi" in name:
            last_nhwc = e - s
        elif "k_color_grads" in name:
            cg.append(e - s)
            dx0.append(last_ld)
            nhwc.append(last_nhwc)
    cg, dx0, nhwc = cg[args.skip:], dx0[args.skip:], [t for t in nhwc[args.skip:] if t is not None]
    h, w, elems = -(-args.height // 4), -(-args.width // 4), []
    for c in (96, 192, 384, 768):
        elems.append(args.batch * c * h * w)
        h, w = -(-h // 2), -(-w // 2)
    cg_bytes = 2 * (3 * sum(elems[:3]) + 2 * elems[3])
    nhwc_bytes = 2 * 2 * sum(elems)  # the backward's four-job bf16 NCHW -> NHWC launch: read + write
    med = statistics.median

    def bw(nbytes, ns):
        return {"us": round(med(ns) / 1e3, 2), "us_min": round(min(ns) / 1e3, 2), "us_max": round(max(ns) / 1e3, 2),
                "MB": round(nbytes / 1e6, 1), "GB_s": round(nbytes / med(ns), 1),
                "share_of_8TB_s": round(nbytes / med(ns) / 8000, 3)}
    out = {"steps": len(cg), "k_color_grads": bw(cg_bytes, cg),
           "dsam0_dx": {"us": round(med(dx0) / 1e3, 2), "us_min": round(min(dx0) / 1e3, 2),
                        "us_max": round(max(dx0) / 1e3, 2)}}
    if nhwc:
        out["k_nchw_to_nhwc_multi_before_it"] = bw(nhwc_bytes, nhwc)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
