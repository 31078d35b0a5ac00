"""Mask-logit error of the whole model against the reference fixtures (G5 320x240, G7 640x480)
with the bf16 hot path in its plain mode and in the float32-interface mode,
by bench.parity's own definition: unforced, and with the reference's attention masks forced
(arithmetic only).  Each mode also with the ratio predictor alone in float32 (the reference's
window decisions): what remains then is the rounding of the DSAM operands (activations and
code-merged filters to bf16) alone.

    python tools/parity_interface_dtype.py [--fixtures g5 g7]

bench.parity sets the model's mode through set_compute_dtype(dtype); for the new mode that
method is wrapped here to add interface=torch.float32 (bench.py itself is not touched).  Prints
one JSON line per run and a table."""
import argparse
import json
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "tests/golden")]
import torch  # noqa: E402

import bench  # noqa: E402
from rgbd_amd.custom_model import CustomMask2FormerForUniversalSegmentation as Model  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--fixtures", nargs="+", default=["g5", "g7"])
a = ap.parse_args()
dev = torch.device("cuda")
orig = Model.set_compute_dtype
rows = []
for fx in a.fixtures:
    for interface in (None, torch.float32):
        for ratio_fp32 in (False, True):
            Model.set_compute_dtype = lambda self, dtype, _i=interface: orig(self, dtype, _i)
            try:
                r = bench.parity(dev, torch.bfloat16, ratio_fp32=ratio_fp32, fixture=fx)
            finally:
                Model.set_compute_dtype = orig
            row = {"fixture": fx, "mode": "bf16" if interface is None else "bf16+f32io",
                   "ratio_predictor": "f32" if ratio_fp32 else "bf16",
                   "forced_rel": r["mask_logit_max_rel_err_masks_forced"], "unforced_rel": r["mask_logit_max_rel_err"],
                   "attention_flips_unforced": r["attention_flips"]["unforced_run"],
                   "region_code_cells_flipped": r["region_code_cells_flipped"], "input_sha_match": r["input_sha_match"]}
            rows.append(row)
            print(json.dumps(row), flush=True)
print(f"{'fixture':8s}{'mode':12s}{'ratio':7s}{'forced rel':>12s}{'unforced rel':>14s}")
for r in rows:
    print(f"{r['fixture']:8s}{r['mode']:12s}{r['ratio_predictor']:7s}{r['forced_rel']:12.3e}{r['unforced_rel']:14.3e}")
