"""Generate tests/golden/g10_overlay.npz by importing the REFERENCE's predictor itself.

Runs only where the reference checkout is present (not on the GPU box):
    python tests/golden/make_overlay_golden.py

mask2former/predictor.py imports cv2, pycocotools, matplotlib and tqdm at module level; none of
them is touched by the two functions recorded here, so whichever is absent is replaced by an
empty module for the import (the device make_golden.py uses for cv2).  No file of the reference
is modified or copied; the fixture holds data only:

  record 1  a 24x40 uint8 image, a float32 map with ids -1..5, segments_info ids, a colour
            mapping (id 4 is left out of it: the reference's grey default) and the output of
            _create_gt_overlay_with_consistent_colors at alpha 0.6 and 0.37
  record 2  generate_consistent_colors(100)
"""
import importlib
import sys
import types
from pathlib import Path

import numpy as np

REF = "/root/reference"
OUT = Path(__file__).resolve().parent / "g10_overlay.npz"


def _shim(name, **attrs):
    try:
        importlib.import_module(name)
    except ImportError:
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        sys.modules[name] = mod
        return mod
    return sys.modules[name]


def import_predictor():
    _shim("cv2")
    pkg = _shim("pycocotools")
    mask = _shim("pycocotools.mask")
    if not hasattr(pkg, "mask"):
        pkg.mask = mask
    mpl = _shim("matplotlib")
    plt = _shim("matplotlib.pyplot")
    if not hasattr(mpl, "pyplot"):
        mpl.pyplot = plt
    _shim("tqdm", tqdm=lambda it=None, *a, **k: it)
    if REF not in sys.path:
        sys.path.insert(0, REF)
    return importlib.import_module("mask2former.predictor")


def main():
    pred = import_predictor()
    rng = np.random.RandomState(10)
    H, W = 24, 40
    image = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    image[0, :16, 0] = np.arange(240, 256)  # bright and dark runs: the clip and the truncation
    image[1, :16, 1] = np.arange(0, 16)
    seg = rng.randint(-1, 6, size=(H, W)).astype(np.float32)
    ids = [0, 1, 2, 3, 4, 5]
    colors = {0: (255, 0, 0), 1: (0, 255, 0), 2: (13, 77, 201), 3: (254, 253, 1), 5: (50, 128, 99)}  # 4: default grey
    prediction = {"segmentation": seg, "segments_info": [{"id": i} for i in ids]}
    alphas = [0.6, 0.37]
    outs = [pred._create_gt_overlay_with_consistent_colors(image, prediction, colors, alpha=a) for a in alphas]
    state = np.random.get_state()
    palette = pred.generate_consistent_colors(100)
    np.random.set_state(state)
    np.savez_compressed(
        OUT, image=image, seg=seg, ids=np.array(ids, np.int32),
        color_ids=np.array(sorted(colors), np.int32), color_rgb=np.array([colors[k] for k in sorted(colors)], np.uint8),
        alphas=np.array(alphas, np.float64), overlays=np.stack(outs).astype(np.uint8),
        palette100=np.array(palette, np.int32), numpy_version=np.array(np.__version__))
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes), numpy {np.__version__}")


if __name__ == "__main__":
    main()
