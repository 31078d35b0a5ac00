"""Generate tests/golden/k5_sizes.json: what the K5 size queries of the C ABI return.

    python tests/golden/make_k5_sizes_golden.py [path/to/librgbd_hip.so]

The committed file was produced by the library built from commit 9665e93, the last one with all of
K5 in csrc/dsam_conv.hip, before that file was split by leg.  The queries are host arithmetic (no
device needed), and a slip in them is a device buffer overrun, so tests/test_k5_sizes.py holds every
later library to these values.  Regenerate only when a change means to alter a plan or workspace
layout, and say so in that commit.

Shapes: kinds FWD / DX / DW x dtypes f32 / bf16 x (Cin, Cout) with all three chunk groupings
(KC = 3, 2, 1) and dW tile heights (FM = 6, 4, 2) x (B, h, w) covering the 8 x 16-tile and linear
tilings, ragged edges and the one-pixel grid.

  sizes   rows [dtype, kind, Cin, Cout, B, h, w, rgbd_dsam_plan_size, rgbd_dsam_run_workspace_size]
  packed  rows [dtype, Cin, Cout, rgbd_dsam_packed_elems]
"""
import ctypes
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
OUT = HERE / "k5_sizes.json"
DEFAULT_LIB = HERE.parents[1] / "rgb-d-instance-segmentation_amd" / "librgbd_hip.so"

DTYPES = [0, 1]  # RGBD_F32, RGBD_BF16
KINDS = [0, 1, 2]  # RGBD_LEG_FWD, RGBD_LEG_DX, RGBD_LEG_DW
CHANNELS = [(96, 192), (192, 384), (384, 768), (64, 96), (32, 32)]
GRIDS = [(8, 120, 160), (3, 25, 33), (2, 16, 24), (1, 180, 320), (1, 1, 1)]


def bind(path):
    L = ctypes.CDLL(str(path))
    L.rgbd_dsam_plan_size.restype = ctypes.c_size_t
    L.rgbd_dsam_plan_size.argtypes = [ctypes.c_int] * 6
    L.rgbd_dsam_run_workspace_size.restype = ctypes.c_size_t
    L.rgbd_dsam_run_workspace_size.argtypes = [ctypes.c_int] * 7
    L.rgbd_dsam_packed_elems.restype = ctypes.c_longlong
    L.rgbd_dsam_packed_elems.argtypes = [ctypes.c_int] * 3
    return L


def query(L):
    sizes = [[dt, kind, ci, co, B, h, w, L.rgbd_dsam_plan_size(kind, B, ci, h, w, co),
              L.rgbd_dsam_run_workspace_size(dt, kind, B, ci, h, w, co)]
             for dt in DTYPES for kind in KINDS for ci, co in CHANNELS for B, h, w in GRIDS]
    packed = [[dt, ci, co, L.rgbd_dsam_packed_elems(dt, ci, co)] for dt in DTYPES for ci, co in CHANNELS]
    return {"sizes": sizes, "packed": packed}


def main():
    got = query(bind(sys.argv[1] if len(sys.argv) > 1 else DEFAULT_LIB))
    rows = lambda v: "[\n" + ",\n".join("  " + json.dumps(r) for r in v) + "\n ]"
    OUT.write_text("{\n" + ",\n".join(f' "{k}": {rows(v)}' for k, v in got.items()) + "\n}\n")
    print(f"wrote {OUT}: {len(got['sizes'])} size rows, {len(got['packed'])} packed rows")


if __name__ == "__main__":
    main()
