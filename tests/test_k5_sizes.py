"""The K5 plan / workspace / packed-weight size queries return exactly the recorded values
(tests/golden/k5_sizes.json, see make_k5_sizes_golden.py).  Host arithmetic only: no GPU.  The
callers allocate what these return and the kernels index by the same formulas, so a slip here is a
device buffer overrun."""
import json
from pathlib import Path

from rgbd_amd import _lib

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "k5_sizes.json").read_text())


def test_golden_covers_the_table():
    sizes = GOLDEN["sizes"]
    assert len(sizes) == 2 * 3 * 5 * 5 and len({tuple(r[:7]) for r in sizes}) == len(sizes)
    assert {r[0] for r in sizes} == {_lib.RGBD_F32, _lib.RGBD_BF16} and {r[1] for r in sizes} == {0, 1, 2}
    assert {(r[2], r[3]) for r in sizes} == {(96, 192), (192, 384), (384, 768), (64, 96), (32, 32)}
    assert {tuple(r[4:7]) for r in sizes} == {(8, 120, 160), (3, 25, 33), (2, 16, 24), (1, 180, 320), (1, 1, 1)}
    assert len(GOLDEN["packed"]) == 2 * 5


def test_plan_and_run_workspace_sizes_match_golden():
    L = _lib.lib()
    bad = []
    for dt, kind, ci, co, B, h, w, plan, run in GOLDEN["sizes"]:
        got = (L.rgbd_dsam_plan_size(kind, B, ci, h, w, co), L.rgbd_dsam_run_workspace_size(dt, kind, B, ci, h, w, co))
        if got != (plan, run):
            bad.append(((dt, kind, ci, co, B, h, w), got, (plan, run)))
    assert not bad, bad[:5]


def test_packed_elems_match_golden():
    L = _lib.lib()
    for dt, ci, co, n in GOLDEN["packed"]:
        assert L.rgbd_dsam_packed_elems(dt, ci, co) == n, (dt, ci, co)
