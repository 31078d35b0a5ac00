"""csrc/segment_match.hip on the GPU against the numpy checker (tests/checkers/match_ref.py, itself
pinned to the reference's output by tests/test_match_ref.py) and against the reference's recorded
output G11.  Everything is integer counts and float64 quotients of integers: every comparison is
exact equality."""
from pathlib import Path

import numpy as np
import pytest
import torch

from checkers import match_cases as mc, match_ref
from rgbd_amd import overlay

pytestmark = pytest.mark.gpu
G11 = Path(__file__).parent / "golden" / "g11_match.npz"


@pytest.mark.parametrize("ranges", mc.RANGES, ids=lambda r: f"{r[0]}x{r[1]}")
@pytest.mark.parametrize("shape", mc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_contingency_is_the_checker(shape, ranges):
    """Both accumulation paths (mc.RANGES: the first four ranges take the LDS table, (256, 256) the
    global one), both load widths (offsets (0, 0): 16-byte loads, every other pair: a lane per
    cell), all four dtype pairs, shared and unshared keys."""
    na, nb = ranges
    for kind in mc.KINDS:
        for da in mc.DTYPES:
            for db in mc.DTYPES:
                a, b, want = mc.contingency_case(shape, ranges, (da, db), kind)
                assert want.sum() == a.size
                for off_a in mc.OFFSETS:
                    for off_b in mc.OFFSETS:
                        got, lead = mc.run_contingency_raw(a, b, na, nb, off_a, off_b)
                        assert np.array_equal(got, want), (kind, da, db, off_a, off_b)
                        assert (lead == 0xA5).all()


def test_contingency_of_a_map_with_itself_and_wrapper_shapes():
    a, _, _ = mc.contingency_case((3, 33, 129), (100, 100), ("f32", "i32"), "blocks")
    d = torch.from_numpy(a).cuda()
    c = overlay.label_contingency(d, d, 100, 100)
    assert np.array_equal(c.cpu().numpy(), match_ref.contingency(a, a, 100, 100))
    off = c[:, :100, :100] * (1 - torch.eye(100, dtype=torch.int32, device="cuda"))
    assert int(off.abs().sum()) == 0        # a map against itself: a diagonal table
    out = torch.full((3, 101, 101), 7, dtype=torch.int32, device="cuda")
    assert overlay.label_contingency(d, d, 100, 100, out=out) is out and torch.equal(out, c)
    with pytest.raises(ValueError):
        overlay.label_contingency(d, d[:2], 100, 100)
    with pytest.raises(overlay._lib.RgbdHipError, match="unsupported shape"):
        overlay.label_contingency(d, d, 257, 3)


@pytest.mark.parametrize("thr", [0.5, 0.0, 1.0])
@pytest.mark.parametrize("G", [0, 1, 7, 100])
@pytest.mark.parametrize("P", [0, 1, 7, 100])
def test_greedy_match_is_the_checker(P, G, thr):
    counts, a_list, b_list, hw = mc.table_case(P, G)
    want = match_ref.greedy_match(counts, a_list, b_list, thr)
    got, _ = mc.run_match_raw(counts, a_list, b_list, hw, thr)
    for g, w, what in zip(got, want, ("matched", "b_match_count", "n_filtered")):
        assert np.array_equal(g, w), what
    if P == 100 and G == 100 and thr < 1.0:
        assert (want[0] >= 0).sum() > 50     # the case does match


def test_lut_and_track_kernels_are_the_checker():
    counts, a_list, b_list, hw = mc.table_case(100, 100)
    matched, b_count, n_f = match_ref.greedy_match(counts, a_list, b_list, 0.0)
    rng = np.random.RandomState(4)
    B, na, nb = counts.shape[0], counts.shape[1] - 1, counts.shape[2] - 1
    gt_colors = rng.randint(0, 1 << 24, size=(B, nb)).astype(np.int32)
    gt_colors[:, ::4] = -1
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    lut = overlay.match_lut(d(counts), d(a_list), d(b_list), d(matched), d(n_f), d(gt_colors), (9, 8, 7))
    want = match_ref.gt_lut(counts, a_list, b_list, matched, n_f, gt_colors, match_ref.pack((9, 8, 7)))
    assert np.array_equal(lut.cpu().numpy(), want)
    assert (want == match_ref.pack((9, 8, 7))).any() and (want == -1).any() and (want >= 0).sum() > 50
    # tracks: a square table, identity lists
    Q = 37
    sq = np.zeros((2, Q + 1, Q + 1), np.int32)
    sq[:, :Q, :Q] = rng.randint(0, 3, size=(2, Q, Q)) * (rng.rand(2, Q, Q) < 0.1)
    sq[:, 5, :] = 0
    sq[:, :, 9] = 0
    ids = np.tile(np.arange(Q, dtype=np.int32), (2, 1))
    m, _, _ = match_ref.greedy_match(sq, ids, ids, 0.3)
    prev = rng.permutation(2 * Q).astype(np.int32).reshape(2, Q)
    prev[:, 9] = -1
    nxt = np.array([100, 7], np.int32)
    want_t, want_n = match_ref.track_assign(sq, m, prev, nxt)
    d_n = d(nxt)
    got_t = overlay.track_assign(d(sq), d(m), d(prev), d_n)
    assert np.array_equal(got_t.cpu().numpy(), want_t) and np.array_equal(d_n.cpu().numpy(), want_n)
    assert (want_t >= 100).any() and (want_t == -1).any() and (want_n > nxt).all()
    pal = np.array(overlay.consistent_colors(11), np.uint8)
    assert np.array_equal(overlay.track_lut(got_t, d(pal)).cpu().numpy(), match_ref.track_lut(want_t, pal))


@pytest.fixture(scope="module")
def g11():
    return np.load(G11)


def _case(g11, k, dtype=torch.float32):
    g = {n.split("_", 1)[1]: g11[n] for n in g11.files if n.startswith(f"c{k}_")}
    pred = {"segmentation": torch.from_numpy(g["pred"]).cuda().to(dtype),
            "segments_info": [{"id": int(i), "label_id": 0, "score": 1.0} for i in g["pred_ids"]]}
    gt = {"segmentation": torch.from_numpy(g["gt"]).cuda().to(dtype),
          "segments_info": [{"id": int(i), "label_id": 0} for i in g["gt_ids"]]}
    colors = {int(i): tuple(int(v) for v in c) for i, c in zip(g["color_ids"], g["color_rgb"])}
    return g, pred, gt, colors


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.int64], ids=["f32", "i32", "i64"])
@pytest.mark.parametrize("k", range(8))
def test_wrappers_are_the_reference_on_g11(g11, k, dtype):
    g, pred, gt, colors = _case(g11, k, dtype)
    image = torch.from_numpy(g11["image"]).cuda()
    thr = float(g["thr"])
    matched, is_matched, counts = overlay.match_segments(pred, gt, iou_threshold=thr)
    assert matched == g["matched"].tolist() and is_matched == g["is_matched"].tolist()
    assert counts == g["gt_counts"].tolist()
    for alpha, want in zip(g11["alphas"], g["overlays"]):
        got = overlay.consistent_prediction_overlay(image, pred, colors, gt, alpha=float(alpha), iou_threshold=thr)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), f"alpha {alpha}"


def test_wrappers_on_the_g11_batch(g11):
    """All eight cases as one batch (per-image lists, id ranges and colour mappings), and the device
    tensors of return_tensors."""
    cases = [_case(g11, k) for k in range(8)]
    image = torch.from_numpy(g11["image"]).cuda()
    same_thr = [i for i, c in enumerate(cases) if float(c[0]["thr"]) == 0.5]
    preds, gts = [cases[i][1] for i in same_thr], [cases[i][2] for i in same_thr]
    triples = overlay.match_segments(preds, gts, iou_threshold=0.5)
    for i, (m, im, c) in zip(same_thr, triples):
        g = cases[i][0]
        assert m == g["matched"].tolist() and im == g["is_matched"].tolist() and c == g["gt_counts"].tolist()
    out = overlay.consistent_prediction_overlay(image[None].expand(len(same_thr), -1, -1, -1).contiguous(), preds,
                                                [cases[i][3] for i in same_thr], gts, alpha=0.37)
    for row, i in zip(out, same_thr):
        assert np.array_equal(row.cpu().numpy(), cases[i][0]["overlays"][1])
    t = overlay.match_segments(preds, gts, return_tensors=True)
    assert t["matched"].is_cuda and t["counts"].dtype == torch.int32 and t["n_filtered"].shape == (len(same_thr), 2)
