"""The overlay checker (tests/checkers/overlay_ref.py) and ``overlay.consistent_colors`` against
the reference's own output, recorded in tests/golden/g10_overlay.npz (make_overlay_golden.py):
the numpy restatement the GPU tests compare against is the reference's arithmetic, bit for bit."""
import numpy as np

from checkers import overlay_ref
from rgbd_amd import overlay


def test_checker_reproduces_reference_overlay(golden):
    g = golden("g10_overlay")
    image, seg = g["image"], g["seg"]
    assert image.shape == (24, 40, 3) and seg.min() == -1 and seg.max() == 5
    colors = {int(k): tuple(int(v) for v in rgb) for k, rgb in zip(g["color_ids"], g["color_rgb"])}
    assert 4 not in colors  # one id takes the reference's default grey
    lut = overlay_ref.lut_from_colors(colors, g["ids"].tolist(), 6)
    for alpha, want in zip(g["alphas"].tolist(), g["overlays"]):
        got = overlay_ref.blend(image[None], seg[None], lut[None], alpha)[0]
        assert got.dtype == np.uint8 and np.array_equal(got, want), f"alpha {alpha}"
        # the int32 form of the same map paints the same pixels
        assert np.array_equal(overlay_ref.blend(image[None], seg[None].astype(np.int32), lut[None], alpha)[0], want)
    assert (g["overlays"][0] != g["overlays"][1]).any() and (g["overlays"][0] != image).any()


def test_checker_leaves_unnamed_pixels_alone(golden):
    g = golden("g10_overlay")
    image, seg = g["image"], g["seg"].copy()
    seg[0, 0], seg[0, 1], seg[0, 2] = 2.5, 7.0, np.nan  # not an integer, past the table, NaN
    lut = overlay_ref.lut_from_colors({}, [0, 1, 2, 3], 6)  # ids 4 and 5 have no entry
    got = overlay_ref.blend(image[None], seg[None], lut[None], 0.6)[0]
    keep = (seg < 0) | (seg > 3) | np.isnan(seg) | (seg != np.floor(seg))
    assert np.array_equal(got[keep], image[keep]) and (got[~keep] != image[~keep]).any()


def test_lut_build_rules():
    seg_id = np.array([[0, -1, 1, 2, 1], [-1, -1, -1, 0, 9]], np.int32)
    topk = np.array([[7, 3, 12, 7, 5], [1, 2, 3, 4, 5]], np.int32)  # flat query * C + class indices, C = 5
    pal = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 90]], np.uint8)

    def packed(k):
        r, g, b = (int(v) for v in pal[k % 3])
        return r | (g << 8) | (b << 16)
    by_label = overlay_ref.build_lut(seg_id, topk, 5, pal, 0, 4)
    # id 1 is named by slots 2 and 4: the later one (label 5 % 5 = 0) decides; labels wrap the palette
    assert by_label.tolist() == [[packed(2), packed(0), packed(2), -1], [packed(4), -1, -1, -1]]
    by_id = overlay_ref.build_lut(seg_id, topk, 5, pal, 1, 4)
    assert by_id.tolist() == [[packed(0), packed(1), packed(2), -1], [packed(0), -1, -1, -1]]


def test_consistent_colors_match_reference_and_spare_global_state(golden):
    g = golden("g10_overlay")
    np.random.seed(1234)
    before = np.random.get_state()
    got = overlay.consistent_colors(100)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert got == [tuple(int(v) for v in row) for row in g["palette100"]]
    assert all(isinstance(v, int) and 50 <= v < 255 for c in got for v in c)
    assert overlay.consistent_colors(3) == got[:3] and overlay.consistent_colors(3, seed=7) != got[:3]
