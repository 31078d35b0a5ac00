"""rgbd_overlay_lut / rgbd_overlay_blend and their wrappers on the GPU, every result compared bit
for bit with the numpy checker (tests/checkers/overlay_ref.py, itself pinned to the reference's
output by tests/test_overlay_ref.py)."""
import numpy as np
import pytest
import torch

from checkers import overlay_cases as oc
from checkers import overlay_ref
from rgbd_amd import overlay

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("alpha", [0.6, 0.5, 0.37, 1 / 3, 0.0, 1.0])
def test_blend_arithmetic_exhaustive(alpha):
    """Every pixel value x against every colour value c, laid out as one 256 x 256 image: row = c
    (the pixel's id, its table entry the colour), column = x.  Channel 0 holds the (x, c) pair
    itself; the other two permute both, so each channel's byte lane sees every pair as well."""
    x = np.arange(256, dtype=np.int64)
    rgb = np.empty((1, 256, 256, 3), np.uint8)
    rgb[0, :, :, 0] = x[None, :]
    rgb[0, :, :, 1] = (255 - x)[None, :]
    rgb[0, :, :, 2] = ((x * 7 + 3) % 256)[None, :]
    c = np.arange(256, dtype=np.int64)
    lut = (c | ((255 - c) << 8) | (((c * 13 + 5) % 256) << 16)).astype(np.int32)[None]
    for perm in (lambda v: v, lambda v: 255 - v, lambda v: (v * 13 + 5) % 256):
        assert sorted(perm(c).tolist()) == list(range(256))
    seg = np.broadcast_to(np.arange(256, dtype=np.float32)[:, None], (256, 256))[None].copy()
    want = overlay_ref.blend(rgb, seg, lut, alpha)
    for s in (seg, seg.astype(np.int32)):
        got = overlay.blend(torch.from_numpy(rgb).to(DEV), torch.from_numpy(s).to(DEV), torch.from_numpy(lut).to(DEV),
                            alpha).cpu().numpy()
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"alpha {alpha}: {len(bad)} bytes differ, first (b, c, x, ch) = {bad[0].tolist()}"
    if alpha == 0.0:
        assert np.array_equal(want, rgb)
    if alpha == 1.0:
        assert np.array_equal(want[0, :, :, 0], np.broadcast_to(c[:, None], (256, 256)))


@pytest.mark.parametrize("dtype", oc.DTYPES)
@pytest.mark.parametrize("off", oc.OFFSETS)
@pytest.mark.parametrize("shape", oc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_blend_shapes_and_alignments(shape, off, dtype):
    """Tails, groups straddling images, ids outside the table, entries of -1, at byte offsets 0
    (the 16-byte path), 1 and 7 (the byte path, the map misaligned too) into larger allocations."""
    rgb, seg, lut, want = oc.case(shape, dtype)
    got, lead = oc.run_raw(rgb, seg, lut, oc.ALPHA, off)
    assert np.array_equal(got, want)
    assert (lead == 0xA5).all(), "bytes ahead of an offset buffer were written"
    # the pixels that must pass through do, and something was painted
    ids = np.nan_to_num(seg.astype(np.float64), nan=-1.0)
    named = (ids >= 0) & (ids < oc.N_IDS) & (ids == np.floor(ids))
    col = np.take_along_axis(lut, np.where(named, ids, 0).astype(np.int64).reshape(len(lut), -1), 1).reshape(ids.shape)
    keep = ~named | (col < 0)
    assert np.array_equal(got[keep], rgb[keep])
    if rgb.size > 100:
        assert keep.any() and (got[~keep] != rgb[~keep]).any()


@pytest.mark.parametrize("off", [1, 7])
@pytest.mark.parametrize("shape", oc.SHAPES[2:], ids=lambda s: "x".join(map(str, s)))
def test_blend_wrapper_on_offset_views(shape, off):
    """Through the wrapper: the image and the output are views with a storage offset (what a crop
    or a slice of a larger frame buffer hands over), the map stays 4-byte aligned."""
    rgb, seg, lut, want = oc.case(shape, "f32")
    n = rgb.size
    src = torch.zeros(n + 64, dtype=torch.uint8, device=DEV)
    dst = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    src[off:off + n].copy_(torch.from_numpy(rgb.reshape(-1)))
    out = overlay.blend(src[off:off + n].view(rgb.shape), torch.from_numpy(seg).to(DEV), torch.from_numpy(lut).to(DEV),
                        oc.ALPHA, out=dst[off:off + n].view(rgb.shape))
    assert np.array_equal(out.cpu().numpy(), want)
    assert (dst[:off] == 0xA5).all() and (dst[off + n:] == 0xA5).all()


def _lut_case(seed, B, Q, C, n_colors, n_ids):
    rng = np.random.RandomState(seed)
    seg_id = np.full((B, Q), -1, np.int32)
    for b in range(B):  # kept slots get the ids 0..n-1 in slot order, as rgbd_pp_instance numbers them
        kept = np.sort(rng.choice(Q, size=rng.randint(0, Q + 1), replace=False))
        seg_id[b, kept] = np.arange(len(kept))
    topk = rng.randint(0, Q * C, size=(B, Q)).astype(np.int32)
    topk[:, 1::3] = topk[:, 0::3][:, :topk[:, 1::3].shape[1]]  # duplicate labels
    pal = rng.randint(0, 256, size=(n_colors, 3)).astype(np.uint8)
    return seg_id, topk, pal


@pytest.mark.parametrize("color_by", ["label", "id"])
@pytest.mark.parametrize("B,Q,C,n_colors,n_ids", [(1, 1, 1, 1, 1), (2, 5, 5, 3, 4), (3, 100, 48, 7, 100),
                                                  (2, 300, 48, 100, 300)])
def test_lut_build(B, Q, C, n_colors, n_ids, color_by):
    seg_id, topk, pal = _lut_case(B * 100 + Q, B, Q, C, n_colors, n_ids)
    if Q >= 5:
        seg_id[0, :5] = [0, -1, 1, 2, 1]  # one id named twice: the later slot decides
        seg_id[B - 1, -1] = n_ids + 3     # an id past the table is ignored
    want = overlay_ref.build_lut(seg_id, topk, C, pal, 0 if color_by == "label" else 1, n_ids)
    got = overlay.build_lut(torch.from_numpy(seg_id).to(DEV), torch.from_numpy(topk).to(DEV), C,
                            torch.from_numpy(pal).to(DEV), color_by, n_ids)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    if Q >= 5:
        assert (want == -1).any() and (want >= 0).any()
    # the palette may also be given as tuples
    got2 = overlay.build_lut(torch.from_numpy(seg_id).to(DEV), torch.from_numpy(topk).to(DEV), C,
                             [tuple(int(v) for v in p) for p in pal], color_by, n_ids)
    assert torch.equal(got, got2)


def test_overlay_segments_hf_format(golden):
    """The reference's call shape on its own fixture: one result dict and an id -> colour mapping."""
    g = golden("g10_overlay")
    colors = {int(k): tuple(int(v) for v in rgb) for k, rgb in zip(g["color_ids"], g["color_rgb"])}
    img = torch.from_numpy(g["image"]).to(DEV)
    res = {"segmentation": torch.from_numpy(g["seg"]).to(DEV), "segments_info": [{"id": int(i)} for i in g["ids"]]}
    for alpha, want in zip(g["alphas"].tolist(), g["overlays"]):
        got = overlay.overlay_segments(img, res, colors, alpha=alpha)
        assert got.is_cuda and got.dtype == torch.uint8 and got.shape == img.shape
        assert np.array_equal(got.cpu().numpy(), want), f"alpha {alpha}"
    # a batch; only the ids segments_info lists are painted; an int64 class map is taken too
    res2 = {"segmentation": torch.from_numpy(g["seg"]).to(DEV).long(), "segments_info": [{"id": 1}, {"id": 5}]}
    res1 = dict(res, segmentation=res["segmentation"].long())
    got = overlay.overlay_segments(torch.stack([img, img]), [res1, res2], colors).cpu().numpy()
    assert np.array_equal(got[0], g["overlays"][0])
    lut2 = overlay_ref.lut_from_colors(colors, [1, 5], 6)
    assert np.array_equal(got[1], overlay_ref.blend(g["image"][None], g["seg"][None], lut2[None], 0.6)[0])
    # nothing kept: the frame comes back
    none = {"segmentation": torch.full((24, 40), -1.0, device=DEV), "segments_info": []}
    assert torch.equal(overlay.overlay_segments(img, none, colors), img)


def test_refusals():
    img = torch.zeros(2, 4, 6, 3, dtype=torch.uint8, device=DEV)
    seg = torch.zeros(2, 4, 6, device=DEV)
    lut = torch.zeros(2, 3, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="GPU only"):
        overlay.blend(img.cpu(), seg, lut)
    with pytest.raises(RuntimeError, match="GPU only"):
        overlay.blend(img, seg.cpu(), lut)
    with pytest.raises(RuntimeError, match="contiguous"):
        overlay.blend(torch.zeros(2, 4, 6, 4, dtype=torch.uint8, device=DEV)[..., :3], seg, lut)  # RGBA's RGB
    with pytest.raises(RuntimeError, match="contiguous"):
        overlay.blend(img, seg.transpose(1, 2).contiguous().transpose(1, 2), lut)
    with pytest.raises(ValueError):
        overlay.blend(img, seg.double(), lut)
    with pytest.raises(ValueError):
        overlay.blend(img, seg[:1], lut)
    with pytest.raises(RuntimeError, match="bad argument"):
        overlay.blend(img, seg, lut, out=img)  # in place
    with pytest.raises(RuntimeError, match="GPU only"):
        overlay.overlay_segments(img[0], {"segmentation": seg[0].cpu(), "segments_info": []}, {})
    with pytest.raises(ValueError):
        overlay.build_lut(lut, lut, 5, [(1, 2, 3)], color_by="score")
