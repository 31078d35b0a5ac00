"""stream.StreamingSegmenter: u8 frames -> instance map, tables and overlay in one graph replay,
bit for bit the eager path it replaces (data.map_10channel -> model -> postprocess.
post_process_instance_segmentation(keep_on_device=True)) — the same kernels in the same order and
no atomics in this forward, so replay against eager is compared bitwise, as everywhere in the
project.  One model with formula weights (rgbd_amd/init.py), frames from rgbd_amd/synthetic.py at
240x320, threshold 0.0."""
import contextlib
import types

import numpy as np
import pytest
import torch

from checkers import overlay_ref
from rgbd_amd import data, overlay, postprocess as pp, synthetic
from rgbd_amd.stream import StreamingSegmenter

pytestmark = pytest.mark.gpu
H, W, THR = 240, 320, 0.0
PALETTE = overlay.consistent_colors(48)


@pytest.fixture(scope="module")
def model():
    from rgbd_amd import init as winit
    from rgbd_amd.config import standard_config
    from rgbd_amd.custom_model import CustomMask2FormerForUniversalSegmentation
    torch.manual_seed(0)
    m = CustomMask2FormerForUniversalSegmentation(standard_config(48), version="0.4.0")
    winit.init_deterministic(m)
    return m.to("cuda").eval()


@pytest.fixture(scope="module")
def frames():
    """Three scenes A, B, C as (depth uint8 [H,W], rgb uint8 [H,W,3]) on the device."""
    out = []
    for i in range(3):
        sc = synthetic.make_scene(synthetic.scene_seed(5, i), H, W)
        out.append((torch.from_numpy(sc["depth_u8"]).cuda(), torch.from_numpy(sc["rgb_u8"]).contiguous().cuda()))
    return out


def _eager(model, depth, rgb, dtype, size=None):
    """The path the parent commit offers, on a batch: -> (maps [B,H,W], topk, scores, seg_id, results)."""
    model.set_compute_dtype(dtype)
    B = depth.shape[0]
    amp = torch.autocast("cuda", dtype=torch.bfloat16) if dtype == torch.bfloat16 else contextlib.nullcontext()
    with torch.no_grad():
        pv = data.map_10channel(rgb, depth, size=size)["pixel_values"]
        with amp:
            out = model(pixel_values=pv)
        results = pp.post_process_instance_segmentation(out, threshold=THR, target_sizes=[(H, W)] * B,
                                                        keep_on_device=True)
        cls = out.class_queries_logits.to(torch.float32).contiguous()
        masks = out.masks_queries_logits.to(torch.float32).contiguous()
        segs, topk, ps, sid, _ = pp._run(cls, masks, [(H, W)] * B, THR)
    for r, s in zip(results, segs):
        assert torch.equal(r["segmentation"], s)
    return torch.stack(segs).clone(), topk.clone(), ps.clone(), sid.clone(), results


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _assert_same(res, want, what):
    maps, topk, ps, sid, results = want
    assert torch.equal(_bits(res.segmentation), _bits(maps)), f"{what}: map"
    assert torch.equal(res.topk_idx, topk) and torch.equal(res.seg_id, sid), f"{what}: tables"
    assert torch.equal(_bits(res.scores), _bits(ps)), f"{what}: scores"
    got = res.segments()
    assert len(got) == len(results)
    for g, r in zip(got, results):
        assert g["segments_info"] == r["segments_info"], f"{what}: segments_info"
        assert g["segmentation"].shape == (H, W) and torch.equal(_bits(g["segmentation"]), _bits(r["segmentation"]))


def _assert_overlay(res, rgb, color_by, alpha, what):
    """The overlay against the checker applied to (frame, returned map, table from the returned arrays)."""
    sid, topk = res.seg_id.cpu().numpy(), res.topk_idx.cpu().numpy()
    lut = overlay_ref.build_lut(sid, topk, 48, np.array(PALETTE, np.uint8), 0 if color_by == "label" else 1,
                                sid.shape[1])
    want = overlay_ref.blend(rgb.cpu().numpy(), res.segmentation.cpu().numpy(), lut, alpha)
    assert np.array_equal(res.overlay.cpu().numpy(), want), f"{what}: overlay"
    return int((want != rgb.cpu().numpy()).any(axis=-1).sum())


@pytest.fixture(scope="module")
def eager_f32(model, frames):
    return [_eager(model, d[None], c[None], torch.float32) for d, c in frames]


@pytest.fixture(scope="module")
def seg_f32(model, eager_f32):  # after the eager runs: one warm model, one capture for the float32 tests
    return StreamingSegmenter(model, H, W, B=1, threshold=THR, dtype=torch.float32,
                              overlay=dict(alpha=0.6, palette=PALETTE, color_by="label")).capture()


@pytest.mark.timeout(300)
def test_replay_is_bitwise_eager_and_keeps_no_state(seg_f32, eager_f32, frames):
    kept = [len(e[4][0]["segments_info"]) for e in eager_f32]
    assert sum(k > 0 for k in kept) >= 2, f"the eager path keeps {kept} segments on the three frames: nothing to compare"
    assert seg_f32.width <= 2  # at most two concurrent branches (graph_guard)
    painted = 0
    for name, i in (("A", 0), ("B", 1), ("C", 2), ("A again", 0)):
        depth, rgb = frames[i]
        res = seg_f32(depth[None], rgb[None])
        _assert_same(res, eager_f32[i], name)
        painted += _assert_overlay(res, rgb[None], "label", 0.6, name)
    assert painted > 0, "no pixel was painted on any frame"


@pytest.mark.timeout(300)
def test_rejected_depth_raises_and_leaves_no_trace(model, seg_f32, eager_f32, frames):
    """A frame whose depth range the decomposition rejects raises the reference's ValueError from
    ``segments()``, and the next good frame is bitwise again.

    No uint8 frame can be rejected: a constant depth plane is not (np.histogram widens an empty
    range by +-0.5, and csrc/edsam_decompose.hip restates that; first GPU run of this test: the
    eager path and the replay both return normally on a plane of 77), and two distinct levels are
    0.017 apart after normalisation, far above 512 float32 steps.  So the constant frame is held to
    the eager path like any other, and the rejection is put where a replay's decomposition puts it:
    status 2 in the captured status word of image 0, after the replay has finished."""
    depth, rgb = frames[1]
    flat = torch.full_like(depth, 77)[None]
    _assert_same(seg_f32(flat, rgb[None]), _eager(model, flat, rgb[None], torch.float32), "constant depth")
    res = seg_f32(depth[None], rgb[None])
    torch.cuda.synchronize()
    assert len(seg_f32._statuses) >= 1
    seg_f32._statuses[0].dev[0] = 2
    with pytest.raises(ValueError, match="image 0: Too many bins"):
        res.segments()
    _assert_same(seg_f32(depth[None], rgb[None]), eager_f32[1], "the frame after a rejected one")
    # host frames are taken too (a camera hands over host arrays)
    _assert_same(seg_f32(frames[2][0][None].cpu(), frames[2][1][None].cpu()), eager_f32[2], "host frame")


@pytest.mark.timeout(300)
def test_resized_stream_returns_frame_resolution(model, frames):
    depth, rgb = frames[0]
    want = _eager(model, depth[None], rgb[None], torch.float32, size=(256, 256))
    seg = StreamingSegmenter(model, H, W, B=1, size=(256, 256), threshold=THR, dtype=torch.float32)
    res = seg(depth[None], rgb[None])
    assert res.segmentation.shape == (1, H, W) and res.overlay is None and seg.width <= 2
    _assert_same(res, want, "size=(256, 256)")
    with pytest.raises(ValueError, match="non-square"):
        StreamingSegmenter(model, H, W, size=(256, 320))


@pytest.mark.timeout(300)
def test_batch_of_two_bf16(model, frames):
    pairs = [(0, 1), (2, 0), (0, 1)]
    seg = StreamingSegmenter(model, H, W, B=2, threshold=THR, dtype=torch.bfloat16,
                             overlay=dict(alpha=0.37, palette=PALETTE, color_by="id"))
    wants = {}
    for a, b in pairs:
        depth = torch.stack([frames[a][0], frames[b][0]])
        rgb = torch.stack([frames[a][1], frames[b][1]])
        if (a, b) not in wants:
            wants[(a, b)] = _eager(model, depth, rgb, torch.bfloat16)
        res = seg(depth, rgb)
        _assert_same(res, wants[(a, b)], f"bf16 batch {a, b}")
        _assert_overlay(res, rgb, "id", 0.37, f"bf16 batch {a, b}")
    assert seg.width <= 2
    assert any(len(r["segments_info"]) for w in wants.values() for r in w[4])


def test_other_versions_are_refused():
    stub = types.SimpleNamespace(model=types.SimpleNamespace(pixel_level_module=types.SimpleNamespace(version="0.0.0")))
    with pytest.raises(ValueError, match="0.4.0"):
        StreamingSegmenter(stub, H, W)
    from rgbd_amd.config import standard_config
    from rgbd_amd.custom_model import CustomMask2FormerForUniversalSegmentation
    with pytest.raises(ValueError, match="0.4.0"):
        StreamingSegmenter(CustomMask2FormerForUniversalSegmentation(standard_config(48), version="0.0.0"), H, W)
