"""stream.StreamingSegmenter(track=...): ids that are stable from frame to frame, computed inside
the captured graph.  Every replay is held bitwise to the eager composition (the eager path of
tests/test_gpu_stream_segment.py, then overlay.label_contingency -> greedy_iou_match ->
track_assign on state kept here), ``track_id`` to the numpy checker run over the successive
returned maps, and the ``color_by="track"`` overlay to the checker's blend.  240x320, threshold 0.0."""
import numpy as np
import pytest
import torch

from checkers import match_ref, overlay_ref
from rgbd_amd import overlay
from rgbd_amd.stream import StreamingSegmenter
from test_gpu_stream_segment import H, W, THR, PALETTE, _assert_same, _eager, frames, model  # noqa: F401

pytestmark = pytest.mark.gpu
IOU = 0.5


class EagerTracks:
    """The tracking stage composed from the wrappers, with its own device state."""

    def __init__(self, B, Q):
        self.B, self.Q = B, Q
        self.ids = torch.arange(Q, dtype=torch.int32, device="cuda").repeat(B, 1).contiguous()
        self.reset()

    def reset(self):
        self.prev_seg = torch.full((self.B, H, W), -1.0, device="cuda")
        self.prev_track = torch.full((self.B, self.Q), -1, dtype=torch.int32, device="cuda")
        self.next_track = torch.zeros((self.B,), dtype=torch.int32, device="cuda")

    def step(self, seg):
        counts = overlay.label_contingency(seg, self.prev_seg, self.Q, self.Q)
        matched, _, _ = overlay.greedy_iou_match(counts, self.ids, self.ids, H * W, IOU)
        track = overlay.track_assign(counts, matched, self.prev_track, self.next_track)
        self.prev_seg, self.prev_track = seg.clone(), track.clone()
        return track


class CheckerTracks:
    """The same on the host, from the maps the segmenter returned."""

    def __init__(self, B, Q):
        self.B, self.Q = B, Q
        self.reset()

    def reset(self):
        self.prev_seg = np.full((self.B, H, W), -1, np.float32)
        self.prev_track = np.full((self.B, self.Q), -1, np.int32)
        self.next_track = np.zeros((self.B,), np.int32)

    def step(self, seg):
        track, self.next_track = match_ref.track_step(seg, self.prev_seg, self.prev_track, self.next_track, self.Q, IOU)
        self.prev_seg, self.prev_track = seg.copy(), track
        return track


class _Untracked:
    """A StreamResult whose segments() leaves the "track_id" entries out: what the eager path returns."""

    def __init__(self, res):
        self._res = res
        self.segmentation, self.topk_idx, self.seg_id, self.scores = res.segmentation, res.topk_idx, res.seg_id, res.scores

    def segments(self):
        return [{"segmentation": r["segmentation"],
                 "segments_info": [{k: v for k, v in s.items() if k != "track_id"} for s in r["segments_info"]]}
                for r in self._res.segments()]


def _run_sequence(model, frames, dtype, batches, alpha):
    """frames A, B, A, reset_tracks(), A, A over ``batches`` (tuples of frame indices per step)."""
    B = len(batches[0])
    seg = StreamingSegmenter(model, H, W, B=B, threshold=THR, dtype=dtype, track=dict(iou_threshold=IOU),
                             overlay=dict(alpha=alpha, palette=PALETTE, color_by="track"))
    Q = seg.Q
    eager, checker = EagerTracks(B, Q), CheckerTracks(B, Q)
    wants, tracks, n_tracked = {}, [], 0
    for step, idx in enumerate(batches):
        if step == 3:
            seg.reset_tracks()
            eager.reset()
            checker.reset()
        depth = torch.stack([frames[i][0] for i in idx])
        rgb = torch.stack([frames[i][1] for i in idx])
        if idx not in wants:
            wants[idx] = _eager(model, depth, rgb, dtype)
        res = seg(depth, rgb)
        what = f"step {step} frames {idx}"
        _assert_same(_Untracked(res), wants[idx], what)         # map, tables, scores, segments_info
        want_t = eager.step(wants[idx][0])
        assert res.track_id.dtype == torch.int32 and torch.equal(res.track_id, want_t), f"{what}: track_id (eager)"
        seg_h = res.segmentation.cpu().numpy()
        chk_t = checker.step(seg_h)
        assert np.array_equal(res.track_id.cpu().numpy(), chk_t), f"{what}: track_id (checker)"
        lut = match_ref.track_lut(chk_t, np.array(PALETTE, np.uint8))
        assert np.array_equal(res.overlay.cpu().numpy(), overlay_ref.blend(rgb.cpu().numpy(), seg_h, lut, alpha)), \
            f"{what}: overlay"
        for b, r in enumerate(res.segments()):
            for s in r["segments_info"]:
                assert s["track_id"] == int(chk_t[b, s["id"]])
        # a track exactly where the map holds pixels of the id
        present = np.stack([np.isin(np.arange(Q), seg_h[b]) for b in range(B)])
        assert np.array_equal(chk_t >= 0, present), what
        n_tracked += int(present.sum())
        tracks.append(chk_t)
    assert seg.width <= 2 and seg._host.shape[0] == 4
    assert n_tracked > 0, "no frame kept a segment: nothing was tracked"
    # after the reset the first frame's segments count from 0 in id order, as on the very first frame
    assert np.array_equal(tracks[3], tracks[0])
    for b in range(B):
        got = tracks[3][b][tracks[3][b] >= 0]
        assert got.tolist() == list(range(len(got)))
    assert np.array_equal(tracks[4], tracks[3])   # the same frame again: every segment keeps its track
    return seg


@pytest.mark.timeout(300)
def test_tracks_float32(model, frames):
    _run_sequence(model, frames, torch.float32, [(0,), (1,), (0,), (0,), (0,)], 0.6)


@pytest.mark.timeout(300)
def test_tracks_batch_of_two_bf16(model, frames):
    _run_sequence(model, frames, torch.bfloat16, [(0, 1), (2, 0), (0, 1), (0, 1), (0, 1)], 0.37)


@pytest.mark.timeout(300)
def test_without_track_nothing_changes(model, frames):
    """No ``track=``: the segmenter of the parent commit — three table rows, no tracking state, the
    eager path's bits."""
    depth, rgb = frames[0]
    seg = StreamingSegmenter(model, H, W, B=1, threshold=THR, dtype=torch.float32,
                             overlay=dict(alpha=0.6, palette=PALETTE, color_by="id"))
    res = seg(depth[None], rgb[None])
    _assert_same(res, _eager(model, depth[None], rgb[None], torch.float32), "no tracking")
    assert res.track_id is None and seg._host.shape[0] == 3 and not hasattr(seg, "_prev_seg") and seg.width <= 2
    assert all("track_id" not in s for r in res.segments() for s in r["segments_info"])
    seg.reset_tracks()  # harmless


def test_options_are_checked(model):
    with pytest.raises(ValueError, match="needs track"):
        StreamingSegmenter(model, H, W, overlay=dict(color_by="track"))
    with pytest.raises(ValueError, match="unknown keys"):
        StreamingSegmenter(model, H, W, track=dict(threshold=0.5))
    with pytest.raises(ValueError, match="2\\^21 pixels"):
        StreamingSegmenter(model, 2048, 2048, track={})
