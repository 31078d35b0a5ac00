"""stream.StreamingSegmenter(encode=True): the COCO RLE strings, boxes and areas of every frame's
segments, encoded inside the captured graph (csrc/rle_encode.hip).  ``to_json()`` of every replay is
held to ``export.prediction_to_json`` on the torch path over ``segments()``, and the replay's
characters, offsets and per-mask block bitwise to the eager call on the returned map and table.
240x320, threshold 0.0."""
import pytest
import torch

from checkers import rle_encode_cases as rc
from rgbd_amd import export
from rgbd_amd.stream import StreamingSegmenter
from test_gpu_stream_segment import H, W, THR, PALETTE, frames, model  # noqa: F401

pytestmark = pytest.mark.gpu


def _torch_json(monkeypatch, segments, original_size):
    monkeypatch.setattr(export, "HIP_RLE_ENCODE", False)   # the parent's path
    want = [export.prediction_to_json(s, original_size) for s in segments]
    monkeypatch.undo()
    return want


def _assert_replay_is_eager(seg, res):
    B, Q = seg.B, seg.Q
    N = B * Q
    torch.cuda.synchronize()
    eager = rc.raw_encode(0, res.segmentation, res.seg_id.contiguous(), B, N, H, W, seg._enc["cap_counts"],
                          seg._enc["cap_chars"], n_ids=Q)
    head = seg._enc["head"]
    n = int(eager["offsets"][-1])
    assert torch.equal(head[4:5 + N], eager["offsets"]) and torch.equal(head[5 + N:].reshape(N, 8), eager["info"])
    assert torch.equal(head[:4].view(torch.int64), eager["totals"])
    assert torch.equal(seg._enc["chars"][:n], eager["chars"][:n])
    assert torch.equal(seg._enc["host"], head.cpu())
    return n


def _run(model, frames, monkeypatch, dtype, batches, **kw):
    B = len(batches[0])
    seg = StreamingSegmenter(model, H, W, B=B, threshold=THR, dtype=dtype, encode=True, **kw)
    n_masks = n_chars = 0
    for step, idx in enumerate(batches):
        res = seg(torch.stack([frames[i][0] for i in idx]), torch.stack([frames[i][1] for i in idx]))
        segments = res.segments()
        for original in (None, (2 * H, 2 * W + 1)):
            got = res.to_json(original)
            want = _torch_json(monkeypatch, segments, original)
            assert len(got) == B
            for g, w_, s in zip(got, want, segments):
                tracks = g.pop("track_ids", None)
                assert g == w_ and list(g) == list(w_), f"step {step} frames {idx}"
                if "track" in kw:
                    nonempty = [x for x in s["segments_info"] if bool((s["segmentation"] == x["id"]).any())]
                    assert tracks == [x["track_id"] for x in nonempty] and len(tracks) == len(g["labels"])
                else:
                    assert tracks is None
                n_masks += len(g["masks"])
        n_chars += _assert_replay_is_eager(seg, res)
    assert n_masks > 0 and n_chars > 0, "no frame kept a segment: nothing was encoded"
    assert seg.width <= 2
    return seg


@pytest.mark.timeout(300)
def test_to_json_float32(model, frames, monkeypatch):
    seg = _run(model, frames, monkeypatch, torch.float32, [(0,), (1,), (0,)])
    assert seg._host.shape[0] == 3


@pytest.mark.timeout(300)
def test_to_json_with_tracks_batch_of_two_bf16(model, frames, monkeypatch):
    seg = _run(model, frames, monkeypatch, torch.bfloat16, [(0, 1), (2, 0), (0, 1)], track=dict(iou_threshold=0.5),
               overlay=dict(alpha=0.6, palette=PALETTE, color_by="track"))
    assert seg._host.shape[0] == 4


def test_without_encode_nothing_changes(model):
    """No ``encode=``: no encoder buffer, the pinned block of the parent commit, and no to_json."""
    plain = StreamingSegmenter(model, H, W, B=2, threshold=THR)
    assert plain._enc is None and tuple(plain._host.shape) == (3, 2, plain.Q)
    tracked = StreamingSegmenter(model, H, W, B=1, threshold=THR, track={})
    assert tracked._enc is None and tuple(tracked._host.shape) == (4, 1, tracked.Q)
    enc = StreamingSegmenter(model, H, W, B=2, threshold=THR, encode=True)
    assert tuple(enc._host.shape) == (3, 2, enc.Q) and enc._enc["host"].is_pinned()
    assert enc._enc["host"].numel() == 4 + 2 * enc.Q + 1 + 8 * 2 * enc.Q
    assert (enc._enc["cap_counts"], enc._enc["cap_chars"]) == rc.capacity(0, 2, 2 * enc.Q, H, W)
    with pytest.raises(RuntimeError, match="encode=True"):
        from rgbd_amd.stream import StreamResult
        StreamResult(plain, torch.cuda.Event()).to_json()
