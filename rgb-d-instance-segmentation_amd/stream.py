"""C5 (BASELINE configs[4]): RealSense-style streaming inference of the hot path, one frame (or
a small fixed batch) at a time, replayed from a HIP graph.

At 1280x720, B=1 the kernels of one frame take about 1 ms, and issuing the ~40 launches of the
path from Python (ctypes + torch allocator) costs a comparable amount of host time.  The whole
inference path — u8 frames -> 10-channel pixel_values + DGGM planes (K1) -> ratio predictor
eval (K4) -> decomposition (K3) -> DSAM x3 cascade (K5) -> DGGM + final sum (K2) — is captured
once per shape into a graph (torch.cuda.CUDAGraph over hipGraph) and replayed per frame from
static device buffers, so the per-frame host cost is one graph launch.

Reference path per frame: CustomMask2FormerPixelLevelModule.forward (custom_model.py:324-355)
in eval mode, with the dataloader's 10-channel assembly (dataloader.py:386-425) moved on-device.
The Swin colour features are inputs (``colors``), as in the module (they come from the encoder,
outside the hot path).
"""
import contextlib
import ctypes
import logging

import torch

from . import _lib, data, export, ops, overlay as overlay_ops
from .graph_guard import check_and_instantiate
from .hot_path import hot_path, prepare

export_log = logging.getLogger(export.__name__)  # to_json warns where prediction_to_json warns


class StreamingHotPath:
    def __init__(self, ratio_predictor, dsams, dggm, H, W, B=1, dtype=torch.bfloat16, device="cuda",
                 color_channels=(96, 192, 384, 768), interface_dtype=None):
        self.rp, self.dsams, self.dg = ratio_predictor, list(dsams), dggm
        self.dtype = dtype
        self.interface_dtype = interface_dtype  # hot_path.float32_interface; the static colour buffers follow it
        for m in [self.rp, self.dg] + self.dsams:
            m.compute_dtype = dtype
            m.eval()
        dev = torch.device(device)
        self.depth_u8 = torch.zeros((B, H, W), dtype=torch.uint8, device=dev)
        self.rgb_u8 = torch.zeros((B, H, W, 3), dtype=torch.uint8, device=dev)
        h, w = -(-H // 4), -(-W // 4)
        self.colors = []
        for c in color_channels:
            self.colors.append(torch.zeros((B, c, h, w), dtype=interface_dtype or dtype, device=dev))
            h, w = -(-h // 2), -(-w // 2)
        self.graph = None
        self.outs = None

    def _run(self):
        pv = ops.assemble_pixel_values(self.depth_u8, self.rgb_u8)
        prep = prepare(pv, self.colors, self.dtype, dsam_modules=self.dsams,  # beside the ratio predictor
                       interface_dtype=self.interface_dtype)
        ratio = self.rp(pv[:, 3:6])
        return hot_path(pv, ratio, self.colors, self.dsams, self.dg, dtype=self.dtype, prepared=prep,
                        interface_dtype=self.interface_dtype), ratio

    def capture(self):
        """Warm up (packs weights, sizes workspaces) on a side stream, then capture the path."""
        with torch.no_grad():
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(2):
                    self._run()
            torch.cuda.current_stream().wait_stream(s)
            self.graph = torch.cuda.CUDAGraph(keep_graph=True)
            with torch.cuda.graph(self.graph):
                self.outs = self._run()
            self.width = check_and_instantiate(self.graph, "StreamingHotPath")
        return self

    def __call__(self, depth_u8=None, rgb_u8=None, colors=None):
        """Copy the frame (if given) into the static buffers and replay.  Returns the 4 backbone
        features and the ratio, as static tensors overwritten by the next call."""
        if self.graph is None:
            self.capture()
        if depth_u8 is not None:
            self.depth_u8.copy_(depth_u8, non_blocking=True)
        if rgb_u8 is not None:
            self.rgb_u8.copy_(rgb_u8, non_blocking=True)
        if colors is not None:
            for dst, src in zip(self.colors, colors):
                dst.copy_(src, non_blocking=True)
        self.graph.replay()
        return self.outs


class StreamResult:
    """What one ``StreamingSegmenter`` call returns.  The tensors are the segmenter's static
    device buffers — valid once the stream reaches them, overwritten by the next call:

      segmentation  float32 [B,H,W]   segment id per pixel at frame resolution, -1 = none
      overlay       uint8 [B,H,W,3]   the frame with every kept segment painted (None without ``overlay=``)
      seg_id, topk_idx  int32 [B,Q]   the tables of rgbd_pp_instance
      scores        float32 [B,Q]
      track_id      int32 [B,Q]       by segment id: the track the segment belongs to, -1 for an id
                                      without pixels (None without ``track=``)

    ``segments()`` is the only host wait (``to_json()``, with ``encode=True``, waits on the same event)."""

    def __init__(self, owner, event):
        self._owner, self._event = owner, event
        self.segmentation = owner.segmentation
        self.overlay = owner.overlay_u8
        self.seg_id, self.topk_idx, self.scores = owner.seg_id, owner.topk_idx, owner.scores
        self.track_id = owner.track_id

    def segments(self):
        """Wait for this call's replay, raise the reference's ValueError for a frame whose depth
        range the decomposition rejected, and return what
        ``postprocess.post_process_instance_segmentation(..., keep_on_device=True)`` returns: per
        image ``{"segmentation": float32 [H,W] on the device, "segments_info": [...]}``, read
        from the pinned copy of the tables the replay made.  With ``track=`` every entry also
        holds ``"track_id"``."""
        o = self._owner
        self._event.synchronize()
        for st in o._statuses:
            st.check()
        topk_h, sid_h = o._host[0].tolist(), o._host[1].tolist()
        ps_h = o._host[2].view(torch.float32).tolist()
        results = []
        track_h = o._host[3].tolist() if o.track_cfg is not None else None
        for i in range(o.B):
            segments = [{"id": sid_h[i][j], "label_id": topk_h[i][j] % o.num_labels, "was_fused": False,
                         "score": round(ps_h[i][j], 6)}
                        for j in range(o.Q) if sid_h[i][j] >= 0]
            if track_h is not None:
                for seg in segments:
                    seg["track_id"] = track_h[i][seg["id"]]
            results.append({"segmentation": o.segmentation[i], "segments_info": segments})
        return results

    def to_json(self, original_size=None):
        """Per image exactly what ``export.prediction_to_json(self.segments()[i], original_size)``
        returns — ``{"labels", "scores", "bboxes", "masks"}``, and with ``track=`` a ``"track_ids"``
        list alongside ``labels`` — from the strings, boxes and areas the replay itself encoded
        (``StreamingSegmenter(encode=True)``; csrc/rle_encode.hip).  Waits on the event
        ``segments()`` waits on, reads the per-mask block from its pinned copy and then exactly the
        characters.  ``original_size``: one (h, w) written as every mask's ``size``."""
        o = self._owner
        if o._enc is None:
            raise RuntimeError("to_json needs StreamingSegmenter(encode=True)")
        results = self.segments()
        head = o._enc["host"].numpy()
        N = o.B * o.Q
        offsets, info = head[4:5 + N], head[5 + N:].reshape(N, 8)
        if info[:, 7].any():  # the buffers hold the bound no frame exceeds
            raise RuntimeError(f"StreamingSegmenter: the encoder's buffers overflowed (status {info[:, 7].max()})")
        text = o._enc["chars"][:int(offsets[-1])].cpu().numpy().tobytes().decode("ascii")
        h, w = (int(original_size[0]), int(original_size[1])) if original_size is not None else (o.H, o.W)
        sid_h = o._host[1].tolist()
        out = []
        for i, res in enumerate(results):
            slot = {sid: j for j, sid in enumerate(sid_h[i]) if sid >= 0}
            data = {"labels": [], "scores": [], "bboxes": [], "masks": []}
            if o.track_cfg is not None:
                data["track_ids"] = []
            for s in res["segments_info"]:
                m = i * o.Q + slot[s["id"]]
                _, _, area, x0, y0, x1, y1, _ = (int(v) for v in info[m])
                if area == 0:
                    export_log.warning("instance id %s has an empty mask: skipped", s["id"])
                    continue
                data["labels"].append(int(s["label_id"]))
                data["scores"].append(float(s.get("score", 1.0)))
                data["bboxes"].append([float(x0), float(y0), float(x1 - x0 + 1), float(y1 - y0 + 1)])
                data["masks"].append({"size": [h, w], "counts": text[offsets[m]:offsets[m + 1]]})
                if o.track_cfg is not None:
                    data["track_ids"].append(s["track_id"])
            out.append(data)
        return out


class StreamingSegmenter:
    """C5 end to end: u8 frames in, instance map, segment tables and blended overlay out, one
    graph replay per call.

    The captured path, in order: K1 assembly (``data.map_10channel``; with ``size=(S, S)`` the
    frames are resized to the model size on the device first, non-square sizes are refused as
    there) -> the whole drop-in model in eval mode under no_grad (``set_compute_dtype(dtype,
    interface_dtype)``; bf16 runs under the bf16 autocast of the whole-model benchmark) ->
    ``rgbd_pp_instance`` at the frame's (H, W), the target size ``process_prediction`` asks for ->
    with ``track=dict(iou_threshold=0.5)`` the tracking stage (below) -> with
    ``overlay=dict(alpha=0.6, palette=[(r, g, b), ...], color_by="label" | "id" | "track")`` the
    colour table and the blend (csrc/overlay.hip) -> the copy of the tables to one pinned host
    block.  Between the frame copy and the event ``StreamResult.segments()`` waits on, nothing
    touches the host.

    Segment ids are positions among the kept queries of one frame.  ``track=`` gives every segment
    an id that is stable from frame to frame (csrc/segment_match.hip): the
    contingency table of this frame's map against the previous frame's, the greedy IoU match of
    the Q x Q segments, the assignment — a matched segment inherits its predecessor's track, the
    other non-empty ones take fresh numbers in ascending id order — and the copy of map and track
    table into the "previous" buffers, all in the captured path and on its stream.  The state
    (previous map, its tracks, the next free number per image) lives on the device;
    ``reset_tracks()`` forgets it.  ``overlay=dict(color_by="track")`` colours a segment by
    ``palette[track % n_colors]``.  A track that is absent for a frame is not found again.

    ``encode=True`` records the stream: ``rgbd_rle_encode_labels`` (csrc/rle_encode.hip, DESIGN.md
    §5.21) runs in the captured path after ``rgbd_pp_instance`` (and the tracking stage) on the
    float32 map with the device ``seg_id`` table as its ids, into static buffers sized by
    ``rgbd_rle_encode_capacity`` — the bound no frame exceeds — and its per-mask block rides to a
    pinned block of its own beside the tables; ``StreamResult.to_json()`` returns the reference's
    per-image JSON from them.  Without it nothing of this exists: no buffer, no launch.

    ``model``: a CustomMask2FormerForUniversalSegmentation of version 0.4.0 on the GPU (put into
    eval mode here)."""

    def __init__(self, model, H, W, B=1, size=None, threshold=0.5, dtype=torch.bfloat16, interface_dtype=None,
                 overlay=None, track=None, encode=False):
        plm = model.model.pixel_level_module
        if getattr(plm, "version", None) != "0.4.0":
            raise ValueError("StreamingSegmenter runs the paper model (version 0.4.0), not "
                             f"{getattr(plm, 'version', None)!r}")
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("rgbd_amd ops run on the GPU only (no CPU fallback); move the model to the GPU")
        if size is not None:
            size = (int(size[0]), int(size[1]))
            if size[0] != size[1] and size != (H, W):
                raise ValueError(f"size {size}: non-square model sizes are refused, as data.resize_frames refuses "
                                 "them (the reference transposes their gradient planes, SURVEY Q18)")
        self.model, self.size, self.threshold = model.eval(), size, float(threshold)
        self.dtype, self.interface_dtype = dtype, interface_dtype
        self.B, self.H, self.W = B, H, W
        self.Q, self.num_labels = int(model.config.num_queries), int(model.config.num_labels)
        self.depth_u8 = torch.zeros((B, H, W), dtype=torch.uint8, device=dev)
        self.rgb_u8 = torch.zeros((B, H, W, 3), dtype=torch.uint8, device=dev)
        self.segmentation = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        self.track_cfg = None
        if track is not None:
            cfg = dict(iou_threshold=0.5)
            unknown = set(track) - set(cfg)
            if unknown:
                raise ValueError(f"track: unknown keys {sorted(unknown)} (iou_threshold)")
            cfg.update(track)
            if self.Q > overlay_ops.MAX_MATCH_IDS or H * W > 1 << 21:
                raise ValueError(f"track: at most {overlay_ops.MAX_MATCH_IDS} queries and 2^21 pixels per frame, got "
                                 f"{self.Q} and {H * W}")
            self.track_cfg = cfg
        rows = 3 if self.track_cfg is None else 4  # the track table rides in the same pinned block
        self._tables = torch.zeros((rows, B, self.Q), dtype=torch.int32, device=dev)
        self.topk_idx, self.seg_id = self._tables[0], self._tables[1]
        self.scores = self._tables[2].view(torch.float32)
        self._host = torch.empty((rows, B, self.Q), dtype=torch.int32, pin_memory=True)
        self.track_id = None
        if self.track_cfg is not None:
            Q = self.Q
            self.track_id = self._tables[3]
            self._prev_seg = torch.full((B, H, W), -1.0, dtype=torch.float32, device=dev)
            self._prev_track = torch.full((B, Q), -1, dtype=torch.int32, device=dev)
            self._next_track = torch.zeros((B,), dtype=torch.int32, device=dev)
            self._counts = torch.empty((B, Q + 1, Q + 1), dtype=torch.int32, device=dev)
            self._ids = torch.arange(Q, dtype=torch.int32, device=dev).repeat(B, 1).contiguous()
            self._match = (torch.empty((B, Q), dtype=torch.int32, device=dev),
                           torch.empty((B, Q), dtype=torch.int32, device=dev),
                           torch.empty((B, 2), dtype=torch.int32, device=dev))
        self.overlay_cfg = None
        self.overlay_u8 = self._lut = self._palette = None
        if overlay is not None:
            cfg = dict(alpha=0.6, palette=None, color_by="label")
            unknown = set(overlay) - set(cfg)
            if unknown:
                raise ValueError(f"overlay: unknown keys {sorted(unknown)} (alpha, palette, color_by)")
            cfg.update(overlay)
            if cfg["color_by"] not in ("label", "id", "track"):
                raise ValueError(f"overlay color_by {cfg['color_by']!r}: 'label', 'id' or 'track' expected")
            if cfg["color_by"] == "track" and self.track_cfg is None:
                raise ValueError("overlay color_by 'track' needs track=dict(...)")
            if cfg["palette"] is None:
                cfg["palette"] = overlay_ops.consistent_colors(max(self.num_labels, self.Q))
            self.overlay_cfg = cfg
            self._palette = overlay_ops._palette(cfg["palette"], dev)
            self._lut = torch.empty((B, self.Q), dtype=torch.int32, device=dev)
            self.overlay_u8 = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
        self._enc = None
        if encode:
            N = B * self.Q
            if self.Q > export.MAX_IDS or N > export.MAX_DEVICE_MASKS or H * W >= 2 ** 31:
                raise ValueError(f"encode: at most {export.MAX_IDS} queries, {export.MAX_DEVICE_MASKS} masks and 2^31 - 1 "
                                 f"pixels per frame, got {self.Q}, {N} and {H * W}")
            cap_counts, cap_chars = export._capacity(0, B, N, H, W)  # segment ids are distinct within a frame
            cap_chars = min(cap_chars, 2 ** 31 - 1)
            head = torch.zeros((4 + N + 1 + 8 * N,), dtype=torch.int32, device=dev)  # totals | offsets | info
            ws_bytes = _lib.lib().rgbd_rle_encode_workspace_size(0, B, N, H, W, cap_counts)
            self._enc = dict(cap_counts=cap_counts, cap_chars=cap_chars, head=head,
                             chars=torch.zeros((cap_chars,), dtype=torch.uint8, device=dev),
                             ws=torch.empty((ws_bytes,), dtype=torch.uint8, device=dev),
                             host=torch.empty((head.numel(),), dtype=torch.int32, pin_memory=True))
        self._th, self._tw = (ctypes.c_int * B)(*[H] * B), (ctypes.c_int * B)(*[W] * B)
        self._seg_ptrs = (ctypes.c_void_p * B)(*[self.segmentation[b].data_ptr() for b in range(B)])
        self._statuses = ()
        self.graph = None
        self.width = None

    def _run(self):
        self.model.set_compute_dtype(self.dtype, self.interface_dtype)
        pv = data.map_10channel(self.rgb_u8, self.depth_u8, size=self.size)["pixel_values"]
        amp = torch.autocast("cuda", dtype=torch.bfloat16) if self.dtype == torch.bfloat16 else contextlib.nullcontext()
        with amp:
            out = self.model(pixel_values=pv)
        cls = out.class_queries_logits.to(torch.float32).contiguous()
        masks = out.masks_queries_logits.to(torch.float32).contiguous()
        B, Q, C1 = cls.shape
        if (B, Q, C1 - 1) != (self.B, self.Q, self.num_labels):
            raise RuntimeError(f"StreamingSegmenter: the model returned {tuple(cls.shape)} class logits")
        dev = cls.device
        L = _lib.lib()
        st = ops._stream(dev)
        ws = ops._workspace(dev, L.rgbd_pp_instance_workspace_size(B, Q), "postprocess")
        _lib.check(L.rgbd_pp_instance(ops._p(cls), ops._p(masks), B, Q, C1, masks.shape[-2], masks.shape[-1], self._th,
                                      self._tw, ctypes.c_double(self.threshold), self._seg_ptrs, ops._p(self.topk_idx),
                                      ops._p(self.scores), ops._p(self.seg_id), ops._p(ws), st), "rgbd_pp_instance")
        if self.track_cfg is not None:
            overlay_ops.label_contingency(self.segmentation, self._prev_seg, Q, Q, out=self._counts)
            overlay_ops.greedy_iou_match(self._counts, self._ids, self._ids, self.H * self.W,
                                         self.track_cfg["iou_threshold"], out=self._match)
            overlay_ops.track_assign(self._counts, self._match[0], self._prev_track, self._next_track,
                                     out=self.track_id)
            self._prev_seg.copy_(self.segmentation)
            self._prev_track.copy_(self.track_id)
        if self._enc is not None:
            e, N = self._enc, B * Q
            head = e["head"]
            _lib.check(L.rgbd_rle_encode_labels(_lib.RGBD_F32, ops._p(self.segmentation), B, self.H, self.W, Q,
                                                ops._p(self.seg_id), Q, e["cap_counts"], e["cap_chars"],
                                                ops._p(e["chars"]), ops._p(head[4:5 + N]), ops._p(head[5 + N:]),
                                                ops._p(head[:4]), ops._p(e["ws"]), st), "rgbd_rle_encode_labels")
        if self.overlay_cfg is not None and self.overlay_cfg["color_by"] == "track":
            overlay_ops.track_lut(self.track_id, self._palette, out=self._lut)
        elif self.overlay_cfg is not None:
            overlay_ops.build_lut(self.seg_id, self.topk_idx, self.num_labels, self._palette,
                                  self.overlay_cfg["color_by"], out=self._lut)
        if self.overlay_cfg is not None:
            overlay_ops.blend(self.rgb_u8, self.segmentation, self._lut, self.overlay_cfg["alpha"], out=self.overlay_u8)
        self._host.copy_(self._tables, non_blocking=True)
        if self._enc is not None:
            self._enc["host"].copy_(self._enc["head"], non_blocking=True)

    def capture(self):
        """Two eager warm-up runs on a side stream (weight packs, workspaces, device constants),
        then the capture on that stream; at most two concurrent branches (graph_guard)."""
        plm = self.model.model.pixel_level_module
        with torch.no_grad():
            self.stream = torch.cuda.Stream()
            self.stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self.stream):
                for _ in range(2):
                    self._run()
            torch.cuda.current_stream().wait_stream(self.stream)
            graph = torch.cuda.CUDAGraph(keep_graph=True)
            # thread_local, as train_graph.CapturedTrainStep: a process group's watchdog thread may
            # query events while this capture is open
            with torch.cuda.graph(graph, stream=self.stream, capture_error_mode="thread_local"):
                self._run()
            # this capture's statuses: another capture of the same model replaces the module's list
            self._statuses = tuple(getattr(plm, "captured_statuses", ()))
            self.width = check_and_instantiate(graph, "StreamingSegmenter")
            self.graph = graph
        self.reset_tracks()  # the warm-up runs tracked their own frames
        return self

    def reset_tracks(self):
        """Forget the previous frame: the next frame's segments get tracks 0, 1, ... in id order.
        (Queued on the current stream, like the frame copies of a call.)"""
        if self.track_cfg is not None:
            self._prev_seg.fill_(-1.0)
            self._prev_track.fill_(-1)
            self._next_track.zero_()

    def __call__(self, depth_u8=None, rgb_u8=None):
        """Copy the frame (if given: uint8 [B,H,W] / [B,H,W,3], host or device) into the static
        buffers without blocking, replay, record the event.  -> StreamResult."""
        if self.graph is None:
            self.capture()
        if depth_u8 is not None:
            self.depth_u8.copy_(depth_u8, non_blocking=True)
        if rgb_u8 is not None:
            self.rgb_u8.copy_(rgb_u8, non_blocking=True)
        self.graph.replay()
        event = torch.cuda.Event()
        event.record(torch.cuda.current_stream(self.depth_u8.device))
        return StreamResult(self, event)
