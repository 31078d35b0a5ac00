"""f7: the reference's per-image JSON results read back on the device (csrc/rle_decode.hip,
DESIGN §5.20), and its multi-model comparison against one ground truth.

``export`` writes ``{"labels", "scores", "bboxes", "masks": [{"size": [h, w], "counts": <compressed
COCO RLE string>}]}`` per image; the reference's comparison tool works from those files alone
(mask2former/predictor.py:747-1065 ``visualize_multi_model_json_results`` ->
``_create_and_save_multi_model_json_comparison`` -> ``_load_json_prediction_data``) and decodes
every mask with pycocotools on the host.  Here the count strings of all masks of all files go to
the device in one copy; ``rgbd_rle_paint`` decodes them (maskApi.c ``rleFrString``) and paints the
instance-id map — mask i gets id i + 1, later masks over earlier ones, a mask with no set pixel
left out, a mask of another size than the image taken through Pillow's NEAREST resize — and one
small copy brings the per-mask flags back for ``segments_info``.

``load_json_prediction`` returns ``None`` exactly where the reference does: a missing key among
masks / labels / scores, an empty mask list, no surviving segment, and (Q20) a first
mask whose ``size`` differs from ``image_shape`` — the reference's map takes the first mask's size
while every mask ends at ``image_shape``, so each assignment raises inside its ``try`` and is
skipped.  The resize therefore only ever shows for a later mask of a file whose first mask
matches the image.

Deliberate departures, each a ``ValueError`` naming the file and the mask index where the
reference swallows an exception or reads past the end of a C buffer:
  * a mask whose ``counts`` is not a string of ASCII characters (or that lacks ``size`` / ``counts``);
  * a mask that takes part whose string is malformed: a negative count, counts that do not sum
    to h w, or a truncated last group (the status of ``rgbd_rle_counts``);
  * more than 255 masks in one file (ids stay within ``overlay.MAX_MATCH_IDS``).
"""
import ctypes
import json
import os

import numpy as np
import torch

from . import _lib, overlay
from ._lib import check
from .ops import _need_cuda, _p, _stream, _workspace

MAX_MASKS = overlay.MAX_MATCH_IDS - 1
_STATUS = {1: "a negative count", 2: "the counts do not sum to h * w", 4: "a truncated or over-long group"}


def _status_text(st):
    return ", ".join(t for bit, t in _STATUS.items() if st & bit)


def _device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("rgbd_amd ops run on the GPU only (no CPU fallback); got device %r" % (device,))
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _mask_fields(rle, where):
    """(count string as bytes, h, w) of one RLE dict, or ValueError naming ``where``."""
    if not isinstance(rle, dict) or "size" not in rle or "counts" not in rle:
        raise ValueError(f"{where}: a dict with 'size' and 'counts' expected")
    counts = rle["counts"]
    if not isinstance(counts, str):
        raise ValueError(f"{where}: 'counts' must be a compressed RLE string, got {type(counts).__name__}")
    try:
        raw = counts.encode("ascii")
        h, w = (int(v) for v in rle["size"])
    except (UnicodeEncodeError, TypeError, ValueError) as e:
        raise ValueError(f"{where}: {e}") from None
    if h <= 0 or w <= 0 or h * w >= 2 ** 31:
        raise ValueError(f"{where}: size {rle['size']} is not a positive [h, w] below 2^31 pixels")
    return raw, h, w


class _Packed:
    """The device input of the rgbd_rle_* calls for ``files`` = lists of (bytes, h, w, take)."""

    def __init__(self, files, H, W, dev):
        masks = [m for f in files for m in f]
        self.N, self.B, self.H, self.W = len(masks), len(files), int(H), int(W)
        N, B = self.N, self.B
        lens = [len(m[0]) for m in masks]
        meta = np.empty(6 * N + B + 2, np.int32)
        offsets = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])
        if offsets[-1] >= 2 ** 31:
            raise ValueError("the count strings of one call must stay below 2^31 characters")
        meta[:N + 1] = offsets
        meta[N + 1:3 * N + 1] = np.array([[m[1], m[2]] for m in masks], np.int32).reshape(-1)
        meta[3 * N + 1:4 * N + 1] = [int(m[3]) for m in masks]
        resized = [i for i, m in enumerate(masks) if (m[1], m[2]) != (self.H, self.W)]
        slot = np.full(N, -1, np.int32)
        slot[resized] = np.arange(len(resized), dtype=np.int32)
        meta[4 * N + 1:5 * N + 1] = slot
        meta[5 * N + 1:6 * N + 1] = -1
        meta[5 * N + 1:5 * N + 1 + len(resized)] = resized
        meta[6 * N + 1:] = np.concatenate([[0], np.cumsum([len(f) for f in files])])
        self.n_chars, self.n_resized = int(offsets[-1]), len(resized)
        self.meta_host = meta
        # one upload: the meta words, then the characters (4-byte aligned behind them)
        blob = np.concatenate([meta.view(np.uint8), np.frombuffer(b"".join(m[0] for m in masks), np.uint8),
                               np.zeros(1, np.uint8)])
        blob_d = torch.from_numpy(blob).to(dev)
        self.meta_dev = blob_d[:meta.nbytes]
        self.chars = blob_d[meta.nbytes:]
        self.info = torch.empty((N, 4), dtype=torch.int32, device=dev)
        self.dev = dev

    def _mh(self):
        return self.meta_host.ctypes.data_as(ctypes.c_void_p)

    def workspace(self, tag):
        size = _lib.lib().rgbd_rle_workspace_size(self.N, self.n_chars, self.n_resized, self.H, self.W)
        return _workspace(self.dev, size, tag)

    def counts(self):
        ends = torch.empty((max(self.n_chars, 1),), dtype=torch.int32, device=self.dev)
        check(_lib.lib().rgbd_rle_counts(_p(self.chars), self._mh(), _p(self.meta_dev), self.N, self.B, self.H, self.W,
                                         _p(ends), _p(self.info), _stream(self.dev)), "rgbd_rle_counts")
        return ends

    def paint(self):
        out = torch.empty((self.B, self.H, self.W), dtype=torch.int32, device=self.dev)
        ws = self.workspace("rle_paint")
        check(_lib.lib().rgbd_rle_paint(_p(self.chars), self._mh(), _p(self.meta_dev), self.N, self.B, self.H, self.W,
                                        _p(out), _p(self.info), _p(ws), _stream(self.dev)), "rgbd_rle_paint")
        return out

    def stack(self):
        out = torch.empty((self.N, self.H, self.W), dtype=torch.uint8, device=self.dev)
        ws = self.workspace("rle_stack")
        check(_lib.lib().rgbd_rle_stack(_p(self.chars), self._mh(), _p(self.meta_dev), self.N, self.H, self.W,
                                        _p(out), _p(self.info), _p(ws), _stream(self.dev)), "rgbd_rle_stack")
        return out


def rle_counts(rles, device="cuda"):
    """maskApi.c ``rleFrString`` on the device: a list of ``{"size", "counts": str}`` -> per mask
    ``(counts list, status)`` (status 0 = well formed; the bits of rgbd_rle_counts otherwise)."""
    dev = _device(device)
    if not rles:
        return []
    fields = [_mask_fields(r, f"mask {i}") + (1,) for i, r in enumerate(rles)]
    pk = _Packed([fields], fields[0][1], fields[0][2], dev)
    ends = pk.counts()
    host = torch.cat([pk.info.reshape(-1), ends]).cpu().numpy()
    info, e = host[:4 * pk.N].reshape(pk.N, 4), host[4 * pk.N:].view(np.uint32).astype(np.int64)
    out = []
    for i in range(pk.N):
        o = int(pk.meta_host[i])
        ee = e[o:o + int(info[i, 0])]
        out.append((np.diff(ee, prepend=0).tolist(), int(info[i, 1])))
    return out


def decode_masks(rles, device="cuda"):
    """``pycocotools.mask.decode`` on the device: a list of ``{"size": [h, w], "counts": str}``, all
    of one size -> ``torch.bool [N, h, w]``.  ValueError naming the index for a malformed string."""
    dev = _device(device)
    if not rles:
        return torch.zeros((0, 0, 0), dtype=torch.bool, device=dev)
    fields = [_mask_fields(r, f"mask {i}") + (1,) for i, r in enumerate(rles)]
    h, w = fields[0][1:3]
    for i, f in enumerate(fields):
        if f[1:3] != (h, w):
            raise ValueError(f"mask {i}: size {[f[1], f[2]]} differs from mask 0's {[h, w]}")
    pk = _Packed([fields], h, w, dev)
    out = pk.stack()
    status = pk.info.cpu().numpy()[:, 1]
    for i in np.nonzero(status)[0]:
        raise ValueError(f"mask {int(i)}: malformed RLE string ({_status_text(int(status[i]))})")
    return out.view(torch.bool)


def _read(src):
    """(parsed dict or None, a name for messages).  A file that cannot be read or parsed is the
    reference's ``None`` (it swallows the exception)."""
    if isinstance(src, dict):
        return src, "<dict>"
    name = os.fspath(src)
    try:
        with open(name, "r") as f:
            return json.load(f), name
    except (OSError, ValueError):
        return None, name


def _file_masks(data, name, image_shape):
    """The masks of one file that go to the device, [(bytes, h, w, take)], or None where the
    reference returns None before (or whatever) it decodes."""
    if not isinstance(data, dict) or not all(k in data for k in ("masks", "labels", "scores")):
        return None
    masks, n_lab = data["masks"], min(len(data["labels"]), len(data["scores"]))
    if not masks:
        return None
    if len(masks) > MAX_MASKS:
        raise ValueError(f"{name}: {len(masks)} masks; at most {MAX_MASKS} per file (mask {MAX_MASKS} would take an id "
                         f"past overlay.MAX_MATCH_IDS)")
    fields = [_mask_fields(m, f"{name}: mask {i}") + (int(i < n_lab),) for i, m in enumerate(masks)]
    if fields[0][1:3] != tuple(image_shape):  # Q20: the map takes the first mask's size; every assignment fails
        return None
    return fields


def load_json_predictions(srcs, image_shape, device="cuda"):
    """``_load_json_prediction_data`` for a batch of files (paths or parsed dicts) of one
    ``image_shape`` (H, W): one launch set for all files and one host read (the per-mask flags).
    -> per file ``None`` where the reference returns it, else the HF-format
    ``{"segmentation": int32 [H, W] device tensor (0 = background, mask i = id i + 1),
    "segments_info": [{"id", "label_id", "score"}]}`` that ``overlay.overlay_segments``,
    ``overlay.match_segments``, ``overlay.consistent_prediction_overlay`` and
    ``export.prediction_to_json`` take as is."""
    dev = _device(device)
    H, W = (int(v) for v in image_shape)
    if H <= 0 or W <= 0 or H * W >= 2 ** 31:
        raise ValueError(f"image_shape {tuple(image_shape)}: a positive (H, W) below 2^31 pixels expected")
    parsed = [_read(s) for s in srcs]
    files = [_file_masks(d, name, (H, W)) for d, name in parsed]
    live = [b for b, f in enumerate(files) if f is not None]
    out = [None] * len(files)
    if not live:
        return out
    pk = _Packed([files[b] for b in live], H, W, dev)
    maps = pk.paint()
    info = pk.info.cpu().numpy()  # the one host read
    row = 0
    for k, b in enumerate(live):
        data, name = parsed[b]
        segs = []
        for i, f in enumerate(files[b]):
            n_counts, status, has_set, _ = (int(v) for v in info[row])
            row += 1
            if not f[3]:
                continue
            if status:
                raise ValueError(f"{name}: mask {i}: malformed RLE string ({_status_text(status)})")
            if has_set:
                segs.append({"id": i + 1, "label_id": data["labels"][i], "score": data["scores"][i]})
        if segs:
            out[b] = {"segmentation": maps[k], "segments_info": segs}
    return out


def load_json_prediction(src, image_shape, device="cuda"):
    """``_load_json_prediction_data(json_file_path, image_shape)`` (predictor.py:974-1065) for one
    path or parsed dict; see ``load_json_predictions``."""
    return load_json_predictions([src], image_shape, device)[0]


def multi_model_comparison(image_u8, gt_json, model_jsons, alpha=0.6, iou_threshold=0.5, color_seed=42):
    """Steps 2-5 of ``_create_and_save_multi_model_json_comparison`` (predictor.py:864-908): the
    ground truth and every model's JSON (paths or parsed dicts) loaded in one batch at the image's
    size, the GT painted in ``overlay.consistent_colors(len(gt ids), color_seed)`` zipped onto its
    ids, and each model matched to the GT by IoU and painted in its GT instance's colour, red for
    a false positive.  image_u8: uint8 [H, W, 3] on the device.

    -> ``{"gt_overlay": uint8 [H, W, 3], "model_overlays": uint8 [M, H, W, 3], "gt": result or None,
    "models": [result or None], "gt_color_mapping": {id: (r, g, b)}}``, tensors on the device.
    The bare image stands where a load is ``None`` (a missing GT; a failed model), as in the
    reference.  One departure: with no GT but a model that loads, the reference falls back to
    colours drawn at random; this path draws none and returns the bare image for that model.
    Layout, titles and file writing are presentation and are not done here."""
    _need_cuda(image_u8)
    if image_u8.dtype != torch.uint8 or image_u8.dim() != 3 or image_u8.shape[2] != 3:
        raise ValueError("image_u8 must be uint8 [H, W, 3]")
    H, W = image_u8.shape[:2]
    model_jsons = list(model_jsons)
    loaded = load_json_predictions([gt_json] + model_jsons, (H, W), image_u8.device)
    gt, models = loaded[0], loaded[1:]
    mapping = {}
    gt_overlay = image_u8.clone()
    model_overlays = image_u8[None].repeat(len(models), 1, 1, 1)
    if gt is not None:
        ids = [s["id"] for s in gt["segments_info"]]
        mapping = dict(zip(ids, overlay.consistent_colors(len(ids), seed=color_seed)))
        gt_overlay = overlay.overlay_segments(image_u8, gt, mapping, alpha)
        hit = [k for k, m in enumerate(models) if m is not None]
        if hit:
            painted = overlay.consistent_prediction_overlay(
                image_u8[None].repeat(len(hit), 1, 1, 1), [models[k] for k in hit], mapping, [gt] * len(hit),
                alpha=alpha, iou_threshold=iou_threshold)
            for j, k in enumerate(hit):
                model_overlays[k] = painted[j]
    return {"gt_overlay": gt_overlay, "model_overlays": model_overlays, "gt": gt, "models": models,
            "gt_color_mapping": mapping}
