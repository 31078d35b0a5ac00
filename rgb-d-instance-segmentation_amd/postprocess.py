"""f4: instance post-processing on the device.

The reference turns its predictions into instance maps with the Hugging Face image processor on
the CPU (mask2former/predictor.py:697-700, process_prediction ->
Mask2FormerImageProcessor.post_process_instance_segmentation, transformers 5.15
image_processing_mask2former.py:627-744): per image a 100-query top-k over the class
probabilities, 100 bilinear 384x384 mask upsamplings, sigmoid mask scores, a nearest resize to
the original size and an ordered paint of the kept masks.  ``post_process_instance_segmentation``
does the same on the GPU (csrc/postprocess.hip, rgbd_pp_instance) with the reference's
arguments and return format; ``install`` swaps it into an image processor instance, so
``process_prediction`` runs unchanged.

Parity (tests/test_gpu_postprocess.py, against the HF processor on the CPU): the top-k indices
come out in CPU torch.topk(sorted=False)'s order (libstdc++ nth_element, restated and pinned in
oracle/postprocess.py), so segment ids, labels and the painted map are identical; pred scores
agree to float32 summation order (rtol 1e-5).  A pixel whose interpolated logit lies within a
few ulp of 0 could binarise differently (the CPU kernel's rounding is not reproduced bit for
bit); the fixtures check none does.

f4b: the processor's other two post-processors, ``post_process_semantic_segmentation`` and
``post_process_panoptic_segmentation`` (transformers 5.15 image_processing_pil_mask2former.py:587
and :788), on the GPU as well (csrc/postprocess_dense.hip, rgbd_pp_semantic / rgbd_pp_panoptic;
DESIGN §5.16); ``install(..., tasks=("instance", "semantic", "panoptic"))`` routes them.  Parity
(tests/test_gpu_postprocess_dense.py) is against float64: semantic scores within
2e-5 max(1, max|S|), maps identical wherever the float64 top-2 gap exceeds the float32 error bar,
segments_info identical.
"""
import ctypes
import numbers

import torch

from . import _lib
from ._lib import check
from .ops import _need_cuda, _p, _stream, _workspace

CHUNK = 64  # images per launch (bounds the device copy of the mask logits)


def _run(cls, masks, sizes, threshold):
    B, Q, C1 = cls.shape
    h, w = masks.shape[-2:]
    dev = cls.device
    segs = [torch.empty(s, dtype=torch.float32, device=dev) for s in sizes]
    topk = torch.empty((B, Q), dtype=torch.int32, device=dev)
    ps = torch.empty((B, Q), dtype=torch.float32, device=dev)
    sid = torch.empty((B, Q), dtype=torch.int32, device=dev)
    L = _lib.lib()
    ws = _workspace(dev, L.rgbd_pp_instance_workspace_size(B, Q), "postprocess")
    th = (ctypes.c_int * B)(*[s[0] for s in sizes])
    tw = (ctypes.c_int * B)(*[s[1] for s in sizes])
    sp = (ctypes.c_void_p * B)(*[t.data_ptr() for t in segs])
    check(L.rgbd_pp_instance(_p(cls), _p(masks), B, Q, C1, h, w, th, tw, ctypes.c_double(threshold), sp, _p(topk),
                             _p(ps), _p(sid), _p(ws), _stream(dev)), "rgbd_pp_instance")
    return segs, topk, ps, sid, ws


def _binary_maps(ws, B, Q, b, size, sid, n_kept, dev):
    """The kept masks of image b at its target size, stacked in segment-id order (float 0/1)."""
    out = torch.empty((n_kept, *size), dtype=torch.float32, device=dev)
    check(_lib.lib().rgbd_pp_binary_maps(_p(ws), B, Q, b, size[0], size[1], _p(sid), _p(out), _stream(dev)),
          "rgbd_pp_binary_maps")
    return out


def post_process_instance_segmentation(outputs, threshold: float = 0.5, mask_threshold: float = 0.5,
                                       overlap_mask_area_threshold: float = 0.8, target_sizes=None,
                                       return_coco_annotation: bool = False, return_binary_maps: bool = False,
                                       device=None, keep_on_device: bool = False):
    """Same arguments and results as the HF method (mask_threshold and
    overlap_mask_area_threshold are accepted and unused there too).  Inputs may be CPU tensors
    (the reference passes the predictions as numpy-backed CPU tensors); they are moved to
    ``device`` (default: the current GPU).  Segmentation maps come back as CPU float32 tensors
    like the reference's, or stay on the GPU with ``keep_on_device``."""
    if return_coco_annotation and return_binary_maps:
        raise ValueError("return_coco_annotation and return_binary_maps can not be both set to True.")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    cls_all = outputs.class_queries_logits
    masks_all = outputs.masks_queries_logits
    B = cls_all.shape[0]
    if target_sizes is not None and len(target_sizes) != B:
        raise ValueError("Make sure that you pass in as many target sizes as the batch dimension of the logits")
    results = []
    for b0 in range(0, B, CHUNK):
        b1 = min(B, b0 + CHUNK)
        cls = cls_all[b0:b1].to(device=dev, dtype=torch.float32).contiguous()
        masks = masks_all[b0:b1].to(device=dev, dtype=torch.float32).contiguous()
        _need_cuda(cls, masks)
        sizes = [(384, 384)] * (b1 - b0) if target_sizes is None else \
            [(int(t[0]), int(t[1])) for t in target_sizes[b0:b1]]
        segs, topk, ps, sid, ws = _run(cls, masks, sizes, float(threshold))
        C = cls.shape[-1] - 1
        topk_h, ps_h, sid_h = topk.cpu().tolist(), ps.cpu().tolist(), sid.cpu().tolist()
        for i in range(b1 - b0):
            segments = [{"id": sid_h[i][j], "label_id": topk_h[i][j] % C, "was_fused": False,
                         "score": round(ps_h[i][j], 6)}
                        for j in range(len(sid_h[i])) if sid_h[i][j] >= 0]
            seg = segs[i]
            if return_binary_maps and segments:  # the reference keeps the -1 map when nothing is kept
                seg = _binary_maps(ws, b1 - b0, cls.shape[1], i, sizes[i], sid, len(segments), dev)
            seg = seg if keep_on_device else seg.cpu()
            if return_coco_annotation:
                from transformers.models.mask2former.image_processing_pil_mask2former import convert_segmentation_to_rle
                seg = convert_segmentation_to_rle(seg)
            results.append({"segmentation": seg, "segments_info": segments})
    return results


MAX_CLASSES = 1024  # semantic and panoptic: the fuse set is a 1024-bit mask (csrc/postprocess_dense.hip)
MAX_QUERIES = 1024  # panoptic: the per-image query tables live in LDS


def _chunks(outputs, target_sizes, device):
    """The inputs of the dense post-processors, CHUNK images at a time: float32 class and mask
    logits on the device and the per-image output sizes (384 x 384 without target_sizes)."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    cls_all, masks_all = outputs.class_queries_logits, outputs.masks_queries_logits
    B = cls_all.shape[0]
    if target_sizes is not None and len(target_sizes) != B:
        raise ValueError("Make sure that you pass in as many target sizes as the batch dimension of the logits")
    for b0 in range(0, B, CHUNK):
        b1 = min(B, b0 + CHUNK)
        cls = cls_all[b0:b1].to(device=dev, dtype=torch.float32).contiguous()
        masks = masks_all[b0:b1].to(device=dev, dtype=torch.float32).contiguous()
        _need_cuda(cls, masks)
        sizes = [(384, 384)] * (b1 - b0) if target_sizes is None else \
            [(int(t[0]), int(t[1])) for t in target_sizes[b0:b1]]
        yield dev, cls, masks, sizes


def _size_args(sizes):
    n = len(sizes)
    return (ctypes.c_int * n)(*[s[0] for s in sizes]), (ctypes.c_int * n)(*[s[1] for s in sizes])


def post_process_semantic_segmentation(outputs, target_sizes=None, return_segmentation_scores: bool = False,
                                       device=None, keep_on_device: bool = False):
    """Same arguments and results as the HF method: per image the int64 class map (argmax over
    the classes of sum_q class probability x mask probability, resized to the target size first),
    or a ``SemanticSegmentationPostProcessorOutput`` with the map and the float32 [C, Ht, Wt]
    scores.  Inputs are moved to float32 on ``device`` (default: the current GPU); results come
    back as CPU tensors unless ``keep_on_device``.  rgbd_pp_semantic, csrc/postprocess_dense.hip."""
    results = []
    L = _lib.lib()
    for dev, cls, masks, sizes in _chunks(outputs, target_sizes, device):
        B, Q, C1 = cls.shape
        maps = [torch.empty(s, dtype=torch.int64, device=dev) for s in sizes]
        scores = [torch.empty((C1 - 1, *s), dtype=torch.float32, device=dev) for s in sizes] \
            if return_segmentation_scores else None
        ws = _workspace(dev, L.rgbd_pp_semantic_workspace_size(B, Q, C1), "postprocess_semantic")
        th, tw = _size_args(sizes)
        mp = (ctypes.c_void_p * B)(*[t.data_ptr() for t in maps])
        sp = (ctypes.c_void_p * B)(*[t.data_ptr() for t in scores]) if scores is not None else None
        check(L.rgbd_pp_semantic(_p(cls), _p(masks), B, Q, C1, masks.shape[-2], masks.shape[-1], th, tw, mp, sp,
                                 _p(ws), _stream(dev)), "rgbd_pp_semantic")
        for i in range(B):
            m = maps[i] if keep_on_device else maps[i].cpu()
            if return_segmentation_scores:
                from transformers.image_processing_outputs import SemanticSegmentationPostProcessorOutput
                s = scores[i] if keep_on_device else scores[i].cpu()
                m = SemanticSegmentationPostProcessorOutput(data={"segmentation": m, "segmentation_scores": s})
            results.append(m)
    return results


def post_process_panoptic_segmentation(outputs, threshold: float = 0.5, mask_threshold: float = 0.5,
                                       overlap_mask_area_threshold: float = 0.8, label_ids_to_fuse=None,
                                       target_sizes=None, device=None, keep_on_device: bool = False):
    """Same arguments and results as the HF method: per image ``{"segmentation", "segments_info"}``
    with the int32 segment-id map (0 = no segment), or the float32 map of -1 and an empty list
    when no query passes ``threshold``.  Inputs are moved to float32 on ``device``; maps come back
    as CPU tensors unless ``keep_on_device``.  The segment table (ids, labels, scores) comes back
    in one device-to-host copy per chunk; nothing else synchronises.  rgbd_pp_panoptic,
    csrc/postprocess_dense.hip."""
    if label_ids_to_fuse is None:
        from transformers.models.mask2former.image_processing_pil_mask2former import logger
        logger.warning("`label_ids_to_fuse` unset. No instance will be fused.")
        label_ids_to_fuse = set()
    fuse = (ctypes.c_ulonglong * (MAX_CLASSES // 64))()
    for c in label_ids_to_fuse:
        if isinstance(c, numbers.Integral) and 0 <= c < MAX_CLASSES:  # a label is an int below C
            fuse[int(c) >> 6] |= 1 << (int(c) & 63)
    results = []
    L = _lib.lib()
    for dev, cls, masks, sizes in _chunks(outputs, target_sizes, device):
        B, Q, C1 = cls.shape
        segs = [torch.empty(s, dtype=torch.int32, device=dev) for s in sizes]
        table = torch.empty((B, 1 + 5 * Q), dtype=torch.int32, device=dev)
        ws = _workspace(dev, L.rgbd_pp_panoptic_workspace_size(B, Q), "postprocess_panoptic")
        th, tw = _size_args(sizes)
        sp = (ctypes.c_void_p * B)(*[t.data_ptr() for t in segs])
        check(L.rgbd_pp_panoptic(_p(cls), _p(masks), B, Q, C1, masks.shape[-2], masks.shape[-1], th, tw,
                                 ctypes.c_double(threshold), ctypes.c_double(mask_threshold),
                                 ctypes.c_double(overlap_mask_area_threshold), fuse, sp, _p(table), _p(ws),
                                 _stream(dev)), "rgbd_pp_panoptic")
        tab = table.cpu()
        ids, labels = tab[:, 1:1 + Q].tolist(), tab[:, 1 + Q:1 + 2 * Q].tolist()
        scores = tab[:, 1 + 2 * Q:1 + 3 * Q].contiguous().view(torch.float32).tolist()
        for i in range(B):
            n = int(tab[i, 0])
            seg = segs[i] if n else segs[i].view(torch.float32)  # nothing kept: the cells hold float32 -1
            segments = [{"id": ids[i][k], "label_id": labels[i][k], "was_fused": labels[i][k] in label_ids_to_fuse,
                         "score": round(scores[i][k], 6)} for k in range(n) if ids[i][k] > 0]
            results.append({"segmentation": seg if keep_on_device else seg.cpu(), "segments_info": segments})
    return results


def _device_covers(outputs) -> bool:
    """Inputs the device path takes: a class-logit table the top-k selection fits in LDS."""
    cls = outputs.class_queries_logits
    return cls.dim() == 3 and cls.shape[1] * (cls.shape[2] - 1) * 8 <= 163840 and cls.shape[2] >= 2


def _dense_covers(outputs, panoptic: bool) -> bool:
    """Inputs the semantic / panoptic device paths take: at most MAX_CLASSES classes, and for the
    panoptic path at most MAX_QUERIES queries."""
    cls, masks = outputs.class_queries_logits, outputs.masks_queries_logits
    return cls.dim() == 3 and masks.dim() == 4 and 2 <= cls.shape[2] <= MAX_CLASSES + 1 and cls.shape[1] >= 1 \
        and (not panoptic or cls.shape[1] <= MAX_QUERIES)


_TASKS = {
    "instance": ("post_process_instance_segmentation", post_process_instance_segmentation, _device_covers),
    "semantic": ("post_process_semantic_segmentation", post_process_semantic_segmentation,
                 lambda outputs: _dense_covers(outputs, False)),
    "panoptic": ("post_process_panoptic_segmentation", post_process_panoptic_segmentation,
                 lambda outputs: _dense_covers(outputs, True)),
}


def install(image_processor, device=None, tasks=("instance",)):
    """Route the post-processors named in ``tasks`` ("instance", "semantic", "panoptic") of an HF
    Mask2Former image processor instance through the device paths.  The default routes
    ``post_process_instance_segmentation`` alone, as the reference's predictor calls it and as
    its Evaluator does with ``return_binary_maps=True`` (model_essential_part.py:87-92).
    Each original bound method is kept (``image_processor._hf_<name>``) and taken for inputs the
    device path does not cover (a class table too large for the LDS top-k; more than
    MAX_CLASSES classes or MAX_QUERIES queries for the dense paths), so an installed processor
    never fails where the reference's would not."""
    for task in tasks:
        if task not in _TASKS:
            raise ValueError(f"unknown post-processing task {task!r}: expected one of {sorted(_TASKS)}")
        name, fn, covers = _TASKS[task]
        original = getattr(image_processor, "_hf_" + name, getattr(image_processor, name))
        setattr(image_processor, "_hf_" + name, original)
        setattr(image_processor, name, _routed(original, fn, covers, device))
    return image_processor


def _routed(original, fn, covers, device):
    def method(outputs, *args, **kwargs):
        if not covers(outputs):
            return original(outputs, *args, **kwargs)
        kwargs.setdefault("device", device)
        return fn(outputs, *args, **kwargs)
    return method
