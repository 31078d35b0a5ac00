"""AdamW on the HIP kernel (csrc/adamw.hip, rgbd_adamw_multi), with torch.optim.AdamW's update
(decoupled weight decay, no amsgrad, no maximize).  One launch per group of up to 48 tensors;
the step count lives on the device, so the step can be captured into a HIP graph
(``capturable`` is always true).  fp32 parameters and gradients on the GPU only.

The constructor defaults are torch's (weight_decay 1e-2).  The optimizer the reference's HF
Trainer builds (finetuning.py:98) is ``HipAdamW(params, **HF_TRAINER_ADAMW)``: lr 1e-5 constant
(mask2former/config.json:12-13) and TrainingArguments' defaults for the rest — weight_decay
0.0 (config.json does not set it), betas (0.9, 0.999), eps 1e-8.

A parameter that a HIP layer casts to bfloat16 (dense.cast_weight, under autocast) gets its bf16
copy rewritten by the same launch (rgbd_adamw_multi_shadow) and re-keyed, so the next forward
takes it without one cast launch per weight.

``max_grad_norm`` (``HF_TRAINER_CLIP`` for the reference) adds the Trainer's global-norm clip to
the step: the L2 norm of every gradient of every group (rgbd_grad_sumsq_multi +
rgbd_grad_norm_finalize, no atomics, no host read), and the AdamW launches multiply each gradient
by the clip coefficient they read from the device (rgbd_adamw_multi_scaled), so the gradients are
read once more and never rewritten.  ``clip_grad_norm_`` is the stand-alone form that leaves the
clipped gradients in ``p.grad`` (torch.nn.utils.clip_grad_norm_, L2 only).  DESIGN.md §5.14.

bench.py's optimizer (in-backward groups and the captured step); DESIGN.md §9."""
import ctypes

import torch

from . import _lib
from ._lib import check
from .ops import _stream, _workspace

_MAXT = 48
# HF TrainingArguments' AdamW (adam_beta1/2, adam_epsilon, weight_decay defaults) at the
# reference's learning rate (mask2former/config.json:12)
HF_TRAINER_ADAMW = dict(lr=1e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
# HF TrainingArguments' max_grad_norm default (mask2former/config.json does not set it): the
# Trainer clips the global L2 norm of all gradients to it before every optimizer step
# (Trainer._clip_grad_norm -> torch.nn.utils.clip_grad_norm_, behind finetuning.py:98)
HF_TRAINER_CLIP = 1.0
_NORM_MAXT = 128  # tensors per rgbd_grad_sumsq_multi / rgbd_scale_multi launch


def _check_grads(grads, what):
    dev = grads[0].device
    for g in grads:
        if not g.is_cuda:
            raise RuntimeError(f"{what}: CUDA gradients only (no CPU fallback)")
        if g.dtype != torch.float32 or g.is_sparse or not g.is_contiguous():
            raise RuntimeError(f"{what}: dense contiguous float32 gradients only")
        if g.device != dev:
            raise RuntimeError(f"{what}: all gradients on one device (the global norm is one reduction)")


def _grad_norm_launch(grads, max_norm, out):
    """Norm + finalise of ``grads`` (checked: one device, float32, contiguous) on the current
    stream: out[0] = total norm, out[1] = clip coefficient.  No host read.  Returns the launch
    tables (n, pointers, numels, first slot), one per 128 tensors."""
    L = _lib.lib()
    dev = grads[0].device
    tables = []
    slots = 0
    for i in range(0, len(grads), _NORM_MAXT):
        run = grads[i:i + _NORM_MAXT]
        n = len(run)
        G = (ctypes.c_void_p * n)(*[g.data_ptr() for g in run])
        N = (ctypes.c_longlong * n)(*[g.numel() for g in run])
        tables.append((n, G, N, slots))
        slots += L.rgbd_grad_sumsq_workspace_size(n, N) // 8
    ws = _workspace(dev, 8 * slots, "grad_norm")
    stream = _stream(dev)
    for n, G, N, slot0 in tables:
        check(L.rgbd_grad_sumsq_multi(n, G, N, ctypes.c_void_p(ws.data_ptr()), slot0, stream), "rgbd_grad_sumsq_multi")
    check(L.rgbd_grad_norm_finalize(ctypes.c_void_p(ws.data_ptr()), slots, float(max_norm),
                                    ctypes.c_void_p(out.data_ptr()), stream), "rgbd_grad_norm_finalize")
    return tables


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_ for the L2 norm on the HIP kernels: the gradients of
    ``parameters`` are scaled in place by min(1, max_norm / (total_norm + 1e-6)) and the total norm
    comes back as a 0-d device tensor (three kinds of launch on the current stream, no host read).
    ``foreach`` is accepted for signature compatibility; other ``norm_type`` values and
    ``error_if_nonfinite=True`` (a host read) are not implemented."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    if float(norm_type) != 2.0:
        raise NotImplementedError(f"clip_grad_norm_: only the L2 norm (norm_type=2.0), got {norm_type}")
    if error_if_nonfinite:
        raise NotImplementedError("clip_grad_norm_: error_if_nonfinite=True needs a host read of the norm")
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    _check_grads(grads, "clip_grad_norm_")
    L = _lib.lib()
    dev = grads[0].device
    out = torch.empty(2, dtype=torch.float32, device=dev)
    for n, G, N, _ in _grad_norm_launch(grads, max_norm, out):
        check(L.rgbd_scale_multi(n, G, N, ctypes.c_void_p(out.data_ptr() + 4), _stream(dev)), "rgbd_scale_multi")
    torch.autograd.graph.increment_version(grads)
    return out[0]


def _shadow(p):
    """The bfloat16 copy of ``p`` that dense.cast_weight holds (the bf16 GEMM operand of a HIP
    layer under autocast), re-used as the buffer the step writes the updated copy into; None when
    the parameter has none."""
    hit = getattr(p, "_rgbd_cast", None)
    if hit is None or hit[0][3] != torch.bfloat16:
        return None
    x = hit[1]
    if x.dtype != torch.bfloat16 or x.shape != p.shape or not x.is_contiguous() or x.device != p.device:
        return None
    return x


class HipAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None):
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("HipAdamW: invalid hyper-parameters")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"HipAdamW: max_grad_norm must be positive or None (no clipping), got {max_grad_norm}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=True))
        # one global norm over every group (the Trainer clips model.parameters()), so an option of
        # the optimizer, not of a group
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._clip = None  # device [total_norm, clip coefficient] of the last step

    @property
    def grad_norm(self):
        """The global gradient norm before clipping of the last ``step()``: a 0-d device tensor
        (the same storage every step; read it after a sync of the caller's choosing).  None
        without ``max_grad_norm`` or before the first step."""
        return None if self._clip is None else self._clip[0]

    def _group_state(self, group):
        """The group's parameters with gradients, their moments, and ONE step count per group
        (one device tensor, so a captured graph advances every parameter's step with one kernel).
        That is torch's per-parameter count only while every parameter of the group is stepped
        every time; a parameter that would join a group whose count already runs (its first
        gradient arriving after other parameters' first step) would inherit the group's count
        and a wrong bias correction, so it is refused."""
        params = [p for p in group["params"] if p.grad is not None]
        shared = None
        for p in group["params"]:
            if p in self.state and "step" in self.state[p]:
                shared = self.state[p]["step"]
                break
        if shared is not None and any(not self.state[p] for p in params):
            raise RuntimeError("HipAdamW: a parameter received its first gradient after the rest of its group "
                               "had stepped; its step count would not be its own (put it in its own group)")
        for p in params:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("HipAdamW: contiguous float32 CUDA parameters only (no CPU fallback)")
            g = p.grad
            if g.dtype != torch.float32 or not g.is_contiguous() or g.is_sparse:
                raise RuntimeError("HipAdamW: dense contiguous float32 gradients only")
            st = self.state[p]
            if not st:
                if shared is None:
                    shared = torch.zeros((), dtype=torch.float32, device=p.device)
                st["step"] = shared
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return params, shared

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L = _lib.lib()
        work = [self._group_state(group) for group in self.param_groups]
        scale = None
        if self.max_grad_norm is not None:
            grads = [p.grad for params, _ in work for p in params]
            if grads:
                _check_grads(grads, "HipAdamW(max_grad_norm)")
                if self._clip is None:  # in the first (eager) step, like the moments
                    self._clip = torch.zeros(2, dtype=torch.float32, device=grads[0].device)
                _grad_norm_launch(grads, self.max_grad_norm, self._clip)
                scale = ctypes.c_void_p(self._clip.data_ptr() + 4)
        for group, (params, step) in zip(self.param_groups, work):
            if not params:
                continue
            step.add_(1.0)  # on the device: a captured graph replays the increment
            b1, b2 = group["betas"]
            shadows = [_shadow(p) for p in params]
            for i in range(0, len(params), _MAXT):
                run = params[i:i + _MAXT]
                n = len(run)
                P = (ctypes.c_void_p * n)(*[p.data_ptr() for p in run])
                G = (ctypes.c_void_p * n)(*[p.grad.data_ptr() for p in run])
                M = (ctypes.c_void_p * n)(*[self.state[p]["exp_avg"].data_ptr() for p in run])
                V = (ctypes.c_void_p * n)(*[self.state[p]["exp_avg_sq"].data_ptr() for p in run])
                N = (ctypes.c_longlong * n)(*[p.numel() for p in run])
                sh = shadows[i:i + _MAXT]
                args = (float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                        _stream(run[0].device))
                if scale is not None:
                    S = None
                    if any(x is not None for x in sh):
                        S = (ctypes.c_void_p * n)(*[None if x is None else x.data_ptr() for x in sh])
                    check(L.rgbd_adamw_multi_scaled(n, P, G, M, V, S, N, ctypes.c_void_p(step.data_ptr()), scale,
                                                    *args), "rgbd_adamw_multi_scaled")
                elif any(x is not None for x in sh):
                    S = (ctypes.c_void_p * n)(*[None if x is None else x.data_ptr() for x in sh])
                    check(L.rgbd_adamw_multi_shadow(n, P, G, M, V, S, N, ctypes.c_void_p(step.data_ptr()), *args),
                          "rgbd_adamw_multi_shadow")
                else:
                    check(L.rgbd_adamw_multi(n, P, G, M, V, N, ctypes.c_void_p(step.data_ptr()), *args),
                          "rgbd_adamw_multi")
            # the kernel wrote through raw pointers: bump the version counters (host only, safe
            # under capture) so autograd's saved-tensor checks and version-keyed caches see it
            torch.autograd.graph.increment_version(params)
            for p, x in zip(params, shadows):
                if x is not None:  # the bf16 copy the kernel wrote is current: dense.cast_weight's key
                    # after this step (the global post-step hook advances the epoch by one)
                    p._rgbd_cast = ((p.data_ptr(), p._version, getattr(p, "_rgbd_epoch", 0) + 1, torch.bfloat16), x)
        return loss

    def load_state_dict(self, state_dict):
        """torch's load, then the one-step-count-per-group invariant restored: torch moves each
        parameter's ``step`` separately, which would untie them (after which only the first
        parameter's count would advance).  Every parameter of a group gets the group's first
        stored count as its (shared) step tensor; the counts of a group must agree."""
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            steps = [self.state[p]["step"] for p in group["params"] if p in self.state and "step" in self.state[p]]
            if not steps:
                continue
            vals = {float(s) for s in steps}
            if len(vals) != 1:
                raise ValueError(f"HipAdamW.load_state_dict: parameters of one group at different steps {sorted(vals)}")
            dev = group["params"][0].device
            shared = steps[0].detach().to(device=dev, dtype=torch.float32).clone()
            for p in group["params"]:
                if p in self.state and "step" in self.state[p]:
                    self.state[p]["step"] = shared
