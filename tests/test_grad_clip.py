"""Gradient-norm clipping (rgbd_amd.optim: HipAdamW(max_grad_norm=...), clip_grad_norm_; the
rgbd_grad_sumsq_multi / rgbd_grad_norm_finalize / rgbd_adamw_multi_scaled / rgbd_scale_multi entry
points), the part that needs no GPU: option validation, the refusals, and the host-side argument
validation of the new entry points (nothing is launched)."""
import ctypes

import pytest
import torch

import _rgbd_import  # noqa: F401
from rgbd_amd import _lib

NULL, FAKE = ctypes.c_void_p(0), ctypes.c_void_p(0x1000)
E_ARG = -1


def _param(n=4):
    return torch.zeros(n, requires_grad=True)


def test_max_grad_norm_option_validation():
    from rgbd_amd.optim import HF_TRAINER_ADAMW, HF_TRAINER_CLIP, HipAdamW
    assert HF_TRAINER_CLIP == 1.0
    for bad in (0, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            HipAdamW([_param()], max_grad_norm=bad)
    assert HipAdamW([_param()]).max_grad_norm is None
    assert HipAdamW([_param()], max_grad_norm=None).grad_norm is None
    opt = HipAdamW([_param()], **HF_TRAINER_ADAMW, max_grad_norm=HF_TRAINER_CLIP)
    assert opt.max_grad_norm == 1.0 and opt.grad_norm is None  # no step yet


def test_clipped_step_refuses_cpu_parameters():
    from rgbd_amd.optim import HipAdamW
    p = _param()
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError):
        HipAdamW([p], max_grad_norm=1.0).step()


def test_in_backward_optimizer_refuses_a_clipping_optimizer():
    from rgbd_amd.distributed import InBackwardOptimizer
    from rgbd_amd.optim import HipAdamW
    groups = [[_param()], [_param()], [_param()]]
    with pytest.raises(ValueError, match="after the backward"):
        InBackwardOptimizer(groups, lambda ps: HipAdamW(ps, max_grad_norm=1.0))
    opt = InBackwardOptimizer(groups, lambda ps: HipAdamW(ps))  # without it: as before
    assert len(opt.opts) == 2


def test_clip_grad_norm_refusals():
    from rgbd_amd.optim import clip_grad_norm_
    p = _param()
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="CUDA"):
        clip_grad_norm_([p], 1.0)
    with pytest.raises(RuntimeError, match="CUDA"):
        clip_grad_norm_(p, 1.0)  # a single tensor, as torch accepts
    for nt in (1.0, float("inf"), 3):
        with pytest.raises(NotImplementedError):
            clip_grad_norm_([p], 1.0, norm_type=nt)
    with pytest.raises(NotImplementedError):
        clip_grad_norm_([p], 1.0, error_if_nonfinite=True)
    q = _param()  # no gradient anywhere: torch's answer, nothing launched
    assert float(clip_grad_norm_([q], 1.0)) == 0.0


def _tables(n, ptr=0x1000, numel=8):
    return (ctypes.c_void_p * n)(*[ptr] * n), (ctypes.c_longlong * n)(*[numel] * n)


def test_new_entry_points_validate_on_the_host():
    L = _lib.lib()
    X, N = _tables(2)
    # grad_sumsq: null tables, n above the table size (128), negative numel, negative slot
    assert L.rgbd_grad_sumsq_multi(0, NULL, NULL, NULL, 0, NULL) == 0
    assert L.rgbd_grad_sumsq_multi(2, NULL, N, FAKE, 0, NULL) == E_ARG
    assert L.rgbd_grad_sumsq_multi(2, X, NULL, FAKE, 0, NULL) == E_ARG
    assert L.rgbd_grad_sumsq_multi(2, X, N, NULL, 0, NULL) == E_ARG
    assert L.rgbd_grad_sumsq_multi(2, X, N, FAKE, -1, NULL) == E_ARG
    assert L.rgbd_grad_sumsq_multi(-1, X, N, FAKE, 0, NULL) == E_ARG
    Xb, Nb = _tables(129)
    assert L.rgbd_grad_sumsq_multi(129, Xb, Nb, FAKE, 0, NULL) == E_ARG
    assert L.rgbd_scale_multi(129, Xb, Nb, FAKE, NULL) == E_ARG
    Xn, Nn = _tables(2, numel=-1)
    assert L.rgbd_grad_sumsq_multi(2, Xn, Nn, FAKE, 0, NULL) == E_ARG
    assert L.rgbd_scale_multi(2, Xn, Nn, FAKE, NULL) == E_ARG
    X0, N0 = _tables(2, ptr=0)  # a null tensor with elements
    assert L.rgbd_grad_sumsq_multi(2, X0, N0, FAKE, 0, NULL) == E_ARG
    assert L.rgbd_scale_multi(2, X0, N0, FAKE, NULL) == E_ARG
    Xe, Ne = _tables(2, ptr=0, numel=0)  # only empty tensors: an empty success, nothing launched
    assert L.rgbd_grad_sumsq_multi(2, Xe, Ne, FAKE, 0, NULL) == 0
    assert L.rgbd_scale_multi(2, Xe, Ne, FAKE, NULL) == 0
    # scale: null tables / scalar
    assert L.rgbd_scale_multi(0, NULL, NULL, NULL, NULL) == 0
    assert L.rgbd_scale_multi(2, NULL, N, FAKE, NULL) == E_ARG
    assert L.rgbd_scale_multi(2, X, NULL, FAKE, NULL) == E_ARG
    assert L.rgbd_scale_multi(2, X, N, NULL, NULL) == E_ARG
    # finalise
    assert L.rgbd_grad_norm_finalize(NULL, 0, 1.0, NULL, NULL) == 0
    assert L.rgbd_grad_norm_finalize(NULL, 1, 1.0, FAKE, NULL) == E_ARG
    assert L.rgbd_grad_norm_finalize(FAKE, 1, 1.0, NULL, NULL) == E_ARG
    assert L.rgbd_grad_norm_finalize(FAKE, -1, 1.0, FAKE, NULL) == E_ARG
    # scaled AdamW: the tables of rgbd_adamw_multi (48), plus the device scale
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0, NULL)
    assert L.rgbd_adamw_multi_scaled(0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, *hyper) == 0
    assert L.rgbd_adamw_multi_scaled(2, X, X, X, X, NULL, N, FAKE, NULL, *hyper) == E_ARG   # no scale
    assert L.rgbd_adamw_multi_scaled(2, X, NULL, X, X, NULL, N, FAKE, FAKE, *hyper) == E_ARG
    assert L.rgbd_adamw_multi_scaled(2, X, X, X, X, NULL, N, NULL, FAKE, *hyper) == E_ARG   # no step
    assert L.rgbd_adamw_multi_scaled(2, X, X, X, X, NULL, Nn, FAKE, FAKE, *hyper) == E_ARG  # negative numel
    X49, N49 = _tables(49)
    assert L.rgbd_adamw_multi_scaled(49, X49, X49, X49, X49, NULL, N49, FAKE, FAKE, *hyper) == E_ARG


def test_sumsq_workspace_size_is_eight_bytes_per_chunk():
    L = _lib.lib()
    N = (ctypes.c_longlong * 6)(0, 1, 4096, 4097, 3 * 4096, -5)
    assert L.rgbd_grad_sumsq_workspace_size(6, N) == 8 * (0 + 1 + 1 + 2 + 3 + 0)
    assert L.rgbd_grad_sumsq_workspace_size(6, N) == L.rgbd_grad_sumsq_workspace_size(6, N)
    assert L.rgbd_grad_sumsq_workspace_size(0, N) == 0
    assert L.rgbd_grad_sumsq_workspace_size(3, NULL) == 0
