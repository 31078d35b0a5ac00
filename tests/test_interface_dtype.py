"""The float32-interface bf16 mode of the hot path (compute dtype bfloat16, interface dtype
float32: DESIGN.md §5.11), the parts that need no device: the exported symbols, the host-side
argument checks of the new entry points, the (dtype, interface_dtype) validation of prepare() /
hot_path() and the mode kept on the model."""
import ctypes

import pytest
import torch

from rgbd_amd import _lib, ops
from rgbd_amd.hot_path import float32_interface, hot_path, prepare

NEW = ("rgbd_nchw_to_nhwc_multi_f32", "rgbd_dsam_fwd_nhwc")
E_ARG, E_SHAPE, E_DTYPE = -1, -2, -3


def test_new_symbols_exported():
    L = _lib.lib()
    declared = _lib.header_symbols()
    for name in NEW:
        assert name in declared, f"{name} not declared in include/rgbd_hip.h"
        assert name in _lib.SIGNATURES
        assert hasattr(L, name), f"{name} not exported by librgbd_hip.so"
    for name in ("nchw_to_nhwc_multi_f32", "dsam_fwd_nhwc_f32io"):
        assert callable(getattr(ops, name))


def _job(src, dst, B, C, H, W, dt):
    arr = (ops._NhwcJobF32 * 1)()
    arr[0] = ops._NhwcJobF32(src, dst, B, C, H, W, dt)
    return arr


def test_layout_entry_point_argument_checks():
    """Refused on the host, nothing launched: null pointers, non-positive sizes and misaligned
    pointers RGBD_E_ARG, C % 8 RGBD_E_SHAPE, a destination dtype other than bf16 / float32
    RGBD_E_DTYPE."""
    L = _lib.lib()
    null = ctypes.c_void_p(0)
    fake = 4096
    f = L.rgbd_nchw_to_nhwc_multi_f32
    assert f(0, _job(fake, fake, 1, 8, 2, 2, _lib.RGBD_BF16), null) == E_ARG
    assert f(5, _job(fake, fake, 1, 8, 2, 2, _lib.RGBD_BF16), null) == E_ARG
    assert f(1, null, null) == E_ARG
    assert f(1, _job(None, fake, 1, 8, 2, 2, _lib.RGBD_BF16), null) == E_ARG
    assert f(1, _job(fake, None, 1, 8, 2, 2, _lib.RGBD_F32), null) == E_ARG
    assert f(1, _job(fake, fake, 0, 8, 2, 2, _lib.RGBD_F32), null) == E_ARG
    assert f(1, _job(fake, fake, 1, 8, 2, -1, _lib.RGBD_F32), null) == E_ARG
    assert f(1, _job(fake + 4, fake, 1, 8, 2, 2, _lib.RGBD_F32), null) == E_ARG
    assert f(1, _job(fake, fake + 8, 1, 8, 2, 2, _lib.RGBD_BF16), null) == E_ARG
    assert f(1, _job(fake, fake, 1, 12, 2, 2, _lib.RGBD_BF16), null) == E_SHAPE
    assert f(1, _job(fake, fake, 1, 8, 2, 2, 7), null) == E_DTYPE


def test_dsam_f32io_entry_point_argument_checks():
    """The checks of rgbd_dsam_fwd_nhwc before any launch, its float32 pointers' included: a compute
    dtype other than RGBD_BF16 is RGBD_E_DTYPE; null pointers, bad sizes, no output at all, a bf16
    residual beside a float32 pointer, misaligned float32 pointers and no plan RGBD_E_ARG."""
    L = _lib.lib()
    null = ctypes.c_void_p(0)
    fake = ctypes.c_void_p(4096)

    def call(dt, x, out, ws, res16=null, res32=null, out32=null, B=1, plan=fake):
        return L.rgbd_dsam_fwd_nhwc(dt, x, fake, fake, B, 32, 8, 8, 64, fake, fake, res16, out, res32, out32, plan, ws,
                                    null)
    bf, f32 = _lib.RGBD_BF16, _lib.RGBD_F32
    assert call(f32, fake, fake, fake, out32=fake) == E_DTYPE
    assert call(7, fake, fake, fake, out32=fake) == E_DTYPE
    assert call(bf, null, fake, fake, out32=fake) == E_ARG
    assert call(bf, fake, null, fake) == E_ARG                      # no output at all
    assert call(bf, fake, fake, null, out32=fake) == E_ARG          # no workspace
    assert call(bf, fake, fake, fake, out32=fake, B=0) == E_ARG
    assert call(bf, fake, fake, fake, res16=fake, out32=fake) == E_ARG
    assert call(bf, fake, fake, fake, res16=fake, res32=fake) == E_ARG
    assert call(bf, fake, fake, fake, out32=ctypes.c_void_p(4100)) == E_ARG
    assert call(bf, fake, fake, fake, res32=ctypes.c_void_p(4104), out32=fake) == E_ARG
    assert call(bf, fake, fake, fake, out32=fake, plan=null) == E_ARG


def _cpu_inputs():
    pv = torch.zeros((1, 10, 16, 16))
    colors = [torch.zeros((1, c, 4 >> k or 1, 4 >> k or 1)) for k, c in enumerate([96, 192, 384, 768])]
    return pv, colors


@pytest.mark.parametrize("dtype,interface", [(torch.bfloat16, torch.float16), (torch.float32, torch.float16),
                                             (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16),
                                             (torch.float16, torch.float32)])
def test_bad_mode_is_a_value_error_before_any_tensor_is_touched(dtype, interface):
    """CPU tensors (and no modules at all): the mode is refused first, as a ValueError, not the
    RuntimeError the kernels' wrappers raise for a CPU tensor."""
    pv, colors = _cpu_inputs()
    with pytest.raises(ValueError, match="interface_dtype"):
        prepare(pv, colors, dtype, interface_dtype=interface)
    with pytest.raises(ValueError, match="interface_dtype"):
        hot_path(pv, torch.zeros((1, 1)), colors, None, None, dtype=dtype, interface_dtype=interface)


def test_accepted_modes():
    assert float32_interface(torch.bfloat16, None) is False
    assert float32_interface(torch.float32, None) is False
    assert float32_interface(torch.float32, torch.float32) is False  # the float32 mode
    assert float32_interface(torch.bfloat16, torch.float32) is True
    # a valid mode on CPU tensors gets as far as the wrappers' CPU-tensor refusal
    pv, colors = _cpu_inputs()
    with pytest.raises(RuntimeError, match="GPU only"):
        prepare(pv, colors, torch.bfloat16, interface_dtype=torch.float32)


def test_set_compute_dtype_stores_the_mode():
    from rgbd_amd.config import standard_config
    from rgbd_amd.custom_model import CustomMask2FormerForUniversalSegmentation
    m = CustomMask2FormerForUniversalSegmentation(standard_config(48), version="0.4.0")
    plm = m.model.pixel_level_module
    assert plm.interface_dtype is None
    assert m.set_compute_dtype(torch.bfloat16, interface=torch.float32) is m
    assert plm.compute_dtype == torch.bfloat16 and plm.interface_dtype == torch.float32
    assert plm.dsam0.compute_dtype == torch.bfloat16
    with pytest.raises(ValueError):
        m.set_compute_dtype(torch.float32, interface=torch.bfloat16)
    assert plm.compute_dtype == torch.bfloat16 and plm.interface_dtype == torch.float32  # unchanged by the refusal
    plm.set_compute_dtype(torch.bfloat16)
    assert plm.interface_dtype is None
    m.set_compute_dtype(torch.float32, interface=torch.float32)
    assert plm.compute_dtype == torch.float32 and plm.interface_dtype == torch.float32
