"""C-ABI boundary checks that run without a GPU: the library loads, exports every symbol
include/rgbd_hip.h declares, and the host-side argument validation rejects bad calls
before anything is launched."""
import ctypes

import pytest

from rgbd_amd import _lib


def test_library_loads_and_exports_header_symbols():
    L = _lib.lib()
    declared = _lib.header_symbols()
    assert len(declared) >= 14
    missing = [s for s in declared if not hasattr(L, s)]
    assert not missing, f"declared but not exported: {missing}"
    assert set(declared) == set(_lib.SIGNATURES), "ctypes table out of sync with the header"
    assert L.rgbd_version().startswith(b"rgbd_hip")


def test_decomp_info_layout_matches_header():
    assert _lib.DECOMP_INFO_DTYPE.itemsize == 4 * (3 + 3 + 2 + 3 + 3 + 3) + 4 * 512


def test_argument_validation_without_device():
    L = _lib.lib()
    null = ctypes.c_void_p(0)
    # null pointers / bad sizes are rejected on the host with RGBD_E_ARG, nothing launched
    assert L.rgbd_assemble_pixel_values(null, null, 1, 4, 4, null, null, null) == -1
    assert L.rgbd_dsam_fwd(0, null, null, null, 1, 32, 8, 8, 64, null, null, null, null, null, null, null, null) == -1
    fake = ctypes.c_void_p(0x1000)
    # Cin not a multiple of 8 -> unsupported shape
    assert L.rgbd_dsam_fwd(0, fake, fake, fake, 1, 12, 8, 8, 64, fake, fake, null, fake, null, null, null, null) == -2
    # unknown dtype
    assert L.rgbd_nchw_to_nhwc(7, fake, fake, 1, 1, 1, 1, null) == -3


def test_flat_grids_past_int_range_are_refused():
    """The DGGM kernels and the NHWC multi kernel index one flat grid with an int: a call whose
    block count, or a job whose H * W, does not fit is RGBD_E_SHAPE on the host, nothing launched."""
    from rgbd_amd import ops
    L = _lib.lib()
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(0x1000)
    # 65536 images x 2048 pixel tiles x 32 channel blocks = 2^32 blocks
    assert L.rgbd_dggm_fuse_fwd(1, null, fake, fake, fake, 640, 65536, 8, 8, 1024, 1024, 1024, fake, fake, fake, null) == -2
    assert L.rgbd_dggm_fuse_bwd(1, fake, fake, fake, 640, 65536, 8, 8, 1024, 1024, 1024, fake, fake, fake, fake, fake,
                                null) == -2
    job = (ops._NhwcJob * 1)(ops._NhwcJob(0x1000, 0x1000, 1, 8, 65536, 32768))
    assert L.rgbd_nchw_to_nhwc_multi(1, job, null) == -2


def test_dsam_run_calls_argument_validation_without_device():
    """The other K5 run calls, refused on the host like rgbd_dsam_fwd: null pointers RGBD_E_ARG and
    a contraction channel count that is no multiple of 8 RGBD_E_SHAPE with RGBD_F32 (dX contracts
    over Cout, so its check is Cout % 8; dW's is Cin % 8 as the forward's); with RGBD_BF16 every run
    call needs its leg's plan (NULL: RGBD_E_ARG)."""
    L = _lib.lib()
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(0x1000)
    f32, bf = _lib.RGBD_F32, _lib.RGBD_BF16
    assert L.rgbd_dsam_bwd_data(f32, null, null, 1, 32, 8, 8, 64, null, null, null, null, null, null, null, null) == -1
    assert L.rgbd_dsam_bwd_data(f32, fake, fake, 1, 32, 8, 8, 12, fake, null, null, fake, null, null, fake, null) == -2
    assert L.rgbd_dsam_bwd_weight(f32, null, null, null, null, null, 1, 32, 8, 8, 64, null, null, null, null, null,
                                  null) == -1
    assert L.rgbd_dsam_bwd_weight(f32, fake, null, fake, fake, fake, 1, 12, 8, 8, 64, fake, fake, fake, null, fake,
                                  null) == -2
    assert L.rgbd_dsam_fwd(bf, fake, fake, fake, 1, 32, 8, 8, 64, fake, fake, null, fake, null, null, fake, null) == -1
    assert L.rgbd_dsam_fwd_nhwc(bf, fake, fake, fake, 1, 32, 8, 8, 64, fake, fake, null, fake, null, null, null, fake,
                                null) == -1
    assert L.rgbd_dsam_bwd_data(bf, fake, fake, 1, 32, 8, 8, 64, fake, null, null, fake, null, null, fake, null) == -1
    assert L.rgbd_dsam_bwd_weight(bf, null, fake, fake, fake, fake, 1, 32, 8, 8, 64, fake, fake, fake, null, fake,
                                  null) == -1


def test_layernorm_argument_validation_without_device():
    """The two LayerNorm calls (one per pass; r == NULL is the plain norm): what does not go with
    the plain norm is RGBD_E_ARG, what the fused sum or the backward's clamp / bf16 twin need of C
    and the pointers' alignment RGBD_E_SHAPE, an unknown dtype RGBD_E_DTYPE — nothing launched."""
    L = _lib.lib()
    null, fake, odd = ctypes.c_void_p(0), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1008)
    f32 = _lib.RGBD_F32

    def fwd(x=fake, r=null, C=256, clamp=0.0, s_out=null, y2=null, x_dtype=f32, r_dtype=f32, y_dtype=f32):
        return L.rgbd_layernorm_fwd(x_dtype, x, r_dtype, r, fake, fake, 37, C, 1e-5, clamp, y_dtype, s_out, fake, y2,
                                    fake, fake, null)

    def bwd(C=256, clamp=0.0, dx_bf16=null, x_dtype=f32, dy_dtype=f32, dx=fake):
        return L.rgbd_layernorm_bwd(x_dtype, fake, dy_dtype, fake, fake, null, fake, fake, 37, C, clamp, dx, dx_bf16,
                                    fake, fake, fake, null)

    assert fwd(s_out=fake) == -1 and fwd(y2=fake) == -1 and fwd(clamp=1.0) == -1  # r == NULL: the plain norm
    assert fwd(r=fake) == -1                                                        # r needs s_out
    assert fwd(x=null) == -1 and bwd(dx=null) == -1
    assert fwd(r=fake, s_out=fake, C=1002) == -2
    assert fwd(x=odd, r=fake, s_out=fake) == -2
    assert fwd(r=fake, s_out=fake, y2=odd) == -2
    assert fwd(C=1540) == -2 and fwd(r=fake, s_out=fake, C=1540) == -2 and bwd(C=1540) == -2
    assert fwd(x_dtype=7) == -3 and fwd(y_dtype=7) == -3 and fwd(r=fake, s_out=fake, r_dtype=7) == -3
    assert bwd(x_dtype=7) == -3 and bwd(dy_dtype=7) == -3
    assert bwd(C=1002, clamp=1.0) == -2
    assert bwd(C=1002, dx_bf16=fake) == -2
    assert bwd(dx_bf16=odd) == -2


def test_add_layernorm_entry_points_are_gone():
    """rgbd_layernorm_fwd / _bwd took over the fused calls: header, ctypes table and library."""
    L = _lib.lib()
    for name in ("rgbd_add_layernorm_fwd", "rgbd_add_layernorm_bwd"):
        assert name not in _lib.header_symbols() and name not in _lib.SIGNATURES and not hasattr(L, name)
    assert len(_lib.SIGNATURES) == 126


def test_ops_refuse_cpu_tensors():
    import torch
    from rgbd_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.nchw_to_nhwc(torch.zeros(1, 8, 4, 4))


def test_mask_predictor_install_keeps_state_dict():
    """f1 drop-in: the decoder's Mask2FormerMaskPredictor becomes HipMaskPredictor by a class
    swap — same parameters, same state_dict keys (no GPU needed)."""
    from transformers.models.mask2former.modeling_mask2former import Mask2FormerMaskPredictor
    from rgbd_amd import mask_predictor
    m = Mask2FormerMaskPredictor(hidden_size=32, num_heads=4, mask_feature_size=32)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    assert mask_predictor.install(m) == 1
    assert type(m) is mask_predictor.HipMaskPredictor
    after = m.state_dict()
    assert list(after) == list(before) and all(bool((after[k] == before[k]).all()) for k in before)
    assert mask_predictor.install(m) == 0


def _zero_args(argtypes, fill_int):
    out = []
    for t in argtypes:
        if t in (ctypes.c_double, ctypes.c_float):
            out.append(0.0)
        elif t is ctypes.c_void_p:
            out.append(None)
        elif t is ctypes.c_char_p:
            out.append(b"")
        else:
            out.append(fill_int)
    return out


@pytest.mark.parametrize("fill_int", [0, 1, -1], ids=["sizes0", "sizes1", "sizes-1"])
def test_every_entry_point_survives_null_arguments(fill_int):
    """Host-side robustness of the whole boundary (run under AddressSanitizer by
    ``make -C rgb-d-instance-segmentation_amd/csrc asan-test``): every status-returning entry
    point called with null pointers and all sizes 0, 1 or -1 returns a status — 0 for an empty
    call, a negative argument code or a HIP error — and never reads through a null pointer or
    out of bounds on the host.  Without a GPU (this test is skipped where one is visible: a call
    that passed validation would launch)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: a call that passes validation would launch a kernel on null pointers")
    L = _lib.lib()
    for name, (res, args) in _lib.SIGNATURES.items():
        if res is not ctypes.c_int or name == "rgbd_timing_enable":
            continue
        rc = getattr(L, name)(*_zero_args(args, fill_int))
        assert isinstance(rc, int), name
        if fill_int != 0:  # non-empty work on null pointers must be refused (or fail to launch)
            assert rc != 0, f"{name} accepted null pointers for a non-empty call"


def test_size_queries_are_pure():
    """Workspace / plan size queries: no device needed, deterministic, non-negative."""
    L = _lib.lib()
    for name, (res, args) in _lib.SIGNATURES.items():
        if res is not ctypes.c_size_t or any(a is ctypes.c_void_p for a in args):
            continue
        for v in (0, 1, 8, 480):
            a = [v] * len(args)
            assert getattr(L, name)(*a) == getattr(L, name)(*a), name
