"""C-ABI checks of the classification-loss entry points that run without a GPU: the symbols are
exported and bound, and every documented return code comes back from the host-side validation
before anything is launched (the pointers handed in are never dereferenced)."""
import ctypes

import pytest

from rgbd_amd import _lib

NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(0x1000)
F32, BF16 = _lib.RGBD_F32, _lib.RGBD_BF16
E_ARG, E_SHAPE, E_DTYPE = -1, -2, -3


def _fwd(L, dtype=F32, B=2, Q=5, C1=7, M=3, T=4, **ptr):
    p = dict(logits=FAKE, w=FAKE, rows=FAKE, cols=FAKE, moff=FAKE, toff=FAKE, labels=FAKE, ws=FAKE, loss=FAKE,
             wsum=FAKE, stats=FAKE, target=FAKE)
    p.update(ptr)
    return L.rgbd_class_loss_fwd(dtype, p["logits"], p["w"], B, Q, C1, p["rows"], p["cols"], M, p["moff"], p["toff"],
                                 p["labels"], T, p["ws"], p["loss"], p["wsum"], p["stats"], p["target"], NULL)


def _bwd(L, dtype=F32, B=2, Q=5, C1=7, **ptr):
    p = dict(logits=FAKE, w=FAKE, stats=FAKE, target=FAKE, wsum=FAKE, g=FAKE, glogits=FAKE)
    p.update(ptr)
    return L.rgbd_class_loss_bwd(dtype, p["logits"], p["w"], B, Q, C1, p["stats"], p["target"], p["wsum"], p["g"],
                                 p["glogits"], NULL)


def test_symbols_exported_and_bound():
    L = _lib.lib()
    names = ["rgbd_class_loss_fwd", "rgbd_class_loss_bwd", "rgbd_class_loss_workspace_size",
             "rgbd_class_loss_max_classes"]
    for n in names:
        assert hasattr(L, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES and n in _lib.header_symbols()
    assert L.rgbd_class_loss_max_classes() >= 256
    # one (numerator, denominator) pair per block of rows; nothing for an empty problem
    assert L.rgbd_class_loss_workspace_size(8, 100, 49) >= 8
    assert L.rgbd_class_loss_workspace_size(0, 100, 49) == 0


@pytest.mark.parametrize("name", ["logits", "w", "moff", "toff", "ws", "loss", "wsum", "stats", "target", "rows",
                                  "cols", "labels"])
def test_fwd_null_pointer(name):
    assert _fwd(_lib.lib(), **{name: NULL}) == E_ARG


def test_fwd_no_matches_needs_no_match_arrays():
    """M = 0 is legal and takes no rows / cols / labels; here the shape check is what answers, so
    the null arrays were accepted."""
    L = _lib.lib()
    assert _fwd(L, M=0, T=0, rows=NULL, cols=NULL, labels=NULL, C1=1) == E_SHAPE
    assert _fwd(L, M=-1) == E_ARG and _fwd(L, T=-1) == E_ARG


@pytest.mark.parametrize("name", ["logits", "w", "stats", "target", "wsum", "g", "glogits"])
def test_bwd_null_pointer(name):
    assert _bwd(_lib.lib(), **{name: NULL}) == E_ARG


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_sizes_and_dtype(call):
    L = _lib.lib()
    cap = L.rgbd_class_loss_max_classes()
    for bad in (dict(B=0), dict(B=-1), dict(Q=0), dict(Q=-3), dict(C1=0), dict(C1=-1)):
        assert call(L, **bad) == E_ARG, bad
    assert call(L, C1=1) == E_SHAPE
    assert call(L, C1=cap + 1) == E_SHAPE
    assert call(L, B=1 << 15, Q=1 << 10, C1=64) == E_SHAPE  # B Q C1 = 2^31
    assert call(L, dtype=7) == E_DTYPE
    assert call(L, dtype=-1) == E_DTYPE


def test_cpu_tensors_are_refused():
    import torch
    from rgbd_amd import ops, point_loss
    ind = ops.LsaResult([(torch.zeros(0, dtype=torch.long), torch.zeros(0, dtype=torch.long))])
    ind.rows_all = ind.cols_all = torch.zeros(0, dtype=torch.long)
    ind.counts = (0,)
    with pytest.raises(RuntimeError, match="GPU only"):
        point_loss.class_loss_forward(torch.zeros(1, 4, 5), torch.ones(5), ind.rows_all, ind.cols_all,
                                      torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                                      torch.zeros(0, dtype=torch.long))
