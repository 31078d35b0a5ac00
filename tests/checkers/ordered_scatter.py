"""The summation order of the deterministic scatters (csrc/ordered_gather.hpp), restated in numpy
float32.

Given the stably sorted keys, the tap index each sorted position carries, and the coefficients,
destination ``d`` owns the segment of sorted positions whose key is ``d``.  Its terms are
``coef[idx[j]]`` (point-sample gradient) or ``coef[idx[j]] * row[idx[j]]`` (MSDA value gradient:
one float32 product per channel, formed before it is added).  The segment is cut into chunks of
``CH`` = 256 positions at fixed offsets from its start; each chunk is summed in ascending position
starting from +0, and the chunk sums are added in chunk order starting from +0.  Every operation
is one float32 multiply or one float32 add (numpy rounds each like the GPU's separate v_mul_f32 /
v_add_f32; the library is built without FMA contraction).
"""
import numpy as np

CH = 256  # ORDERED_CH of csrc/ordered_gather.hpp


def ordered_scatter(sorted_keys, sorted_idx, coef, ndest, rows=None, ch=CH):
    """-> float32 [ndest] (rows None) or [ndest, D] (rows: float32 [ntaps, D], indexed by tap).
    Keys >= ndest (the sentinel) belong to no destination."""
    keys = np.asarray(sorted_keys).astype(np.int64)
    idx = np.asarray(sorted_idx).astype(np.int64)
    assert keys.ndim == 1 and keys.shape == idx.shape and (np.diff(keys) >= 0).all()
    t = np.asarray(coef, dtype=np.float32)[idx]
    if rows is not None:
        t = t[:, None] * np.asarray(rows, dtype=np.float32)[idx]  # one rounded product per element
    assert t.dtype == np.float32
    dest = np.arange(ndest)
    lo = np.searchsorted(keys, dest, side="left")
    n = np.searchsorted(keys, dest, side="right") - lo
    out = np.zeros((ndest,) + t.shape[1:], dtype=np.float32)
    nmax = int(n.max()) if ndest else 0
    for c0 in range(0, nmax, ch):
        part = np.zeros_like(out)
        for o in range(c0, min(c0 + ch, nmax)):
            sel = np.nonzero(n > o)[0]
            part[sel] = part[sel] + t[lo[sel] + o]
        sel = np.nonzero(n > c0)[0]
        out[sel] = out[sel] + part[sel]
    return out


def segment_lengths(sorted_keys, ndest):
    """Taps per destination (the sentinel excluded)."""
    keys = np.asarray(sorted_keys).astype(np.int64)
    return np.bincount(keys[keys < ndest], minlength=ndest)
