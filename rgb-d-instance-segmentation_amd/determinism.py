"""The deterministic-mode switch.

With the mode on, the two value-gradient scatters that otherwise sum with float atomics — the
MSDA backward (csrc/msda.hip) and the point-sample backward (csrc/point_loss.hip) — are computed
by an emit pass, a stable sort and a per-destination sum in an order fixed by the inputs
(csrc/ordered_gather.hpp), and the class loss, where it still runs on torch
(point_loss.HIP_CLASS_LOSS off; csrc/class_loss.hip is atomic-free in any mode), takes ATen's
atomic-free 1-d NLL kernel: two training steps from the same state, seeds and inputs then give
the same bits.

The state is tri-state.  ``None`` (the initial value) follows
``torch.are_deterministic_algorithms_enabled()``; ``RGBD_DETERMINISTIC=1`` / ``=0`` in the
environment starts the process at ``True`` / ``False``; ``set_deterministic`` and the
``deterministic`` context manager set it.  The autograd Functions read the switch in ``forward``
and keep it on ``ctx``, so a step's backward always runs in the mode of its forward.
"""
import contextlib
import os

import torch

_ENV = os.environ.get("RGBD_DETERMINISTIC", "").strip()
_state = True if _ENV == "1" else False if _ENV == "0" else None


def set_deterministic(flag):
    """True / False: force the mode on / off; None: follow torch's deterministic-algorithms flag."""
    global _state
    if flag is not None and not isinstance(flag, bool):
        raise TypeError(f"set_deterministic: expected True, False or None, got {flag!r}")
    _state = flag


def get_state():
    """The raw tri-state (True, False or None)."""
    return _state


def is_deterministic() -> bool:
    if _state is None:
        return bool(torch.are_deterministic_algorithms_enabled())
    return _state


@contextlib.contextmanager
def deterministic(flag=True):
    """``with deterministic():`` — the mode set to ``flag`` inside, the previous state (None
    included) restored on the way out."""
    prev = _state
    set_deterministic(flag)
    try:
        yield
    finally:
        set_deterministic(prev)
