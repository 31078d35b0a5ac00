"""Deterministic mode, the parts that need no GPU: the switch (rgbd_amd/determinism.py), the numpy
restatement of the ordered segment sum (tests/checkers/ordered_scatter.py) against float64, and
the C-ABI table."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pathlib import Path

from checkers import ordered_scatter as osc
from rgbd_amd import _lib, determinism

REPO = Path(__file__).resolve().parents[1]


@pytest.fixture
def clean_switch():
    """Every test starts from the unset state with torch's flag off, and leaves both as found."""
    state, flag = determinism.get_state(), torch.are_deterministic_algorithms_enabled()
    determinism.set_deterministic(None)
    torch.use_deterministic_algorithms(False)
    yield
    determinism.set_deterministic(state)
    torch.use_deterministic_algorithms(flag)


def test_switch_is_tri_state(clean_switch):
    assert determinism.get_state() is None and determinism.is_deterministic() is False
    determinism.set_deterministic(True)
    assert determinism.get_state() is True and determinism.is_deterministic() is True
    determinism.set_deterministic(False)
    assert determinism.get_state() is False and determinism.is_deterministic() is False
    determinism.set_deterministic(None)
    assert determinism.get_state() is None
    with pytest.raises(TypeError):
        determinism.set_deterministic(1)


def test_switch_follows_torch_only_when_unset(clean_switch):
    torch.use_deterministic_algorithms(True)
    assert determinism.is_deterministic() is True       # unset: torch's flag decides
    determinism.set_deterministic(False)
    assert determinism.is_deterministic() is False      # set: torch's flag is not consulted
    torch.use_deterministic_algorithms(False)
    determinism.set_deterministic(True)
    assert determinism.is_deterministic() is True
    determinism.set_deterministic(None)
    assert determinism.is_deterministic() is False


def test_context_manager_restores_previous_state(clean_switch):
    for before in (None, True, False):
        determinism.set_deterministic(before)
        with determinism.deterministic():
            assert determinism.is_deterministic() is True
            with determinism.deterministic(False):
                assert determinism.is_deterministic() is False
            assert determinism.get_state() is True
        assert determinism.get_state() is before
        with pytest.raises(RuntimeError):
            with determinism.deterministic(True):
                raise RuntimeError("leaves through an exception")
        assert determinism.get_state() is before


@pytest.mark.parametrize("env,want", [("1", "True True"), ("0", "False False"), (None, "None False")])
def test_environment_variable_sets_initial_state(env, want):
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import _rgbd_import; "
            "from rgbd_amd import determinism as d; print(d.get_state(), d.is_deterministic())")
    e = {k: v for k, v in os.environ.items() if k != "RGBD_DETERMINISTIC"}
    if env is not None:
        e["RGBD_DETERMINISTIC"] = env
    out = subprocess.run([sys.executable, "-c", code, str(REPO)], env=e, capture_output=True, text=True, check=True)
    assert out.stdout.strip() == want


def _random_segments(rng, lengths, ntaps_extra, D):
    """Unsorted taps for destinations of the given segment lengths plus sentinel taps."""
    ndest = len(lengths)
    keys = np.concatenate([np.full(n, d) for d, n in enumerate(lengths)] + [np.full(ntaps_extra, ndest)])
    keys = keys[rng.permutation(keys.size)].astype(np.int32)
    coef = (rng.standard_normal(keys.size) * np.exp(rng.uniform(-6, 6, keys.size))).astype(np.float32)
    rows = None if D is None else rng.standard_normal((keys.size, D)).astype(np.float32)
    return keys, coef, rows


@pytest.mark.parametrize("D", [None, 16], ids=["scalar", "rows"])
def test_restatement_against_float64(D):
    """The float32 restatement against np.add.at in float64: per element within
    (n + 2) 2^-24 sum|terms| (n the segment length: one rounding per product, at most n per
    running sum of n terms and its partials), exactly +0 for the empty segment, and the chunked
    order really taken for the segment longer than two chunks."""
    rng = np.random.default_rng(7)
    lengths = [0, 1, 5, osc.CH, osc.CH + 1, 2 * osc.CH + 37, 3, 0, 64]
    keys, coef, rows = _random_segments(rng, lengths, 29, D)
    order = np.argsort(keys, kind="stable")
    skeys, sidx = keys[order], order
    got = osc.ordered_scatter(skeys, sidx, coef, len(lengths), rows=rows)
    assert got.dtype == np.float32
    assert list(osc.segment_lengths(skeys, len(lengths))) == lengths
    live = keys < len(lengths)
    terms = coef.astype(np.float64) if rows is None else coef.astype(np.float64)[:, None] * rows.astype(np.float64)
    want = np.zeros(got.shape, np.float64)
    mag = np.zeros(got.shape, np.float64)
    np.add.at(want, keys[live], terms[live])
    np.add.at(mag, keys[live], np.abs(terms[live]))
    n = np.asarray(lengths, np.float64).reshape((-1,) + (1,) * (got.ndim - 1))
    bound = (n + 2) * 2.0 ** -24 * mag
    assert (np.abs(got - want) <= bound).all(), float((np.abs(got - want) / np.maximum(bound, 1e-300)).max())
    for d in (0, 7):
        assert not got[d].any() and not np.signbit(got[d]).any()
    # the long segment by hand: chunks of CH from the segment start, partials added in chunk order
    d = 5
    t = coef[sidx[skeys == d]] if rows is None else coef[sidx[skeys == d]][:, None] * rows[sidx[skeys == d]]
    total = np.zeros(t.shape[1:], np.float32)
    for c0 in range(0, len(t), osc.CH):
        part = np.zeros(t.shape[1:], np.float32)
        for x in t[c0:c0 + osc.CH]:
            part = part + x
        total = total + part
    assert np.array_equal(got[d], total)
    flat = np.zeros(t.shape[1:], np.float32)
    for x in t:
        flat = flat + x
    assert not np.array_equal(flat, total), "chunking changed nothing: the case does not pin the order"


def test_restatement_keeps_ascending_tap_order():
    """Within a destination the taps are added in ascending tap index (what the stable sort
    keeps): 2^24 + 1 + 1 differs from 1 + 1 + 2^24 in float32."""
    keys = np.array([0, 0, 0, 1, 1, 1], np.int32)
    coef = np.array([2.0 ** 24, 1, 1, 1, 1, 2.0 ** 24], np.float32)
    got = osc.ordered_scatter(keys, np.arange(6), coef, 2)
    assert got.tolist() == [2.0 ** 24, 2.0 ** 24 + 2]


def test_msda_launch_groups(monkeypatch):
    """Whole images per deterministic launch group: capped by MSDA_DET_MAX_TAPS, never below one
    image, and a single image beyond the int32 tap index is refused."""
    from rgbd_amd import ops
    S, NH, Q, L, P = 1580, 8, 1580, 3, 4
    per_image = NH * Q * L * P * 4
    assert ops.MSDA_DET_MAX_TAPS == 1 << 27
    assert ops._msda_det_group(8, S, NH, Q, L, P) == 8
    assert ops._msda_det_group(1000, S, NH, Q, L, P) == (1 << 27) // per_image
    monkeypatch.setattr(ops, "MSDA_DET_MAX_TAPS", 3 * per_image - 1)
    assert ops._msda_det_group(8, S, NH, Q, L, P) == 2
    monkeypatch.setattr(ops, "MSDA_DET_MAX_TAPS", 5)
    assert ops._msda_det_group(8, S, NH, Q, L, P) == 1
    big_q = ((1 << 31) - 2) // (NH * L * P * 4) + 1
    with pytest.raises(ValueError):
        ops._msda_det_group(1, S, NH, big_q, L, P)
    assert ops._msda_det_group(4, S, NH, big_q - 1, L, P) == 1


def test_new_entry_points_are_in_the_ctypes_table():
    for name in ("rgbd_msda_bwd_emit", "rgbd_msda_bwd_gather", "rgbd_point_sample_bwd_emit", "rgbd_ordered_gather"):
        assert name in _lib.SIGNATURES, name
        assert name in _lib.header_symbols(), name
