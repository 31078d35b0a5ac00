"""The RLE decoder writes nothing outside its buffers (tests/checkers/guard.py: the map, the stack,
the per-mask flags and the workspace sit between 0xFF guard bands), its workspace is exactly the
size the query names, and the guarded run gives the unguarded run's bits — so no element is left
unwritten.  At 23x37 (rows that are no multiple of a lane's 4 pixels) and 97x131 (more than one
block per map)."""
import numpy as np
import pytest
import torch

from checkers import guard, json_import_ref as jr
from oracle import rle

pytestmark = pytest.mark.gpu

SIZES = [(23, 37), (97, 131)]


def _file(size, seed):
    h, w = size
    rng = np.random.RandomState(seed)
    shapes = [(h, w), (h, w), (h // 2, w // 2), (2 * h, 2 * w), (17, 29), (h, w)]
    masks = []
    for i, (hh, ww) in enumerate(shapes):
        m = (rng.rand(hh, ww) < 0.5).astype(np.uint8)
        if i % 2:
            m[:, : ww // 3] = 0
        masks.append(rle.encode(m))
    masks.insert(3, rle.encode(np.zeros((h, w), np.uint8)))
    n = len(masks)
    return {"labels": list(range(n)), "scores": [0.5] * n, "masks": masks}


def _ws_sizes(sw):
    return sorted(int(t.numel()) for t in sw.workspaces().values())


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_loader_stays_inside_its_buffers(size):
    from rgbd_amd import _lib, json_results
    files = [_file(size, 1), {"labels": [], "scores": [], "masks": []}, _file(size, 2)]
    want = json_results.load_json_predictions(files, size)
    with guard.guarded_allocations() as sw:
        got = json_results.load_json_predictions(files, size)
        n = sw.check_all()
        assert sw.passed_through == 0
        sizes = _ws_sizes(sw)
    n_masks = sum(len(f["masks"]) for f in files)
    n_chars = sum(len(m["counts"]) for f in files for m in f["masks"])
    n_resized = sum(tuple(m["size"]) != tuple(size) for f in files for m in f["masks"])
    assert n_resized == 6
    most = max(len(rle.rle_from_string(m["counts"])) for f in files for m in f["masks"])
    assert (most > 4096) == (size == (97, 131))  # past 4096 counts the painter searches E in global memory
    assert sizes == [max(256, _lib.lib().rgbd_rle_workspace_size(n_masks, n_chars, n_resized, *size))]
    assert n == 3  # the maps, the flags, the workspace
    assert got[1] is None and want[1] is None
    for g, w, f in zip(got[::2], want[::2], files[::2]):
        assert torch.equal(g["segmentation"], w["segmentation"]) and g["segments_info"] == w["segments_info"]
        assert np.array_equal(g["segmentation"].cpu().numpy(), jr.load_prediction(f, size)[0])


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_decode_masks_stays_inside_its_buffers(size):
    from rgbd_amd import _lib, json_results
    h, w = size
    rng = np.random.RandomState(h)
    masks = [rng.rand(h, w) < p for p in (0.0, 0.02, 0.5, 1.0, 0.5)]
    rles = [rle.encode(m.astype(np.uint8)) for m in masks]
    want = json_results.decode_masks(rles)
    with guard.guarded_allocations() as sw:
        got = json_results.decode_masks(rles)
        n = sw.check_all()
        assert sw.passed_through == 0
        sizes = _ws_sizes(sw)
    n_chars = sum(len(r["counts"]) for r in rles)
    assert sizes == [max(256, _lib.lib().rgbd_rle_workspace_size(len(rles), n_chars, 0, h, w))]
    assert n == 3  # the stack, the flags, the workspace
    assert torch.equal(got, want) and np.array_equal(got.cpu().numpy(), np.stack(masks))
