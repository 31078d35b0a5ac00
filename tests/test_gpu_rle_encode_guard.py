"""The RLE encoder writes nothing outside its buffers (tests/checkers/guard.py: the characters, the
offsets, the per-mask block, the totals and the workspace sit between 0xFF guard bands) — at exactly
the needed capacity, at a capacity one short, and through the wrappers — its workspace is exactly
the size the query names, and the guarded run gives the unguarded run's bits.  Both modes, at 23x37
(a plane that is no multiple of a lane's 8 cells) with the checkerboards among the masks."""
import numpy as np
import pytest
import torch

from checkers import guard, rle_encode_cases as rc

pytestmark = pytest.mark.gpu

H, W = 23, 37
IDS = [3, 7, 9]


def _inputs(mode):
    cases = rc.masks_of(H, W)
    assert "checkerboard" in cases and "checkerboard_from_1" in cases
    masks = np.stack(list(cases.values()))
    if mode == "stack":
        return (1, torch.from_numpy(masks).cuda(), None, len(masks), len(masks), H, W)
    maps = torch.from_numpy(np.where(masks > 0, 3, 7)).float().cuda()
    ids = torch.tensor([IDS] * len(masks), dtype=torch.int32).cuda()
    return (0, maps, ids, len(masks), 3 * len(masks), H, W)


@pytest.mark.parametrize("mode", ["labels", "stack"])
def test_raw_call_stays_inside_its_buffers(mode):
    from rgbd_amd import _lib
    args = _inputs(mode)
    free = rc.raw_encode(*args, *rc.capacity(args[0], args[3], args[4], H, W))
    need_counts, need = (int(v) for v in free["totals"].cpu().numpy())
    n = int(free["offsets"][-1])
    assert n == need and not bool(free["info"][:, 7].any())
    for short in (0, 1):                      # exactly the need; one character and one count short
        pool = guard.Pool()
        got = rc.raw_encode(*[pool.place(a) if isinstance(a, torch.Tensor) else a for a in args],
                            need_counts - short, need - short, guard_pool=pool)
        assert pool.check_all() == 5 + (2 if mode == "labels" else 1)   # the outputs and the workspace; the inputs
        assert got["ws"].numel() == _lib.lib().rgbd_rle_encode_workspace_size(args[0], args[3], args[4], H, W,
                                                                               need_counts - short)
        if not short:
            assert torch.equal(got["chars"], free["chars"][:n])
            assert all(torch.equal(got[k], free[k]) for k in ("offsets", "info", "totals"))
        else:
            info = got["info"].cpu().numpy()
            assert info[-1, 7] == 1 and not info[:-1, 7].any()
            assert np.array_equal(info[:, [0, 2, 3, 4, 5, 6]], free["info"].cpu().numpy()[:, [0, 2, 3, 4, 5, 6]])
            kept = int(got["offsets"][-1])
            assert kept == int(free["offsets"][-2]) and torch.equal(got["chars"][:kept], free["chars"][:kept])
    pool = guard.Pool()                       # one character short with every count in place
    got = rc.raw_encode(*[pool.place(a) if isinstance(a, torch.Tensor) else a for a in args], need_counts, need - 1,
                        guard_pool=pool)
    pool.check_all()
    assert got["info"][:, 7].tolist() == [0] * (args[4] - 1) + [2]
    assert got["totals"].tolist() == [need_counts, need]


@pytest.mark.parametrize("mode", ["labels", "stack"])
def test_wrappers_stay_inside_their_buffers(mode):
    from rgbd_amd import _lib, export
    args = _inputs(mode)
    call = (lambda **kw: export.encode_mask_stack(args[1], **kw)) if mode == "stack" else \
        (lambda **kw: export.encode_segments_batch(args[1], [IDS] * args[3], **kw))
    want = call()
    need = sum(len(r["counts"]) for r, _, _ in (want if mode == "stack" else [e for img in want for e in img]))
    cap_counts = rc.capacity(args[0], args[3], args[4], H, W)[0]
    for cap, buffers in ((need, 3), (need - 1, 5)):   # head, characters, workspace; the repeated call's head and characters
        with guard.guarded_allocations() as sw:
            got = call(cap_chars=cap)
            n = sw.check_all()
            assert sw.passed_through == 0
            sizes = sorted(int(t.numel()) for t in sw.workspaces().values())
        assert got == want and n == buffers
        assert sizes == [max(256, _lib.lib().rgbd_rle_encode_workspace_size(args[0], args[3], args[4], H, W,
                                                                           cap_counts))]
