"""rgbd_pp_semantic and rgbd_pp_panoptic write nothing outside their outputs and the workspace
bytes their size queries ask for (tests/checkers/guard.py: every output, the segment table, both
workspaces and the inputs sit between 0xFF guard bands), and the guarded run gives the bits of
the plain one -- so no output cell is left unwritten and no guard value is read."""
import types

import pytest
import torch

from checkers import guard, panoptic_ref as pr

pytestmark = pytest.mark.gpu


def _flat(results):
    out = []
    for r in results:
        if isinstance(r, dict):
            out.append(r["segmentation"])
        elif isinstance(r, torch.Tensor):
            out.append(r)
        else:
            out += [r.segmentation, r.segmentation_scores]
    return out


@pytest.mark.parametrize("ti", range(len(pr.CASES[0][7])))
def test_dense_postprocessing_stays_inside_its_buffers(ti):
    from rgbd_amd import _lib, postprocess as pp
    cl, ml, fuse, _ = pr.case_inputs("ragged")
    ts = pr.case_targets("ragged", ti)
    B, Q, C1 = cl.shape
    dev = torch.device("cuda", 0)
    cl, ml = torch.as_tensor(cl).to(dev), torch.as_tensor(ml).to(dev)

    def run(c, m):
        outs = types.SimpleNamespace(class_queries_logits=c, masks_queries_logits=m)
        sem = pp.post_process_semantic_segmentation(outs, target_sizes=ts, return_segmentation_scores=True,
                                                    keep_on_device=True)
        pan = pp.post_process_panoptic_segmentation(outs, label_ids_to_fuse=fuse, target_sizes=ts, keep_on_device=True)
        none = pp.post_process_panoptic_segmentation(outs, threshold=1.1, label_ids_to_fuse=fuse, target_sizes=ts,
                                                     keep_on_device=True)
        return _flat(sem) + _flat(pan) + _flat(none), [p["segments_info"] for p in pan]

    with guard.guarded_allocations() as sw:
        got, got_info = run(sw.place(cl), sw.place(ml))
        n = sw.check_all()
        assert sw.passed_through == 0
        sizes = {key[1]: buf.numel() for key, buf in sw.workspaces().items()}
    L = _lib.lib()
    assert sizes == {"postprocess_semantic": L.rgbd_pp_semantic_workspace_size(B, Q, C1),
                     "postprocess_panoptic": L.rgbd_pp_panoptic_workspace_size(B, Q)}
    # inputs 2, workspaces 2, semantic maps and scores 2 B, panoptic maps B + table, twice
    assert n >= 2 + 2 + 2 * B + 2 * (B + 1)
    want, want_info = run(cl, ml)
    assert got_info == want_info and len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(
            a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), f"output {i} differs"
