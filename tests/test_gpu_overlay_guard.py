"""rgbd_overlay_blend and rgbd_overlay_lut write nothing outside their outputs (tests/checkers/
guard.py: the image, the map, the table and the output sit between 0xFF guard bands, at every byte
offset of the sweep), and the guarded run gives the bits of the plain one — so no output byte is
left unwritten and no guard value is read."""
import numpy as np
import pytest
import torch

from checkers import guard, overlay_cases as oc, overlay_ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", oc.DTYPES)
@pytest.mark.parametrize("off", oc.OFFSETS)
@pytest.mark.parametrize("shape", oc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_blend_stays_inside_its_buffers(shape, off, dtype):
    rgb, seg, lut, want = oc.case(shape, dtype)
    dev = torch.device("cuda", torch.cuda.current_device())
    pool = guard.Pool()
    got, lead = oc.run_raw(rgb, seg, lut, oc.ALPHA, off,
                           alloc=lambda n: pool.new((n,), torch.uint8, dev, tag=f"{n} bytes").payload)
    assert pool.check_all() == 3           # image, map, output: every guard byte intact
    assert (lead == 0xA5).all()            # and the bytes between a payload's start and the offset view
    plain, _ = oc.run_raw(rgb, seg, lut, oc.ALPHA, off)
    assert np.array_equal(got, plain) and np.array_equal(got, want)


@pytest.mark.parametrize("color_by", ["label", "id"])
def test_wrappers_stay_inside_their_buffers(color_by):
    """The wrappers' own allocations (the table, the output image) under guarded_allocations."""
    from rgbd_amd import overlay
    rgb, seg, _, _ = oc.case((3, 33, 129), "f32")
    rng = np.random.RandomState(5)
    B, Q, C = 3, 37, 11
    seg_id = np.full((B, Q), -1, np.int32)
    seg_id[:, ::2] = np.arange(len(range(0, Q, 2)))
    topk = rng.randint(0, Q * C, size=(B, Q)).astype(np.int32)
    pal = np.array(overlay.consistent_colors(7), np.uint8)
    dev = torch.device("cuda", torch.cuda.current_device())

    def run(place):
        lut = overlay.build_lut(place(torch.from_numpy(seg_id).to(dev)), place(torch.from_numpy(topk).to(dev)), C,
                                place(torch.from_numpy(pal).to(dev)), color_by)
        return lut, overlay.blend(place(torch.from_numpy(rgb).to(dev)), place(torch.from_numpy(seg).to(dev)), lut, 0.6)

    with guard.guarded_allocations() as sw:
        lut_g, out_g = run(sw.place)
        n = sw.check_all()
        assert sw.passed_through == 0 and n >= 5 + 2  # five inputs, the table, the image
    lut_p, out_p = run(lambda t: t)
    assert torch.equal(lut_g, lut_p) and torch.equal(out_g, out_p)
    want_lut = overlay_ref.build_lut(seg_id, topk, C, pal, 0 if color_by == "label" else 1, Q)
    assert np.array_equal(lut_p.cpu().numpy(), want_lut)
    assert np.array_equal(out_p.cpu().numpy(), overlay_ref.blend(rgb, seg, want_lut, 0.6))
