"""The segment-matching kernels write nothing outside their outputs (tests/checkers/guard.py: maps,
tables, lists and outputs sit between 0xFF guard bands), and the guarded run gives the bits of the
plain one — so no output cell is left unwritten and no guard value is read."""
from pathlib import Path

import numpy as np
import pytest
import torch

from checkers import guard, match_cases as mc, match_ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ranges", [(5, 7), (100, 256), (256, 256)], ids=lambda r: f"{r[0]}x{r[1]}")
@pytest.mark.parametrize("offs", [(0, 0), (4, 0), (8, 12)], ids=lambda o: f"{o[0]}+{o[1]}")
@pytest.mark.parametrize("shape", mc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_contingency_stays_inside_its_buffers(shape, offs, ranges):
    na, nb = ranges
    a, b, want = mc.contingency_case(shape, ranges, ("f32", "i32"), "noise")
    dev = torch.device("cuda", torch.cuda.current_device())
    pool = guard.Pool()
    got, lead = mc.run_contingency_raw(a, b, na, nb, *offs,
                                       alloc=lambda n: pool.new((n,), torch.uint8, dev, tag=f"{n} bytes").payload)
    assert pool.check_all() == 3           # the two maps and the table: every guard byte intact
    assert (lead == 0xA5).all()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("P,G", [(0, 0), (1, 7), (7, 1), (100, 100)])
def test_match_stays_inside_its_buffers(P, G):
    counts, a_list, b_list, hw = mc.table_case(P, G)
    dev = torch.device("cuda", torch.cuda.current_device())
    pool = guard.Pool()
    got, _ = mc.run_match_raw(counts, a_list, b_list, hw, 0.0, place=lambda t: pool.place(t.to(dev)),
                              new=lambda shape: pool.new(shape, torch.int32, dev, tag=f"out {shape}").payload)
    assert pool.check_all() == 6
    for g, w in zip(got, match_ref.greedy_match(counts, a_list, b_list, 0.0)):
        assert np.array_equal(g, w)


def test_wrappers_stay_inside_their_buffers():
    """The wrappers' own allocations (table, lists, match arrays, colour tables, image) under
    guarded_allocations: the whole G11 batch at threshold 0.5, and one tracking step."""
    from rgbd_amd import overlay
    g11 = np.load(Path(__file__).parent / "golden" / "g11_match.npz")
    ks = [k for k in range(8) if float(g11[f"c{k}_thr"]) == 0.5]
    dev = torch.device("cuda", torch.cuda.current_device())
    image = torch.from_numpy(g11["image"]).to(dev)
    rng = np.random.RandomState(8)
    Q = 9
    cur = rng.randint(-1, Q, size=(2, 5, 33)).astype(np.float32)
    prev = np.roll(cur, 1, axis=2)
    prev_track = rng.permutation(2 * Q).astype(np.int32).reshape(2, Q)
    ids = np.tile(np.arange(Q, dtype=np.int32), (2, 1))

    def run(place):
        preds = [{"segmentation": place(torch.from_numpy(g11[f"c{k}_pred"]).to(dev)),
                  "segments_info": [{"id": int(i)} for i in g11[f"c{k}_pred_ids"]]} for k in ks]
        gts = [{"segmentation": place(torch.from_numpy(g11[f"c{k}_gt"]).to(dev)),
                "segments_info": [{"id": int(i)} for i in g11[f"c{k}_gt_ids"]]} for k in ks]
        colors = [{int(i): tuple(int(v) for v in c) for i, c in zip(g11[f"c{k}_color_ids"], g11[f"c{k}_color_rgb"])}
                  for k in ks]
        imgs = place(image[None].expand(len(ks), -1, -1, -1).contiguous())
        out = overlay.consistent_prediction_overlay(imgs, preds, colors, gts, alpha=0.6)
        d = lambda x: place(torch.from_numpy(x).to(dev))
        counts = overlay.label_contingency(d(cur), d(prev), Q, Q)
        matched, _, _ = overlay.greedy_iou_match(counts, d(ids), d(ids), cur[0].size, 0.25)
        nxt = d(np.array([40, 50], np.int32))
        track = overlay.track_assign(counts, matched, d(prev_track), nxt)
        return out, track, nxt, overlay.track_lut(track, [(1, 2, 3), (4, 5, 6), (7, 8, 9)])

    with guard.guarded_allocations() as sw:
        guarded = run(sw.place)
        n = sw.check_all()
        assert sw.passed_through == 0 and n >= 2 * len(ks) + 1 + 6  # the inputs placed, and what the wrappers made
    plain = run(lambda t: t)
    for g, p in zip(guarded, plain):
        assert torch.equal(g, p)
    for row, k in zip(plain[0], ks):
        assert np.array_equal(row.cpu().numpy(), g11[f"c{k}_overlays"][0])
    want_t, want_n = match_ref.track_step(cur, prev, prev_track, np.array([40, 50], np.int32), Q, 0.25)
    assert np.array_equal(plain[1].cpu().numpy(), want_t) and np.array_equal(plain[2].cpu().numpy(), want_n)
