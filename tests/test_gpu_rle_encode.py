"""The COCO RLE encoder on the device (csrc/rle_encode.hip, rgbd_amd/export.py)
against the oracle (oracle/rle.py: maskApi.c restated).  Everything is bit for bit: no tolerances.
Sizes: 24x40, 23x37, 97x131 as in test_gpu_json_import.py, 128x160 for four-character counts, and
97 x the smallest width that holds two workgroup steps for the chunk edges."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from checkers import rle_encode_cases as rc
from oracle import rle

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden"
SIZES = rc.SIZES
IDS = lambda s: f"{s[0]}x{s[1]}"  # noqa: E731


@pytest.fixture(scope="module")
def export():
    from rgbd_amd import export
    return export


@pytest.fixture(scope="module")
def chunk():
    from rgbd_amd import _lib
    return _lib.lib().rgbd_rle_encode_chunk()


def _check(got, masks, names):
    assert len(got) == len(masks)
    for name, m, (r, bbox, area) in zip(names, masks, got):
        counts, want_bbox, want_area = rc.expected(m)
        assert r["size"] == list(m.shape), name
        assert r["counts"] == counts, name
        assert bbox == want_bbox and area == want_area, name


def _label_cases(masks, dtype):
    """One map per mask: id 3 where the mask is set over a background that names id 7 (float32:
    -1, which names nothing, on every other row of it) -> ids [3, 7, 9]: the mask, most of its
    complement, an id no cell holds."""
    arr = np.stack(masks).astype(np.int64)
    maps = np.where(arr > 0, 3, 7)
    if dtype == torch.float32:
        maps = maps.astype(np.float32)
        maps[:, 1::2][arr[:, 1::2] == 0] = -1.0
    want = [[(mp == i).astype(np.uint8) for i in (3, 7, 9)] for mp in maps]
    return torch.from_numpy(maps).to(dtype).cuda(), want


# ------------------------------------------------------------------ the two modes against the oracle
@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_stack_mode_is_the_oracle(export, size):
    cases = rc.masks_of(*size)
    masks = list(cases.values())
    if size == (128, 160):
        assert len(rc.expected(cases["all_zero"])[0]) == 4          # 20480 >= 16384: a four-character count
    got = export.encode_mask_stack(torch.from_numpy(np.stack(masks)).cuda())
    _check(got, masks, list(cases))
    as_bool = export.encode_mask_stack(torch.from_numpy(np.stack(masks) * 200).cuda())   # set where non-zero
    assert as_bool == got


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32], ids=["f32", "i32"])
@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_label_map_mode_is_the_oracle(export, size, dtype):
    cases = rc.masks_of(*size)
    maps, want = _label_cases(list(cases.values()), dtype)
    got = export.encode_segments_batch(maps, [[3, 7, 9]] * len(cases))
    for name, g, w in zip(cases, got, want):
        _check(g, w, [f"{name}/{i}" for i in (3, 7, 9)])
        assert g[2][1] is None and g[2][2] == 0 and g[2][0]["counts"] == rle.rle_to_string([size[0] * size[1]])


@pytest.mark.parametrize("mode", ["stack", "f32", "i32"])
def test_runs_around_the_chunk_edges(export, chunk, mode):
    cases = rc.chunk_masks(chunk)
    h, w = rc.CHUNK_H, rc.chunk_width(chunk)
    assert h * w >= 2 * chunk + 2 > h * (w - 1)
    masks = list(cases.values())
    ends = {n: rle.rle_from_string(rc.expected(m)[0])[:2] for n, m in cases.items()}
    assert ends["ones_to_chunk-1"] == [0, chunk - 1] and ends["zeros_to_chunk+1"][0] == chunk + 1
    assert ends["span_2chunk+1"] == [1, 2 * chunk + 1]
    if mode == "stack":
        _check(export.encode_mask_stack(torch.from_numpy(np.stack(masks)).cuda()), masks, list(cases))
    else:
        maps, want = _label_cases(masks, torch.float32 if mode == "f32" else torch.int32)
        for name, g, wm in zip(cases, export.encode_segments_batch(maps, [[3, 7, 9]] * len(cases)), want):
            _check(g, wm, [f"{name}/{i}" for i in (3, 7, 9)])


# ------------------------------------------------------------------ label maps
def _float_map(h, w, n_seg, seed):
    m = rc.label_map(h, w, n_seg, seed).astype(np.float32)
    rng = np.random.RandomState(seed + 1)
    for v in (0.5, np.nan, 256.0, 2.5, -0.0, 1e9, -np.inf):      # -0.0 == 0: it names id 0
        m[rng.randint(0, h, 6), rng.randint(0, w, 6)] = v
    return m


@pytest.mark.parametrize("size", SIZES[:3], ids=IDS)
def test_float_map_cells_that_name_nothing(export, size):
    h, w = size
    m = _float_map(h, w, 9, seed=h)
    assert np.isnan(m).any() and (m == 0.5).any() and (m == 256.0).any()
    ids = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 255]
    got = export.encode_segments(torch.from_numpy(m).cuda(), ids)
    _check(got, [(m == i).astype(np.uint8) for i in ids], [f"id {i}" for i in ids])
    assert got[0][2] > 0                                           # the -0.0 cells


@pytest.mark.parametrize("size", SIZES[:3], ids=IDS)
def test_int_map_with_zero_background(export, size):
    h, w = size
    m = rc.label_map(h, w, 9, seed=h + 3, background=0)
    m[0, 0], m[h - 1, w - 1] = 300, -4                             # outside [0, 256): they name nothing
    ids = [0, 3, 1, 9, 200]                                        # the background itself, and an absent id
    got = export.encode_segments(torch.from_numpy(m).to(torch.int32).cuda(), ids)
    _check(got, [(m == i).astype(np.uint8) for i in ids], [f"id {i}" for i in ids])
    assert got[-1][1] is None and got[-1][2] == 0
    small = export.encode_segments(torch.from_numpy(np.clip(m, 0, 255)).to(torch.uint8).cuda(), ids)
    _check(small, [(np.clip(m, 0, 255) == i).astype(np.uint8) for i in ids], [f"u8 id {i}" for i in ids])


def test_padding_and_duplicates_in_the_id_table(export):
    """The raw call: -1 slots yield 0 counts, 0 characters, area 0; a duplicated id yields its
    string twice; both inside one table row."""
    h, w = 23, 37
    m = rc.label_map(h, w, 5, seed=2, background=0)
    maps = torch.from_numpy(m[None]).to(torch.int32).cuda()
    table = [[2, -1, 2, 5, -1, 0, 2]]
    ids = torch.tensor(table, dtype=torch.int32).cuda()
    cap = (7 * (h * w + 1), 7 * (h * w + 1))
    raw = rc.raw_encode(0, maps, ids, 1, 7, h, w, *cap)
    info, strings = raw["info"].cpu().numpy(), rc.strings_of(raw)
    for j, i in enumerate(table[0]):
        if i < 0:
            assert info[j].tolist() == [0, 0, 0, 0, 0, -1, -1, 0] and strings[j] == ""
        else:
            counts, bbox, area = rc.expected((m == i).astype(np.uint8))
            assert strings[j] == counts and info[j, 2] == area and info[j, 7] == 0
            assert info[j, 0] == len(rle.rle_from_string(counts)) and info[j, 1] == len(counts)
            assert bbox is not None and [float(info[j, 3]), float(info[j, 4]), float(info[j, 5] - info[j, 3] + 1),
                                         float(info[j, 6] - info[j, 4] + 1)] == bbox
    tot = raw["totals"].cpu().numpy()
    assert tot[0] == info[:, 0].sum() and tot[1] == info[:, 1].sum() == raw["offsets"].cpu().numpy()[-1]
    got = export.encode_segments(maps[0], [2, 2, 5, 2])
    assert got[0] == got[1] == got[3] and got[0][0]["counts"] == strings[0]


def test_255_segments_in_one_map(export):
    h, w = 97, 131
    rng = np.random.RandomState(7)
    m = (np.arange(h * w).reshape(h, w) // 8 % 255 + 1)           # 8-pixel dashes, every id many runs
    m[rng.rand(h, w) < 0.1] = 0
    ids = list(range(1, 256))
    got = export.encode_segments(torch.from_numpy(m).float().cuda(), ids)
    _check(got, [(m == i).astype(np.uint8) for i in ids], [f"id {i}" for i in ids])


def test_batched_is_single_and_a_second_run_is_bitwise_equal(export):
    h, w = 97, 131
    maps = np.stack([rc.label_map(h, w, n, seed=n) for n in (12, 3, 30)]).astype(np.float32)
    ids = [list(range(1, 13)), [3, 1], list(range(30, 0, -1))]     # B = 3, different id counts
    dev = torch.from_numpy(maps).cuda()
    batch = export.encode_segments_batch(dev, ids)
    assert [len(b) for b in batch] == [12, 2, 30]
    for b in range(3):
        assert batch[b] == export.encode_segments(dev[b], ids[b])
        _check(batch[b], [(maps[b] == i).astype(np.uint8) for i in ids[b]], [f"{b}/{i}" for i in ids[b]])
    assert export.encode_segments_batch(list(dev), ids) == batch   # a list of maps
    table = np.full((3, 30), -1, np.int32)
    for b, row in enumerate(ids):
        table[b, :len(row)] = row
    t = torch.from_numpy(table).cuda()
    cap = rc.capacity(0, 3, 90, h, w)
    one, two = (rc.raw_encode(0, dev, t, 3, 90, h, w, *cap) for _ in range(2))
    n = int(one["offsets"][-1])
    assert n > 0 and torch.equal(one["chars"][:n], two["chars"][:n])
    assert all(torch.equal(one[k], two[k]) for k in ("offsets", "info", "totals"))
    assert int(one["totals"][0]) <= cap[0] and int(one["totals"][1]) <= cap[1]


# ------------------------------------------------------------------ round trips
@pytest.mark.parametrize("size", SIZES[1:3], ids=IDS)
def test_round_trips_through_the_decoder(export, size):
    from rgbd_amd import _lib, json_results
    from rgbd_amd.ops import _p, _stream
    h, w = size
    masks = np.stack(list(rc.masks_of(h, w).values()))
    dev = torch.from_numpy(masks).cuda()
    enc = export.encode_mask_stack(dev)
    assert torch.equal(json_results.decode_masks([r for r, _, _ in enc]), dev.bool())
    # on the device: chars / offsets of the encoder straight into rgbd_rle_stack
    N = len(masks)
    cap = rc.capacity(1, N, N, h, w)
    raw = rc.raw_encode(1, dev, None, N, N, h, w, *cap)
    rest = np.concatenate([np.tile([h, w], N), np.ones(N), np.full(2 * N, -1), [0, N]]).astype(np.int32)
    meta_dev = torch.cat([raw["offsets"], torch.from_numpy(rest).cuda()])           # no host in between
    meta_host = meta_dev.cpu().numpy()                                              # the host's copy, for validation
    L = _lib.lib()
    n_chars = int(meta_host[N])
    out = torch.empty((N, h, w), dtype=torch.uint8, device="cuda")
    info = torch.empty((N, 4), dtype=torch.int32, device="cuda")
    ws = torch.empty((L.rgbd_rle_workspace_size(N, n_chars, 0, h, w),), dtype=torch.uint8, device="cuda")
    assert L.rgbd_rle_stack(_p(raw["chars"]), meta_host.ctypes.data, _p(meta_dev), N, h, w, _p(out), _p(info), _p(ws),
                            _stream(out.device)) == 0
    assert torch.equal(out, dev) and not bool(info[:, 1].any())
    assert info[:, 0].tolist() == raw["info"][:, 0].tolist()                        # the same number of counts


# ------------------------------------------------------------------ the JSON builders, switch on against off
def _both(export, monkeypatch, fn, *args):
    calls = {"n": 0}
    for name in ("encode_segments", "encode_mask_stack"):
        orig = getattr(export, name)

        def spy(*a, _orig=orig, **kw):
            calls["n"] += 1
            return _orig(*a, **kw)
        monkeypatch.setattr(export, name, spy)
    monkeypatch.setattr(export, "HIP_RLE_ENCODE", False)
    off = fn(*args)
    assert calls["n"] == 0
    monkeypatch.setattr(export, "HIP_RLE_ENCODE", True)
    on = fn(*args)
    monkeypatch.undo()
    return on, off, calls["n"]


@pytest.mark.parametrize("size", SIZES[:3], ids=IDS)
def test_prediction_to_json_switch_on_equals_off(export, monkeypatch, size):
    h, w = size
    m = _float_map(h, w, 9, seed=h)
    info = [{"id": i, "label_id": i % 4, "score": 0.25 + i / 100} for i in (4, 1, 11, 9, 2, 0)]   # 11: no pixels
    pred = {"segmentation": torch.from_numpy(m).cuda(), "segments_info": info}
    for original in (None, (2 * h, 3 * w)):
        on, off, n = _both(export, monkeypatch, export.prediction_to_json, pred, original)
        assert n == 1 and json.dumps(on, indent=2) == json.dumps(off, indent=2)
        assert len(on["masks"]) == sum(bool((m == s["id"]).any()) for s in info) < len(info)
        assert on["masks"][0]["size"] == list(original or size)
    pred_i = {"segmentation": torch.from_numpy(rc.label_map(h, w, 6, 1, background=0)).to(torch.int32).cuda(),
              "segments_info": info}
    on, off, n = _both(export, monkeypatch, export.prediction_to_json, pred_i, None)
    assert n == 1 and json.dumps(on) == json.dumps(off)
    # what stays on the torch path: CPU tensors, ids past 255, no segments
    for p in ({"segmentation": pred["segmentation"].cpu(), "segments_info": info},
              {"segmentation": pred["segmentation"], "segments_info": info + [{"id": 256, "label_id": 1}]},
              {"segmentation": pred["segmentation"], "segments_info": []}):
        on, off, n = _both(export, monkeypatch, export.prediction_to_json, p, None)
        assert n == 0 and on == off


@pytest.mark.parametrize("size", SIZES[:3], ids=IDS)
def test_gt_label_to_json_switch_on_equals_off(export, monkeypatch, size):
    h, w = size
    masks = np.stack(list(rc.masks_of(h, w).values())[:8])
    ids = [3, 0, 5, -1, 7, 7, 2, 9]                                 # ids <= 0 and the empty mask are skipped
    for stack in (torch.from_numpy(masks).cuda(), torch.from_numpy(masks * 3).int().cuda(),
                  torch.from_numpy(masks).bool().cuda()):
        on, off, n = _both(export, monkeypatch, export.gt_label_to_json, [stack, ids], None)
        assert n == 1 and json.dumps(on) == json.dumps(off) and len(on["masks"]) == 5
    gt_map = torch.from_numpy(rc.label_map(h, w, 7, 5, background=0)).to(torch.int32).cuda()
    on, off, n = _both(export, monkeypatch, export.gt_label_to_json, [gt_map, None], (h, w))
    assert n == 1 and json.dumps(on) == json.dumps(off) and on["labels"]
    on, off, n = _both(export, monkeypatch, export.gt_label_to_json, [gt_map + 300, None], None)   # ids past 255
    assert n == 0 and on == off
    on, off, n = _both(export, monkeypatch, export.gt_label_to_json, [gt_map.cpu(), None], None)
    assert n == 0 and on == off


def test_g12_load_cases_export_the_same_either_way(export, monkeypatch, tmp_path):
    """Every G12 load case that loads: import on the device, export with the switch on and off,
    and the files the writer leaves are the same bytes."""
    from rgbd_amd import json_results
    g = np.load(GOLDEN / "g12_json_import.npz")
    loaded = []
    for k in range(len(g["names"])):
        got = json_results.load_json_prediction(json.loads(str(g[f"l{k}_json"])), g[f"l{k}_shape"].tolist())
        if got is not None:
            loaded.append(got)
    assert len(loaded) >= 3
    for got in loaded:
        on, off, n = _both(export, monkeypatch, export.prediction_to_json, got, None)
        assert n == 1 and json.dumps(on) == json.dumps(off)
    names = [f"im{k}" for k in range(len(loaded))]
    monkeypatch.setattr(export, "HIP_RLE_ENCODE", True)
    a = export.convert_predictions_to_json(loaded, names, tmp_path / "on")
    monkeypatch.setattr(export, "HIP_RLE_ENCODE", False)
    b = export.convert_predictions_to_json(loaded, names, tmp_path / "off")
    assert [p.read_bytes() for p in a] == [p.read_bytes() for p in b]


# ------------------------------------------------------------------ capacity: the status bit and the retry
def _count_reads(monkeypatch):
    reads = {"n": 0}
    for name in ("cpu", "item", "tolist", "numpy", "__bool__", "__int__", "__float__", "__index__"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, **kw):
            if self.is_cuda:
                reads["n"] += 1
            return _orig(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, counted)
    return reads


@pytest.mark.parametrize("mode", ["labels", "stack"])
def test_a_capacity_one_below_the_need(export, monkeypatch, mode):
    h, w = 97, 131
    m = rc.label_map(h, w, 20, seed=4)
    ids = list(range(1, 21))
    if mode == "labels":
        src, table = torch.from_numpy(m[None]).float().cuda(), torch.tensor([ids], dtype=torch.int32).cuda()
        args, call = (0, src, table, 1, 20, h, w), lambda **kw: export.encode_segments(src[0], ids, **kw)
    else:
        src = torch.from_numpy(np.stack([m == i for i in ids]).astype(np.uint8)).cuda()
        args, call = (1, src, None, 20, 20, h, w), lambda **kw: export.encode_mask_stack(src, **kw)
    cap_counts, cap_chars = rc.capacity(args[0], args[3], args[4], h, w)
    full = rc.raw_encode(*args, cap_counts, cap_chars)
    need_counts, need = (int(v) for v in full["totals"].cpu().numpy())
    assert not bool(full["info"][:, 7].any()) and need == int(full["offsets"][-1]) and 0 < need < cap_chars
    exact = rc.raw_encode(*args, need_counts, need)                # exactly the need: everything fits
    assert torch.equal(exact["chars"], full["chars"][:need]) and torch.equal(exact["info"], full["info"])
    short = rc.raw_encode(*args, cap_counts, need - 1)
    info = short["info"].cpu().numpy()
    assert info[-1, 7] == 2 and not info[:-1, 7].any()            # the last mask is the one that does not fit
    assert short["totals"].cpu().numpy().tolist() == [need_counts, need]
    off_s, off_f = short["offsets"].cpu().numpy(), full["offsets"].cpu().numpy()
    assert off_s[:-1].tolist() == off_f[:-1].tolist() and off_s[-1] == off_s[-2]
    assert torch.equal(short["chars"][:off_s[-1]], full["chars"][:off_s[-1]])
    assert np.array_equal(info[:, :7], full["info"].cpu().numpy()[:, :7])
    fewer = rc.raw_encode(*args, need_counts - 1, cap_chars)       # the counts of the last mask do not fit
    info = fewer["info"].cpu().numpy()
    assert info[-1, 7] == 1 and not info[:-1, 7].any() and int(fewer["totals"][0]) == need_counts
    assert int(fewer["totals"][1]) == need - int(full["info"][-1, 1]) == int(fewer["offsets"][-1])
    # the wrapper: two host reads; with the capacity one short, one more for the repeated call
    reads = _count_reads(monkeypatch)
    want = call()
    assert reads["n"] == 2
    reads["n"] = 0
    got = call(cap_chars=need - 1)
    monkeypatch.undo()
    assert reads["n"] == 3 and got == want
    assert [r["counts"] for r, _, _ in want] == rc.strings_of(full)


def test_batched_reads_do_not_grow_with_the_number_of_masks(export, monkeypatch):
    h, w = 24, 40
    maps = torch.from_numpy(np.stack([rc.label_map(h, w, 40, seed=s) for s in range(6)])).float().cuda()
    reads = _count_reads(monkeypatch)
    out = export.encode_segments_batch(maps, [list(range(1, 41))] * 6)
    monkeypatch.undo()
    assert reads["n"] == 2 and sum(len(o) for o in out) == 240


def test_refusals(export):
    m = torch.zeros((24, 40), dtype=torch.float32)
    with pytest.raises(RuntimeError, match="GPU only"):
        export.encode_segments(m, [1])
    with pytest.raises(RuntimeError, match="GPU only"):
        export.encode_mask_stack(torch.zeros((1, 24, 40), dtype=torch.uint8))
    with pytest.raises(ValueError, match="segment ids"):
        export.encode_segments(m.cuda(), [1, 256])
    with pytest.raises(ValueError, match="dtype"):
        export.encode_segments(m.cuda().double(), [1])
    with pytest.raises(ValueError, match="id lists"):
        export.encode_segments_batch(m.cuda()[None], [[1], [2]])
    assert export.encode_segments(m.cuda(), []) == []
    assert export.encode_mask_stack(torch.zeros((0, 24, 40), dtype=torch.uint8, device="cuda")) == []
