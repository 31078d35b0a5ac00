"""The JSON import on the device (csrc/rle_decode.hip, rgbd_amd/json_results.py) against the oracle
(oracle/rle.py: maskApi.c restated), the numpy checker and the reference's recorded output, G12
(tests/golden/make_json_import_golden.py).  Everything is bit for bit: no tolerances.
Sizes: 24x40, 23x37 and 97x131."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from checkers import json_import_ref as jr
from oracle import rle

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden"
SIZES = [(24, 40), (23, 37), (97, 131)]


@pytest.fixture(scope="module")
def g12():
    return np.load(GOLDEN / "g12_json_import.npz")


@pytest.fixture(scope="module")
def jres():
    from rgbd_amd import json_results
    return json_results


def _names(g, key="names"):
    return [str(n) for n in g[key]]


def _as_rle(counts, size):
    return {"size": list(size), "counts": rle.rle_to_string(counts)}


def _pad_to(counts, total):
    """Close a count list so that it sums to ``total`` (by one more run, or by growing the last)."""
    s = sum(counts)
    assert s <= total
    return counts + [total - s] if s < total else counts


# ------------------------------------------------------------------ the counts stage
def _count_lists(h, w):
    L = h * w
    out = {
        "one_count_all_zero": [L],
        "two_counts_all_one": [0, L],
        "three_counts": [5, 7, L - 12],
        "four_counts": [5, 7, 9, L - 21],               # the first delta-coded count
        "leading_zero": [0, 3, 4, 5, L - 12],
        "zero_runs_in_the_middle": _pad_to([4, 0, 0, 6, 0, 3, 2, 0, 0, 0, 5], L),
        "one_char_counts": _pad_to([1, 2, 3, 4, 5, 6, 7, 8], L),
        # x in [16, 512): two characters; [512, 16384): three (four: the test below)
        "two_char_counts": _pad_to([20, 300, 25, 310, 30], L),
        "negative_one_group": _pad_to([10, 14, 9, 3, 1, 2], L),              # deltas -11 .. -1: one group
        "negative_two_groups": _pad_to([10, 300, 200, 20, 3, 4], L),         # deltas -280, -197: two groups
    }
    if L > 2000:
        out["three_char_counts"] = _pad_to([600, 700, 650, 800], L)
        out["negative_sign_extended"] = _pad_to([3, 900, 880, 100, 60, 17], L)   # -800, -820: sign past two groups
    return out


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_counts_stage_is_rle_from_string(jres, size):
    lists = _count_lists(*size)
    rles = [_as_rle(c, size) for c in lists.values()]
    widths = {len(rle.rle_to_string([c])) for cs in lists.values() for c in cs}
    assert {1, 2}.issubset(widths)
    got = jres.rle_counts(rles)
    for (name, counts), r, (g, status) in zip(lists.items(), rles, got):
        assert g == rle.rle_from_string(r["counts"]) == counts, name
        assert status == 0, name


def test_counts_that_need_up_to_four_characters(jres):
    """Counts of 1, 2, 3 and 4 characters in one string (97x131: 12707 pixels)."""
    size = (97, 131)
    counts = [7, 200, 3000, 9000, 500]
    assert [len(rle.rle_to_string([c])) for c in (7, 200, 3000, 20000)] == [1, 2, 3, 4]
    r = [_as_rle(counts, size), _as_rle([0, 12707], size), _as_rle([12707], size)]
    assert len(r[1]["counts"]) == 1 + 3 and len(r[2]["counts"]) == 3
    big = {"size": [200, 200], "counts": rle.rle_to_string([20000, 16500, 3500])}   # a 4-character count first
    got = jres.rle_counts(r + [big])
    assert [g for g, _ in got] == [counts, [0, 12707], [12707], [20000, 16500, 3500]]
    assert [s for _, s in got] == [0, 0, 0, 0]


def _string_of_length(n_chars, L, chunk):
    """A well-formed count list whose string has exactly ``n_chars`` characters: up to eight
    one-character counts, then counts alternating 17 / 37 per chain (deltas of +-20: two characters
    each) and the closing run; past one chunk, a two-character count sits across the boundary."""
    for lead in range(9):
        for n in range(1, n_chars):
            base = [5] * lead + [17 + 20 * ((i // 2) % 2) + (i % 2) for i in range(n)]
            for tail in ([], base[-2:-1]):  # a count equal to the one two before it: one character more
                counts = base + tail
                if sum(counts) >= L:
                    continue
                counts = counts + [L - sum(counts)]
                s = rle.rle_to_string(counts)
                if len(s) == n_chars and (n_chars <= chunk or (ord(s[chunk - 1]) - 48) & 0x20):
                    return counts, s
    raise AssertionError(f"no string of {n_chars} characters")


def test_strings_around_the_chunk_boundary(jres):
    """Strings of chunk - 1, chunk, chunk + 1 and two chunks + 1 characters, the longer ones with a
    two-character count across the boundary; chains and run ends carry from step to step."""
    from rgbd_amd import _lib
    chunk = _lib.lib().rgbd_rle_chunk()
    size = (97, 131)
    L = size[0] * size[1]
    made = [_string_of_length(n, L, chunk) for n in (chunk - 1, chunk, chunk + 1, 2 * chunk + 1)]
    rles = [{"size": list(size), "counts": s} for _, s in made]
    assert [len(r["counts"]) for r in rles] == [chunk - 1, chunk, chunk + 1, 2 * chunk + 1]
    got = jres.rle_counts(rles)
    for (counts, s), (g, status) in zip(made, got):
        assert g == rle.rle_from_string(s) == counts and status == 0, len(s)


def test_bad_strings_get_their_status(jres):
    size = (24, 40)
    ok = rle.rle_to_string([100, 200, 660])
    neg = rle.rle_to_string([100, -5, 865])
    short = rle.rle_to_string([100, 200, 600])
    trunc = ok[:-1] + chr(((ord(ok[-1]) - 48) | 0x20) + 48)   # the last group announces another that never comes
    got = jres.rle_counts([{"size": list(size), "counts": s} for s in (ok, neg, short, trunc, "")])
    assert [s for _, s in got][0] == 0
    assert got[1][1] & 1 and got[2][1] == 2 and got[3][1] & 4 and got[4][1] == 2 and got[4][0] == []


# ------------------------------------------------------------------ stack mode
def _masks(h, w, seed):
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[:h, :w]
    ms = [np.zeros((h, w), bool), np.ones((h, w), bool), rng.rand(h, w) < 0.5, rng.rand(h, w) < 0.03,
          (x > 3) & (x < w - 2),                      # whole columns: runs that cross column boundaries
          (y % 5 < 3), ((x + y) % 7 < 2) | (y == h - 1)]
    ms[2][0, 0] = True
    ms[3][0, 0] = False
    return np.stack(ms)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_decode_masks_is_rle_decode_and_round_trips(jres, size):
    from rgbd_amd import export
    h, w = size
    m = _masks(h, w, seed=h)
    rles = [rle.encode(k.astype(np.uint8)) for k in m]
    got = jres.decode_masks(rles)
    assert got.dtype == torch.bool and tuple(got.shape) == (len(m), h, w) and got.is_cuda
    want = np.stack([rle.rle_decode(h, w, rle.rle_from_string(r["counts"])) for r in rles]).astype(bool)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(want, m)
    again = export.encode_masks(got)                                   # encode(decode(r)) == r
    assert [r["counts"] for r, _ in again] == [r["counts"] for r in rles]
    back = jres.decode_masks([r for r, _ in export.encode_masks(torch.from_numpy(m).cuda())])
    assert torch.equal(back, torch.from_numpy(m).cuda())              # decode(encode(m)) == m


def test_decode_masks_with_zero_length_runs(jres):
    """Equal neighbouring run ends (zero-length runs in the middle): the search steps over them."""
    h, w = 23, 37
    counts = _pad_to([4, 0, 0, 6, 0, 3, 2, 0, 0, 0, 5, 0, 0, 1, 9], h * w)
    got = jres.decode_masks([_as_rle(counts, (h, w))])[0].cpu().numpy()
    assert np.array_equal(got, rle.rle_decode(h, w, counts).astype(bool))


# ------------------------------------------------------------------ the loader
def _check_loaded(got, g, k):
    assert (got is None) == bool(g[f"l{k}_none"])
    if got is None:
        return
    seg = got["segmentation"]
    assert seg.is_cuda and seg.dtype == torch.int32 and np.array_equal(seg.cpu().numpy(), g[f"l{k}_map"])
    info = got["segments_info"]
    assert [s["id"] for s in info] == g[f"l{k}_ids"].tolist()
    assert [s["label_id"] for s in info] == g[f"l{k}_labels"].tolist()
    assert [s["score"] for s in info] == g[f"l{k}_scores"].tolist()


@pytest.mark.parametrize("k", range(15))
def test_load_json_prediction_is_the_reference(jres, g12, k, tmp_path):
    name = _names(g12)[k]
    text, shape = str(g12[f"l{k}_json"]), g12[f"l{k}_shape"].tolist()
    _check_loaded(jres.load_json_prediction(json.loads(text), shape), g12, k)
    if name in ("covered_empty_repeat", "first_small", "missing_scores"):   # the same through a file
        path = tmp_path / f"{name}.json"
        path.write_text(text)
        _check_loaded(jres.load_json_prediction(str(path), shape), g12, k)


def test_fixture_has_fifteen_load_cases(g12):
    assert len(_names(g12)) == 15


def test_unreadable_file_is_none(jres, tmp_path):
    bad = tmp_path / "bad.json"
    bad.write_text("{not json")
    assert jres.load_json_prediction(str(bad), (24, 40)) is None
    assert jres.load_json_prediction(str(tmp_path / "absent.json"), (24, 40)) is None


def test_256_masks_are_refused_and_255_accepted(jres, g12):
    k = _names(g12).index("many_255")
    data = jr.case_json(g12, f"l{k}_json")
    assert len(data["masks"]) == 255 and jres.load_json_prediction(data, (24, 40)) is not None
    for key in ("masks", "labels", "scores"):
        data[key] = data[key] + data[key][:1]
    with pytest.raises(ValueError, match="256 masks"):
        jres.load_json_prediction(data, (24, 40))


def _random_file(rng, n, size, other_sizes=()):
    h, w = size
    masks = []
    for i in range(n):
        hh, ww = (h, w) if i == 0 or not other_sizes else other_sizes[rng.randint(len(other_sizes))]
        y0, x0 = rng.randint(0, hh - 2), rng.randint(0, ww - 2)
        m = np.zeros((hh, ww), np.uint8)
        m[y0:y0 + rng.randint(1, hh), x0:x0 + rng.randint(1, ww)] = 1
        m &= (rng.rand(hh, ww) < 0.8).astype(np.uint8)
        masks.append(rle.encode(m))
    return {"labels": [int(v) for v in rng.randint(0, 9, n)], "scores": [float(v) for v in rng.rand(n).round(3)],
            "bboxes": [[0.0] * 4] * n, "masks": masks}


@pytest.mark.parametrize("size", SIZES[1:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_loader_is_the_checker_at_ragged_sizes(jres, size):
    """Sizes that are no multiple of the lane's 4 pixels, more than one block (97x131), masks
    of the image's size and resized ones (up, down, ragged) in one file."""
    rng = np.random.RandomState(size[0])
    data = _random_file(rng, 9, size, other_sizes=[size, (size[0] // 2, size[1] // 2), (2 * size[0], 2 * size[1]),
                                                    (17, 29)])
    got = jres.load_json_prediction(data, size)
    seg, ids, labels, scores = jr.load_prediction(data, size)
    assert np.array_equal(got["segmentation"].cpu().numpy(), seg)
    assert [(s["id"], s["label_id"], s["score"]) for s in got["segments_info"]] == list(zip(ids, labels, scores))


def test_batched_load_is_three_single_loads_with_one_host_read(jres, monkeypatch):
    rng = np.random.RandomState(5)
    size = (24, 40)
    files = [_random_file(rng, 0, size), _random_file(rng, 1, size), _random_file(rng, 7, size, [size, (12, 20)])]
    singles = [jres.load_json_prediction(f, size) for f in files]
    reads = {"n": 0}
    for name in ("cpu", "item", "tolist", "numpy", "__bool__", "__int__", "__float__", "__index__"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, **kw):
            if self.is_cuda:
                reads["n"] += 1
            return _orig(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, counted)
    batch = jres.load_json_predictions(files, size)
    monkeypatch.undo()
    assert reads["n"] == 1
    assert singles[0] is None and batch[0] is None
    for s, b in zip(singles[1:], batch[1:]):
        assert torch.equal(s["segmentation"], b["segmentation"]) and s["segments_info"] == b["segments_info"]
    again = jres.load_json_predictions(files, size)   # no atomics: bitwise repeatable
    assert all(torch.equal(a["segmentation"], b["segmentation"]) for a, b in zip(again[1:], batch[1:]))


# ------------------------------------------------------------------ the comparison
@pytest.mark.parametrize("k", range(3))
@pytest.mark.parametrize("a", [0, 1])
def test_multi_model_comparison_is_the_reference(jres, g12, k, a):
    image = torch.from_numpy(g12["image"]).cuda()
    gt = jr.case_json(g12, f"m{k}_gt")
    models = [json.loads(str(t)) for t in g12[f"m{k}_models"]]
    out = jres.multi_model_comparison(image, gt, models, alpha=float(g12["alphas"][a]))
    assert out["gt_overlay"].is_cuda and tuple(out["model_overlays"].shape) == (len(models), 24, 40, 3)
    assert np.array_equal(out["gt_overlay"].cpu().numpy(), g12[f"m{k}_gt_overlays"][a])
    assert np.array_equal(out["model_overlays"].cpu().numpy(), g12[f"m{k}_model_overlays"][a])
    assert (out["gt"] is None) == bool(g12[f"m{k}_gt_none"])
    assert [m is None for m in out["models"]] == g12[f"m{k}_model_none"].tolist()


def test_comparison_cases_cover_q19_a_failed_model_and_no_gt(jres, g12):
    assert _names(g12, "cmp_names") == ["three_models", "resized_model", "gt_none"]
    models = [json.loads(str(t)) for t in g12["m0_models"]]
    covered = jres.load_json_prediction(models[1], (24, 40))
    ids = [s["id"] for s in covered["segments_info"]]
    assert 1 in ids and not bool((covered["segmentation"] == 1).any())   # listed, empty in the map: Q19
    assert g12["m0_model_none"].tolist() == [False, False, True] and bool(g12["m2_gt_none"])
    image = torch.from_numpy(g12["image"]).cuda()
    out = jres.multi_model_comparison(image, jr.case_json(g12, "m2_gt"), [json.loads(str(t)) for t in g12["m2_models"]])
    assert out["models"][0] is not None and torch.equal(out["model_overlays"][0], image)  # no GT: the bare image


# ------------------------------------------------------------------ refusals
def test_refusals(jres, g12):
    a = rle.encode(np.ones((24, 40), np.uint8))
    short = {"size": [24, 40], "counts": rle.rle_to_string([100, 200, 600])}
    with pytest.raises(ValueError, match="mask 1"):
        jres.decode_masks([a, short])
    file = {"labels": [1, 2, 3], "scores": [1.0, 1.0, 1.0], "masks": [a, a, short]}
    with pytest.raises(ValueError, match="mask 2"):
        jres.load_json_prediction(file, (24, 40))
    file["labels"] = [1, 2]                       # the bad mask takes no part: the reference never decodes it
    assert [s["id"] for s in jres.load_json_prediction(file, (24, 40))["segments_info"]] == [1, 2]
    for counts in ([100, 200, 660], b"PPY", None):
        with pytest.raises(ValueError, match="mask 1"):
            jres.load_json_prediction({"labels": [1, 2], "scores": [1.0, 1.0],
                                       "masks": [a, {"size": [24, 40], "counts": counts}]}, (24, 40))
        with pytest.raises(ValueError, match="mask 0"):
            jres.decode_masks([{"size": [24, 40], "counts": counts}])
    with pytest.raises(ValueError, match="mask 1"):
        jres.decode_masks([a, rle.encode(np.ones((12, 20), np.uint8))])   # one size only
    with pytest.raises(RuntimeError):
        jres.decode_masks([a], device="cpu")
    with pytest.raises(RuntimeError):
        jres.load_json_prediction(file, (24, 40), device="cpu")
    with pytest.raises(RuntimeError):
        jres.multi_model_comparison(torch.from_numpy(g12["image"]), file, [file])
