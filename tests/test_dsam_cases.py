"""The case table of checkers/dsam_cases.py reaches every K5 kernel variant (CPU).

dsam_cases restates the kernels' plan arithmetic (ld_kc, ld_linear, the N-tile count of ld_plan;
wg_fm and the tile counts of wg_plan; the dX parity-class sizes of ld_geom); this file first pins
that restatement to the sources' text, then asserts what the table must cover, so that a later
edit of the table cannot silently lose a variant."""
import re
from pathlib import Path

import pytest

from checkers import dsam_cases as cases

CSRC = Path(__file__).resolve().parents[1] / "rgb-d-instance-segmentation_amd" / "csrc"
BF = cases.BF16_CASES


def _variants(kind):
    return {n: cases.conv_variant(kind, *s) for n, s in BF.items()}


def _has(text, *fragments):
    """Every fragment occurs in ``text``, compared without whitespace (formatting may change)."""
    squeezed = re.sub(r"\s+", "", text)
    return all(re.sub(r"\s+", "", f) in squeezed for f in fragments)


def test_restatement_matches_the_sources():
    """Meant to fail when the plan arithmetic in the sources changes: then update the restatement
    in checkers/dsam_cases.py (and the table, if a variant moved) together with these fragments."""
    lds = (CSRC / "dsam_lds.hip").read_text()
    wg = (CSRC / "dsam_wgrad.hip").read_text()
    assert _has(lds, "int ld_kc(int C) { return C % 96 == 0 ? 3 : (C % 64 == 0 ? 2 : 1); }",
                "LD_BM = 128, LD_BN = 192, LD_CH = 8;",
                "blk = (long long)((Hc + 7) / 8 * 8) * ((Wc + 15) / 16 * 16);",
                "return (long long)Hc * Wc * 100 < 85 * blk;", "p.ntn = ceil_div(a.N, LD_BN);")
    assert _has(wg, "int wg_fm(int Cout) { return Cout % 192 == 0 ? 6 : (Cout % 128 == 0 ? 4 : 2); }",
                "p.ntile_kk = ceil_div(9ll * Cin, 128);", "WPX = 64;")


def test_every_kc_forward_and_dx():
    for kind in ("fwd", "dx"):
        assert {v["kc"] for v in _variants(kind).values()} == {1, 2, 3}, kind
    # more than one chunk group per step loop, for each KC that the channel counts allow
    assert any(v["kc"] == 1 and v["ncg"] >= 5 for v in _variants("dx").values())
    assert any(v["kc"] == 2 and v["ncg"] >= 2 for v in _variants("fwd").values())
    assert any(v["kc"] == 3 and v["ncg"] >= 2 for v in _variants("fwd").values())


def test_every_fm_and_ragged_gemm_tiles():
    w = {n: cases.wgrad_variant(*s) for n, s in BF.items()}
    assert {v["fm"] for v in w.values()} == {2, 4, 6}
    assert any(v["kk_tail"] for v in w.values()) and any(not v["kk_tail"] for v in w.values())
    assert any(v["o_tail"] and v["ntile_o"] >= 3 for v in w.values())
    assert any(v["unit_tail"] and v["nunit"] >= 4 for v in w.values())
    assert any(v["nunit"] == 1 and v["unit_tail"] == 1 for v in w.values())


def test_tile_shapes():
    f = _variants("fwd")
    assert any(v["linear"] and v["crosses"] for v in f.values()), "linear tiles spanning two images"
    assert any(v["exact"] for v in f.values()), "8x16 blocks, exact"
    assert any(not v["linear"] and not v["exact"] for v in f.values()), "8x16 blocks, ragged"
    assert any(v["ntn"] == 2 and v["n_last"] < cases.LD_BN for v in f.values()), "two N tiles, the second partly empty"
    assert {v["n_last"] for v in f.values() if v["ntn"] == 1} >= {32, 160, 192}
    assert {cases.CASES[n][2] for n in BF} >= {32, 160, 224, 256}  # N = 32, 160, 224, 256 forward
    assert 96 in {cases.CASES[n][1] for n in BF}                   # N = 96 in a dX


def test_dx_parity_classes():
    sizes = {n: cases.class_sizes(s[3], s[4]) for n, s in BF.items()}
    assert sizes["A"] == [(8, 16), (8, 15), (7, 16), (7, 15)]
    assert any(len(set(c)) == 4 for c in sizes.values()), "four classes of unequal size"
    empty = [n for n, c in sizes.items() if any(hc * wc == 0 for hc, wc in c)]
    assert "F1" in empty and "F2" in empty
    assert sizes["F1"] == [(1, 1), (1, 0), (0, 1), (0, 0)]


@pytest.mark.parametrize("group", [cases.BF16_CASES, cases.CASES], ids=["bf16", "float32"])
def test_n_masks_cover_0_to_4(group):
    assert {n for name in group for n in cases.n_masks_of(name)} == {0, 1, 2, 3, 4}


def test_the_table_case_by_case():
    """The classification the table was chosen for, case by case."""
    f, d = _variants("fwd"), _variants("dx")
    w = {n: cases.wgrad_variant(*s) for n, s in BF.items()}
    assert (f["A"]["kc"], f["A"]["exact"], d["A"]["kc"], w["A"]["fm"], w["A"]["kk_tail"]) == (1, True, 1, 2, 32)
    assert (f["B"]["kc"], f["B"]["linear"], d["B"]["kc"], d["B"]["ncg"], w["B"]["nunit"], w["B"]["unit_tail"]) == \
        (2, True, 1, 5, 4, 63)
    assert (f["C"]["kc"], f["C"]["ntn"], f["C"]["n_last"], f["C"]["linear"], f["C"]["exact"], d["C"]["ncg"]) == \
        (3, 2, 32, False, False, 7)
    assert (f["D"]["kc"], f["D"]["ncg"], f["D"]["linear"], d["D"]["kc"], d["D"]["ncg"], w["D"]["fm"],
            w["D"]["kk_tail"], w["D"]["nunit"]) == (2, 2, True, 2, 4, 4, 0, 1)
    assert (f["E"]["kc"], f["E"]["exact"], d["E"]["kc"], w["E"]["fm"]) == (3, True, 3, 6)
    # the float32 legs: Cin % 8 only, and N = 72 against the float32 kernel's 64-column tile
    assert [s[1] % 32 for s in cases.F32_ONLY_CASES.values()] == [8, 8]
    assert cases.F32_ONLY_CASES["G2"][2] == 72
