"""The ratio predictor's dropout stream as tests/checkers/ratio_dropout.py restates it
(include/rgbd_hip.h documents the rule; tests/test_gpu_ratio_train.py checks the kernels against
this restatement): pinned hash values, drop fractions, independence between consecutive counters
and between the two layers.  Seed 0x5EED, counters 0..3, B = 32 (n = 4096 / 2048 draws per mask);
statistical bounds are 4 sigma of the binomial, sigma = sqrt(q (1 - q) / n)."""
import math

import numpy as np
import pytest

from checkers import ratio_dropout as rd

SEED, B = 0x5EED, 32
COUNTERS = range(4)

# (seed, index, top 24 bits of the splitmix64 finaliser of seed + index * 0x9E3779B97F4A7C15)
PINNED = [
    (0, 0, 0),
    (0x5EED, 0, 10588007),
    (0x5EED, 1, 651773),
    (0x5EED, 4095, 2735208),
    (0x5EED ^ 0x5555, 0, 9467820),
    (0x5EED + 3, 2047, 2912920),
    ((1 << 64) - 1, 5, 11837511),           # seed + index * gamma wraps
    (0x5EED + 2 ** 40 + 5, 77, 14859530),
]


def test_pinned_hash_values():
    for seed, idx, k in PINNED:
        assert rd.bits24(seed, idx) == k, (hex(seed), idx)
        assert int(rd.bits24_array(seed, idx + 1)[idx]) == k, (hex(seed), idx)
        assert rd.u(seed, idx) == np.float32(k / 2.0 ** 24)
        assert 0.0 <= float(rd.u(seed, idx)) < 1.0


def test_float32_thresholds_are_the_integer_form():
    """u < 0.3f  <=>  k <= DROP1_MAX and u < 0.2f  <=>  k <= DROP2_MAX, at the boundary and in the
    masks themselves."""
    s = np.float32(2.0 ** -24)
    for p, kmax in ((rd.P1, rd.DROP1_MAX), (rd.P2, rd.DROP2_MAX)):
        assert np.float32(kmax) * s < np.float32(p)
        assert not (np.float32(kmax + 1) * s < np.float32(p))
    for c in COUNTERS:
        keep1, keep2 = rd.keep_masks(SEED, c, B)
        assert keep1.shape == (B, 128) and keep2.shape == (B, 64) and keep1.dtype == keep2.dtype == bool
        np.testing.assert_array_equal(keep1.reshape(-1), rd.bits24_array(SEED + c, B * 128) > rd.DROP1_MAX)
        np.testing.assert_array_equal(keep2.reshape(-1), rd.bits24_array((SEED + c) ^ 0x5555, B * 64) > rd.DROP2_MAX)


def test_masks_index_by_image_then_unit():
    keep1, keep2 = rd.keep_masks(SEED, 2, B)
    for b, o in ((0, 0), (0, 127), (1, 0), (17, 5), (31, 127)):
        assert keep1[b, o] == (rd.bits24(SEED + 2, b * 128 + o) > rd.DROP1_MAX)
    for b, o in ((0, 0), (0, 63), (1, 0), (17, 5), (31, 63)):
        assert keep2[b, o] == (rd.bits24((SEED + 2) ^ 0x5555, b * 64 + o) > rd.DROP2_MAX)
    # a smaller batch is a prefix of a larger one's stream
    k1, k2 = rd.keep_masks(SEED, 2, 3)
    np.testing.assert_array_equal(k1, keep1[:3])
    np.testing.assert_array_equal(k2, keep2[:3])


def test_counter_adds_to_the_seed_mod_2_64():
    a = rd.keep_masks(SEED, 2 ** 40 + 5, 4)
    b = rd.keep_masks(SEED + 2 ** 40 + 5, 0, 4)
    c = rd.keep_masks(SEED, 2 ** 64 + 2 ** 40 + 5, 4)
    for x, y, z in zip(a, b, c):
        np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(x, z)
    assert not np.array_equal(a[0], rd.keep_masks(SEED, 5, 4)[0])  # the high half of the counter counts


@pytest.mark.parametrize("layer,p,n", [(0, rd.P1, B * 128), (1, rd.P2, B * 64)])
def test_drop_fraction_within_4_sigma(layer, p, n):
    sigma = math.sqrt(p * (1 - p) / n)
    for c in COUNTERS:
        frac = 1.0 - rd.keep_masks(SEED, c, B)[layer].mean()
        print(f"layer {layer} counter {c}: drop fraction {frac:.4f} ({(frac - p) / sigma:+.2f} sigma)")
        assert abs(frac - p) <= 4 * sigma, (c, frac)


@pytest.mark.parametrize("layer,p,n", [(0, rd.P1, B * 128), (1, rd.P2, B * 64)])
def test_consecutive_counters_are_independent(layer, p, n):
    q = p * p + (1 - p) * (1 - p)  # two independent masks agree on a unit with this probability
    sigma = math.sqrt(q * (1 - q) / n)
    masks = [rd.keep_masks(SEED, c, B)[layer] for c in COUNTERS]
    for c in range(len(masks) - 1):
        agree = float((masks[c] == masks[c + 1]).mean())
        print(f"layer {layer} counters {c},{c + 1}: agreement {agree:.4f} (independent: {q:.4f})")
        assert abs(agree - q) <= 4 * sigma, (c, agree)


def test_layers_draw_different_sequences():
    """fc_layers.5's uniforms (seed ^ 0x5555) are not fc_layers.2's: neither equal nor a shift of
    one another over the first 2048 draws, and uncorrelated within 4 sigma."""
    n = B * 64
    for c in COUNTERS:
        s = SEED + c
        k1, k2 = rd.bits24_array(s, B * 128), rd.bits24_array(s ^ 0x5555, n)
        assert not np.array_equal(k1[:n], k2)
        assert np.intersect1d(k1, k2).size <= 4  # 4096 x 2048 pairs of 24-bit values: 0.5 expected by chance
        r = float(np.corrcoef(k1[:n].astype(np.float64), k2.astype(np.float64))[0, 1])
        assert abs(r) <= 4 / math.sqrt(n), r
