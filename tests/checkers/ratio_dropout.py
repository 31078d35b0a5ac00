"""Replay of the ratio predictor's train-mode dropout stream (include/rgbd_hip.h, the comment
above `rgbd_ratio_forward`; `hash_uniform`, `k_rp_tail_fc1` and `k_rp_tail_head` in csrc/ratio_tail.hip),
restated in Python integers and NumPy uint64:

    s = seed + counter                                             (mod 2^64)
    u(seed, i) = (splitmix64_finaliser(seed + i * 0x9E3779B97F4A7C15) >> 40) * 2^-24
    fc_layers.2: unit o of image b is dropped when u(s, b * 128 + o) < 0.3f, kept units / 0.7f
    fc_layers.5: unit o of image b is dropped when u(s ^ 0x5555, b * 64 + o) < 0.2f, kept / 0.8f

The kernels compare in float32: k * 2^-24 is exact in float32 for a 24-bit k, float32(0.3) =
5033165 * 2^-24 and float32(0.2) = 3355443.25 * 2^-24, so the comparisons are k <= 5033164 and
k <= 3355443; `keep_masks` compares the float32 values themselves and `DROP1_MAX` / `DROP2_MAX`
state the integer form (tests/test_ratio_dropout_stream.py asserts that the two agree)."""
import numpy as np

MASK64 = (1 << 64) - 1
GOLDEN_GAMMA = 0x9E3779B97F4A7C15
P1, P2 = 0.3, 0.2
N1, N2 = 128, 64
DROP1_MAX = 5033164   # largest 24-bit k with float32(k * 2^-24) < float32(0.3)
DROP2_MAX = 3355443   # ... < float32(0.2)


def bits24(seed, idx):
    """The top 24 bits of the splitmix64 finaliser of seed + idx * GOLDEN_GAMMA, Python ints."""
    z = (int(seed) + int(idx) * GOLDEN_GAMMA) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    z ^= z >> 31
    return z >> 40


def u(seed, idx):
    """u(seed, idx) as the float32 the kernel compares."""
    return np.float32(bits24(seed, idx)) * np.float32(2.0 ** -24)


def bits24_array(seed, n):
    """bits24(seed, i) for i in range(n), vectorised in uint64 (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & MASK64) + np.arange(n, dtype=np.uint64) * np.uint64(GOLDEN_GAMMA)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.int64)


def uniforms(seed, n):
    """float32 [n]: u(seed, i) for i in range(n)."""
    return bits24_array(seed, n).astype(np.float32) * np.float32(2.0 ** -24)


def keep_masks(seed, counter, B):
    """(keep1 bool [B, 128], keep2 bool [B, 64]): the units fc_layers.2 / fc_layers.5 keep in the
    train forward that finds `counter` in the device counter."""
    s = (int(seed) + int(counter)) & MASK64
    keep1 = ~(uniforms(s, B * N1) < np.float32(P1))
    keep2 = ~(uniforms(s ^ 0x5555, B * N2) < np.float32(P2))
    return keep1.reshape(B, N1), keep2.reshape(B, N2)
