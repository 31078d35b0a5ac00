"""bench.py's plain run on the GPU: the headline figure alone, and --dump-outputs."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]


B, H, W, STEPS, WARMUP = 2, 96, 128, 3, 1


@pytest.fixture(scope="module")
def plain_runs(tmp_path_factory):
    """Two plain runs with the same arguments, each a process of its own: (result line, wall
    seconds, folder of dumped arrays) per run."""
    import time
    runs = []
    for i in range(2):
        d = tmp_path_factory.mktemp(f"dump{i}")
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup",
                            str(WARMUP), "--batch", str(B), "--height", str(H), "--width", str(W),
                            "--dump-outputs", str(d)], capture_output=True, text=True, timeout=120, cwd=REPO)
        wall = time.perf_counter() - t0
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]  # stdout: the one JSON line only
        runs.append((json.loads(lines[0]), wall, d))
    return runs


def test_bench_plain_run_line(plain_runs):
    """``bench.py --gpus 1 --steps N --warmup W`` prints one line with the headline figure
    (ms_per_step x value = the batch) and none of the --full legs."""
    out = plain_runs[0][0]
    assert out["steps"] == STEPS and out["warmup"] == WARMUP and out["n_gpus"] == 1 and out["graph"] is True
    assert out["unit"] == "img/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    assert out["ms_per_step"] > 0 and abs(out["value"] * out["ms_per_step"] / 1e3 / B - 1) < 1e-2
    for key in ("roofline", "kernels", "kernel_ms", "eager_img_s", "inference_img_s", "parity", "c5_stream",
                "full_model", "cpu_baseline"):
        assert key not in out


def test_bench_plain_run_spends_under_30_s_outside_its_steps(plain_runs):
    """The whole process, start to exit, less its (N + W) steps: at most 30 s, so that a leg of
    --full that found its way back into the plain run shows (the first run includes whatever a
    first run compiles or tunes)."""
    for out, wall, _ in plain_runs:
        outside = wall - (STEPS + WARMUP) * out["ms_per_step"] / 1e3
        print(f"wall {wall:.2f} s, outside the steps {outside:.2f} s")
        assert outside < 30.0


def test_bench_dump_outputs_same_from_run_to_run(plain_runs):
    """--dump-outputs: the last timed step's four output features, whole at this shape, finite
    float32, from identical inputs in both runs.

    feature0 (the DGGM fusion of the first colour map: no DSAM feeds it, so neither the window
    ratio nor the region codes do) is the same in two runs up to bf16 rounding: 2 bf16 ulps of the
    element (2 x 2^-7 relative) plus the same fraction of the array's rms for elements that cancel
    to near zero.

    feature1..3 come through the DSAM cascade, whose region codes are discrete decisions on the
    ratio predictor's output, and that output is not reproducible in train mode: two processes
    on the same input and the same BatchNorm state gave ratios 0.2548 and 0.2578, and the codes of
    a few cells flipped with them.  A flipped cell takes another filter, so no element-wise bound
    holds there (measured at this shape: feature0 0 of 147 456 elements differ; feature1 5 424 of
    73 728, max 1.14 at rms 2.18; at 640x480 B=8 the codes agreed and features 1..3 differed by
    one bf16 ulp, 0.0625 at magnitude 8-16).  Their differences are printed, not asserted."""
    sizes, h, w = [], -(-H // 4), -(-W // 4)
    for c in (96, 192, 384, 768):
        sizes.append(B * c * h * w)
        h, w = -(-h // 2), -(-w // 2)
    names = [f"feature{k}.npy" for k in range(4)]
    for _, _, d in plain_runs:
        assert sorted(f.name for f in d.iterdir()) == names
    for k, (name, n) in enumerate(zip(names, sizes)):
        a, b = np.load(plain_runs[0][2] / name), np.load(plain_runs[1][2] / name)
        for x in (a, b):
            assert x.dtype == np.float32 and x.shape == (n,) and np.isfinite(x).all() and x.std() > 0
        rms = float(np.sqrt(np.mean(a.astype(np.float64) ** 2)))
        diff = np.abs(a - b)
        print(f"{name}: max|run1 - run2| = {diff.max():.4g}, rms {rms:.4g}, differing {int((diff > 0).sum())} of {n}")
        if k == 0:
            assert (diff <= 2.0 ** -6 * (np.maximum(np.abs(a), np.abs(b)) + rms)).all()


def test_bench_plain_run_two_ranks_gloo():
    """The plain run at N = 2 (both ranks on the one GPU over gloo): the data-parallel step's
    figure alone, none of the --full legs (no scaling baseline, no per-kernel timings)."""
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "2", "--backend", "gloo", "--steps", "2",
                        "--warmup", "1", "--height", "96", "--width", "128"],
                       capture_output=True, text=True, timeout=200, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 16 and out["distributed"]["backend"] == "gloo"
    assert out["value"] > 0 and abs(out["value"] * out["ms_per_step"] / 1e3 / 16 - 1) < 1e-2
    assert out["ddp_form"] == "eager, all-reduces overlapped"
    for key in ("roofline", "kernels", "kernel_ms", "eager_img_s", "scaling_baseline_img_s", "full_model"):
        assert key not in out
