"""The float64 restatement of K5 (tests/checkers/dsam_ref.py) and its comparator, checked on the
CPU before tests/test_gpu_dsam_parity.py relies on them.

1. Exact weights: with filter values that are multiples of 2^-6 in [-7, 7] * 2^-6 every merged
   sum is exact in bf16, so the merged-by-code references for y, dx and dW/db equal float64
   autograd through the literal five-convolution module formula, to 1e-12 of the magnitude.
2. The yardsticks: torch's CPU float32 path against the checker (dsam_cases.cpu_float32_ratios,
   pinned to one thread so that the figures do not follow the machine's core count); K5_F, K5_X
   and K5_B cover 8 times the ratios measured here and are no more than a tenth above that.
3. The emulated bf16 kernel (checkers/dsam_emul.py: float32, tap by tap and code by code) passes
   the comparator on every case and code map with 1/8 of the constants.  On the bf16 outputs the
   2^-8 |ref| term is exactly the one rounding of the result (bf16 keeps 8 significant bits, so
   round-to-nearest moves a value by up to 2^-8 of it) and the emulation uses nearly all of it;
   the 1/8 applies to the K * EPS * A term beside it.  Where ``k_of`` caps a constant at the
   number of summands (dW of case F) the bound is rigorous for any summation order and the
   emulation is held to it whole.
4. The mutants of dsam_emul are rejected on every case and code map where they change the
   emulation's result at all; the failing share is printed.  Each mutant is judged on the output
   the GPU test compares: the forward's float32 output, dX's bf16 output, dW/db.  each_add is
   judged on the forward only: dX has no float32 output, and against 2^-8 |ref| of its bf16 one a
   filter error of 2^-9 per element mostly hides; the forward reads the same packed filters.  Smallest
   failing shares seen: bias_prefix 0.33 (one of three images), each_add 0.99, code_dst 0.37,
   code_src 0.20, right_edge 0.059 (one output column), prev_image 0.004 (the rows of one tile
   past the boundary), drop_unit 0.056, drop_kk 0.037 (the columns dropped), db_all 0.25 (one of
   four biases)."""
import pytest
import torch
import torch.nn.functional as F

from checkers import dsam_cases as cases
from checkers import dsam_emul as emul
from checkers import dsam_ref as R

BF = list(cases.BF16_CASES)
PAIRS = [(n, k) for n in BF for k in cases.MAPS]


def _literal_autograd(i, code, cw, pw, b4):
    """float64 autograd through the module formula -> y, dx (+ gin), dconv, dproj, dbias."""
    x = i["x"].double().requires_grad_(True)
    cw, pw, b4 = (t.double().requires_grad_(True) for t in (cw, pw, b4))
    y = F.conv2d(x, pw, stride=2, padding=1)
    for n in range(4):
        y = y + F.conv2d(x * ((code >> n) & 1)[:, None].double(), cw[n], stride=2, padding=1)
    y = y + torch.stack([b4[:n].sum(0) if n > 0 else b4[:1].sum(0) * 0 for n in i["n_masks"]])[:, :, None, None]
    y = y + i["residual"].double()
    y.backward(i["gy"].double())
    return dict(y=y.detach(), dx=x.grad + i["gin"].double(), dconv=cw.grad, dproj=pw.grad, dbias=b4.grad)


@pytest.mark.parametrize("name", ["A", "B", "D", "F2"])
@pytest.mark.parametrize("kind", ["rand", "scene"])
def test_exact_weights_merged_equals_literal(name, kind):
    i = cases.inputs(name, True)
    code = cases.code_map(name, kind)
    g = torch.Generator().manual_seed(3)
    cw = torch.randint(-7, 8, i["conv_w"].shape, generator=g).float() / 64
    pw = torch.randint(-7, 8, i["proj_w"].shape, generator=g).float() / 64
    wq = R.merged_filters(cw, pw)
    for k in range(16):  # nothing lost in the one rounding
        want = pw.double() + sum(cw[n].double() for n in range(4) if (k >> n) & 1)
        assert torch.equal(wq[k], want)
    lit = _literal_autograd(i, code, cw, pw, i["bias4"])
    got = dict(y=R.fwd_merged(i["x"], code, i["n_masks"], wq, i["bias4"], i["residual"]),
               dx=R.dx_merged(i["gy"], code, wq, i["gin"]), **R.dw_ref(i["x"], i["gy"], code, i["n_masks"]))
    lit2 = dict(y=R.fwd_literal(i["x"], code, i["n_masks"], cw, pw, i["bias4"], i["residual"]),
                dx=R.dx_literal(i["gy"], code, cw, pw, i["gin"]))
    for leg, (v, a) in got.items():
        assert float(((v - lit[leg]).abs() - 1e-12 * a).max()) <= 0, leg
        assert bool((a >= v.abs() * (1 - 1e-12)).all()), f"{leg}: magnitude below the value"
    for leg, (v, a) in lit2.items():
        assert float(((v - lit[leg]).abs() - 1e-12 * a).max()) <= 0, leg
        assert bool((a >= got[leg][1] * (1 - 1e-12)).all()), leg  # |sum of filters| <= sum of |filters|


def test_yardsticks_cover_the_cpu_float32_path():
    worst = {}
    for bf in (True, False):
        for name in (cases.BF16_CASES if bf else cases.CASES):
            for kind in cases.MAPS:
                for leg, r in cases.cpu_float32_ratios(name, kind, bf).items():
                    if r > worst.get((leg, bf), (0.0,))[0]:
                        worst[(leg, bf)] = (r, name, kind)
    for key, v in sorted(worst.items()):
        print(f"cpu float32 vs float64 {key[0]:6s} {'bf16 operands' if key[1] else 'float32     '}: "
              f"{v[0]:.3f} at {v[1]} {v[2]}")
    top = lambda *legs: max(worst[(leg, bf)][0] for leg in legs for bf in (True, False))
    # each constant covers 8 x the measured ratio and is not inflated past it (rounding up, and a
    # tenth for a torch build whose single-thread kernels block their sums differently)
    for k, t in ((cases.K5_F, top("y")), (cases.K5_X, top("dx")), (cases.K5_B, top("dconv", "dproj", "dbias"))):
        assert 8 * t <= k <= 1.1 * 8 * t + 1, (k, t)


@pytest.mark.parametrize("name,kind", PAIRS)
def test_emulation_within_an_eighth_of_the_bounds(name, kind):
    i, code, ref = cases.reference(name, kind, True)
    y32, dx32, d = emul.fwd(name, i, code), emul.dx(name, i, code), emul.dw(name, i, code)
    def k8(leg):  # an eighth of the constant, the whole of a rigorous one
        k = cases.k_of(name, leg)
        return k if k == cases.summands(name)[leg] else k / 8
    r = dict(y_f32=R.compare(y32, *ref["y"], k8("y")),
             y_bf16=R.compare(R.bf16(y32), *ref["y"], k8("y"), R.BF16_REL),
             dx_bf16=R.compare(R.bf16(dx32), *ref["dx"], k8("dx"), R.BF16_REL),
             **{leg: R.compare(d[leg], *ref[leg], k8(leg)) for leg in d})
    print(f"emulation {name} {kind} (error / bound at K / 8): " + "  ".join(f"{k} {v[0]:.3f}" for k, v in r.items()))
    for k, (ratio, share) in r.items():
        assert ratio < 1 and share == 0, (k, ratio, share)


MUTANTS = {  # mutant -> (leg it is judged on, emulation)
    "bias_prefix": "y", "each_add": "y", "code_dst": "y", "right_edge": "y", "prev_image": "y",
    "code_src": "dx", "drop_unit": "dw", "drop_kk": "dw", "db_all": "dw",
}


def _run(name, i, code, leg, mutant):
    if leg == "y":
        return dict(y=emul.fwd(name, i, code, mutant))
    if leg == "dx":
        return dict(dx=R.bf16(emul.dx(name, i, code, mutant)))
    return emul.dw(name, i, code, mutant)


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutant_rejected_wherever_it_changes_the_result(mutant):
    leg = MUTANTS[mutant]
    changed = 0
    for name, kind in PAIRS:
        i, code, ref = cases.reference(name, kind, True)
        good, bad = _run(name, i, code, leg, None), _run(name, i, code, leg, mutant)
        diff = [k for k in good if not torch.equal(good[k], bad[k])]
        if not diff:
            continue
        changed += 1
        for k in diff:
            ratio, share = R.compare(bad[k], *ref[k], cases.k_of(name, k), R.BF16_REL if leg == "dx" else 0.0)
            print(f"mutant {mutant} {name} {kind} {k}: error / bound {ratio:.3g}, failing share {share:.3f}")
            assert ratio > 1 and share > 0, (mutant, name, kind, k, ratio)
    assert changed >= 3, f"{mutant} changed {changed} cases only: the table no longer exercises it"
