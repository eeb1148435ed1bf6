"""The references of tests/test_gpu_schwarz_shapes.py, checked on the CPU (tests/schwarz_reference.py says what they are):

  * the vectorised restatement `Sweep` in complex128 equals `mg_oracle.Schwarz` to rounding at every shape, block solver, schedule
    and start, with either precision's MinRes threshold, and no <Dr,Dr> comes closer than 1 % to a threshold, so that correct fp32
    code decides every step as the fp64 reference does: near EPS_float = 1e-6 the 96 or more components of D r are of size 1e-4 and
    carry the rounding of a residual that started at size 0.3, 3e-8 each, which moves <Dr,Dr> by less than 0.1 %;
  * the spread, the distance of the complex64 restatements in three summation orders from the fp64 reference, printed per case;
    its maximum is LARGEST_SPREAD, from which the GPU test takes its fp32 bar, and ten times it lies below TOL_SWEEP;
  * the bar discriminates: four wrong smoothers lie at least 100 bars from the reference at every shape."""
import numpy as np
import pytest
import schwarz_reference as sr

_SPREAD = {}


def cases(name):
    return [(oe, m, st) for oe in sr.forms(name) for m in sr.METHODS for st in sr.STARTS]


def spreads(name):
    if name not in _SPREAD:
        _SPREAD[name] = {c: sr.spread(name, c[1], c[0], c[2]) for c in cases(name)}
    return _SPREAD[name]


def form_name(oe):
    return "odd-even" if oe else "plain"


@pytest.mark.parametrize("name", list(sr.SHAPES))
def test_sweep_restates_the_oracle(name):
    eta, phi0 = (sr.cvec(v) for v in sr.vectors(sr.SHAPES[name][1]))
    worst, margin = 0.0, np.inf
    for oe, method, start in cases(name):
        cycles, guess = sr.STARTS[start]
        for prec in (32, 64) if cycles == 3 else (32,):       # the thresholds only matter once the residual is small
            sw = sr.Sweep(name, sr.schwarz(name, method, oe, prec))
            d = sr.relerr(sw.smooth(eta, cycles, phi0 if guess else None), sr.reference(name, method, oe, start, prec))
            worst, margin = max(worst, d), min(margin, sw.margin)
            assert d < 1e-12, (oe, method, start, prec, d)
            assert sw.margin > 0.01, (oe, method, start, prec, sw.margin)
    print(f"{name}: Sweep in complex128 vs mg_oracle.Schwarz {worst:.2e}; closest <Dr,Dr> to a threshold: off by a factor {1 + margin:.3g}")


@pytest.mark.parametrize("name", list(sr.SHAPES))
def test_spread(name):
    sp = spreads(name)
    for (oe, method, start), s in sp.items():
        print(f"spread {name:6s} {form_name(oe):8s} method {method} {start:14s} {s:.3e}")
    print(f"spread {name}: largest {max(sp.values()):.3e}; fp32 bar {sr.fp32_bar():.3e}")
    assert max(sp.values()) <= sr.LARGEST_SPREAD * (1 + 1e-3)
    # rounding the operator and the input alone moves the reference by 4.5e-8: a spread below that would not be one of an fp32 sweep
    assert min(sp.values()) > 4.5e-8


def test_the_recorded_spread_is_the_largest_and_the_bar_lies_below_tol_sweep():
    largest = max(max(spreads(name).values()) for name in sr.SHAPES)
    print(f"largest spread {largest:.4e}, recorded {sr.LARGEST_SPREAD:.4e}, bar {sr.fp32_bar():.3e}, TOL_SWEEP {sr.TOL_SWEEP:.1e}")
    assert abs(largest / sr.LARGEST_SPREAD - 1) < 1e-3
    assert sr.fp32_bar() <= sr.TOL_SWEEP


# cycles from zero at which each wrong smoother is run: the fewest at which it can differ (one MinRes step fewer and the list-4/5
# rule show in the first cycle, a stale or misdirected residual update in the second), where the iterate is still far from converged
MUTANTS = {"iter3": 1, "no45": 1, "stale": 2, "swap": 2}


@pytest.mark.parametrize("name", list(sr.SHAPES))
def test_the_bar_tells_wrong_smoothers_apart(name):
    """every block solver and schedule the mutant exists for.  "swap" needs a direction with more than two blocks, which the 512-site
    shape does not have (two blocks per direction, to stay at 8192 sites); "no45" is a rule of the red-black schedule and needs a
    block of list 4 or 5 (second colour, no face on the upper lattice boundary), which two blocks per direction do not have either"""
    eta = sr.cvec(sr.vectors(sr.SHAPES[name][1])[0])
    need = 100 * sr.fp32_bar()
    swap = sr.ell(name).cols_swapped is not None
    assert swap == (name != "512")
    short = []
    for oe in sr.forms(name):
        for method in sr.METHODS:
            S = sr.schwarz(name, method, oe, 32)
            ref = {c: S.smooth(eta, c) for c in set(MUTANTS.values())}
            for mutant, cycles in MUTANTS.items():
                lists45 = method == 2 and any(b["colour"] == 1 and b["list"] in (4, 5) for b in S.blocks)
                assert method != 2 or lists45 == (name != "512")
                if (mutant == "swap" and not swap) or (mutant == "no45" and not (method == 2 and lists45)):
                    continue
                d = sr.relerr(sr.Sweep(name, S, mutant=mutant).smooth(eta, cycles), ref[cycles])
                print(f"mutant {name:6s} {form_name(oe):8s} method {method} {mutant:6s} {cycles} from zero {d:.3e} = {d / sr.fp32_bar():.0f} bars")
                if not d >= need:
                    short.append((oe, method, mutant, d))
    assert not short, (need, short)
