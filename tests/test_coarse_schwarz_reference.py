"""The references of tests/test_gpu_coarse_schwarz_shapes.py, checked on the CPU (tests/coarse_schwarz_reference.py says what they
are):

  * the vectorised restatement `CoarseSweep` in complex128 equals `mg_oracle.Schwarz` (plain-block MinRes on coarse_matrix) to
    rounding at every shape, dof count, schedule and start, with either precision's MinRes threshold, and no <Dr,Dr> comes closer
    than 3 % to a threshold, so that correct fp32 code decides every step as the fp64 reference does (the components of D r carry
    a relative rounding of a few 1e-7 each, which moves <Dr,Dr> by far less than 1 %);
  * the spread, the distance of the complex64 restatements in three summation orders from the fp64 reference, printed per case;
    its maximum is LARGEST_SPREAD, from which the GPU test takes its fp32 bar, and ten times it lies below TOL_SWEEP; the same in
    complex128 for the two permuted orders (LARGEST_SPREAD_FP64), ten times which lies below the fp64 bar of 1e-11;
  * the bar discriminates: five wrong smoothers lie more than one bar from the reference wherever they can differ;
  * the eps-guard inputs (eta zero on two blocks) give the same finite result in both restatements;
  * the shape list reaches every branch of the fused block solver's launch rule and kernel, according to `path`."""
import numpy as np
import pytest
import coarse_schwarz_reference as cr

_SPREAD, _SPREAD64 = {}, {}


@pytest.fixture(scope="module", params=cr.CASES, ids=[f"{name}-n{n}" for name, n in cr.CASES])
def case(request):
    yield request.param
    cr.forget(*request.param)


def combos():
    return [(m, st) for m in cr.METHODS for st in cr.STARTS]


def spreads(name, n):
    if (name, n) not in _SPREAD:
        _SPREAD[(name, n)] = {c: cr.spread(name, n, *c) for c in combos()}
        # the permuted fp64 orders where the spread is largest, red-black
        _SPREAD64[(name, n)] = {c: cr.spread_fp64(name, n, *c) for c in combos() if c == (2, cr.PERMUTED_START)}
    return _SPREAD[(name, n)]


@pytest.mark.parametrize("n", sorted({n for _, n in cr.CASES}))
def test_the_ordered_products_are_products(n):
    """the tile-by-tile, lane-by-lane sums of CoarseSweep in complex128 against numpy's matrix product, which the complex128
    sweeps in the kernel's order use in their place; in complex64 they lie an fp32 rounding from it"""
    rng = np.random.default_rng(n)
    M = rng.uniform(-1, 1, (7, n, n)) + 1j * rng.uniform(-1, 1, (7, n, n)); v = rng.uniform(-1, 1, (7, n)) + 1j * rng.uniform(-1, 1, (7, n))
    blas = cr.Products(n, np.complex128, cr.KERNEL_ORDER, blas=True)
    g5 = np.concatenate([np.ones(n // 2), -np.ones(n // 2)])
    assert cr.relerr(blas.mv(M.real, M.imag, v), np.einsum("xij,xj->xi", M, v)) < 1e-14
    assert cr.relerr(blas.mv_dag(M.real, M.imag, v), g5 * np.einsum("xji,xj->xi", M.conj(), g5 * v)) < 1e-14
    for order in cr.ORDERS:
        for ct, tol in ((np.complex128, 1e-14), (np.complex64, 1e-6)):
            P = cr.Products(n, ct, order)
            Mr, Mi, vt = M.real.astype(P.rt), M.imag.astype(P.rt), v.astype(ct)
            assert P.mv(Mr, Mi, vt).dtype == ct and P.mv_dag(Mr, Mi, vt).dtype == ct
            assert cr.relerr(P.mv(Mr, Mi, vt), blas.mv(M.real, M.imag, v)) < tol
            assert cr.relerr(P.mv_dag(Mr, Mi, vt), blas.mv_dag(M.real, M.imag, v)) < tol
    plain = cr.Products(n, np.complex128, cr.KERNEL_ORDER, g5_signs=False, blas=True)
    assert cr.relerr(plain.mv_dag(M.real, M.imag, v), np.einsum("xji,xj->xi", M.conj(), v)) < 1e-14


def test_sweep_restates_the_oracle(case):
    name, n = case
    eta, phi0 = (cr.cvec(v) for v in cr.vectors(name, n))
    worst, margin = 0.0, np.inf
    for method, start in combos():
        cycles, guess = cr.STARTS[start]
        for prec in (32, 64) if cycles == 3 else (32,):       # the thresholds only matter once the residual is small
            sw = cr.CoarseSweep(name, n, cr.schwarz(name, n, method, prec))
            d = cr.relerr(sw.smooth(eta, cycles, phi0 if guess else None), cr.reference(name, n, method, start, prec))
            worst, margin = max(worst, d), min(margin, sw.margin)
            assert d < 1e-12, (method, start, prec, d)
            assert sw.margin > 0.03, (method, start, prec, sw.margin)
    print(f"{name} n {n}: CoarseSweep in complex128 vs mg_oracle.Schwarz {worst:.2e}; closest <Dr,Dr> to a threshold: off by a factor {1 + margin:.3g}")


def test_eps_guard_case(case):
    """eta zero on a block of either colour: <Dr,Dr> is exactly zero there, the step is skipped, the result is finite"""
    name, n = case
    eta = cr.cvec(cr.guard_eta(name, n))
    for prec in (32, 64):
        ref = cr.guard_reference(name, n, prec)
        sw = cr.CoarseSweep(name, n, cr.schwarz(name, n, 2, prec))
        got = sw.smooth(eta, 1)
        assert np.all(np.isfinite(ref)) and np.all(np.isfinite(got))
        assert cr.relerr(got, ref) < 1e-12 and sw.margin > 0.03
    S = cr.schwarz(name, n, 2, 32)
    b0 = cr.guard_blocks(name, n)[0]
    assert not np.any(ref[S.blocks[b0]["I"]])          # the first colour's block had nothing to solve
    got32 = cr.CoarseSweep(name, n, S, np.complex64).smooth(eta, 1)
    d = cr.relerr(got32, cr.guard_reference(name, n, 32))
    print(f"{name} n {n}: eps-guard case, complex64 restatement {d:.3e} from the reference")
    assert np.all(np.isfinite(got32)) and d <= cr.LARGEST_SPREAD


def test_spread(case):
    name, n = case
    sp = spreads(name, n)
    for (method, start), s in sp.items():
        print(f"spread {name:5s} n {n:2d} method {method} {start:14s} {s:.3e}")
    s64 = max(_SPREAD64[(name, n)].values())
    print(f"spread {name} n {n}: largest {max(sp.values()):.3e}; fp32 bar {cr.fp32_bar():.3e}; permuted fp64 orders {s64:.3e}")
    assert max(sp.values()) <= cr.LARGEST_SPREAD * (1 + 1e-3)
    assert s64 <= cr.LARGEST_SPREAD_FP64 * (1 + 1e-3)
    # rounding the operator and the input alone moves the result by a few 1e-8: a spread below that would not be one of an fp32 sweep
    assert min(sp.values()) > 3e-8


# cycles from zero at which each wrong smoother is run: the fewest at which it can differ
MUTANTS = {"iter3": 1, "no45": 1, "stale": 2, "nog5": 1, "drop": 1}


def test_the_bar_tells_wrong_smoothers_apart(case):
    """every schedule the mutant exists for; "no45" is a rule of the red-black schedule and needs a block of list 4 or 5 (second
    colour, no face on the upper lattice boundary), which two blocks per direction do not have"""
    name, n = case
    eta = cr.cvec(cr.vectors(name, n)[0])
    B, L, _ = cr.geometry(name, n)
    short = []
    for method in cr.METHODS:
        S = cr.schwarz(name, n, method, 32)
        ref = {c: S.smooth(eta, c) for c in set(MUTANTS.values())}
        lists45 = any(b["colour"] == 1 and b["list"] in (4, 5) for b in S.blocks)
        assert method != 2 or lists45 == any(L[mu] // B[mu] > 2 for mu in range(4))
        for mutant, cycles in MUTANTS.items():
            if mutant == "no45" and not (method == 2 and lists45):
                continue
            d = cr.relerr(cr.CoarseSweep(name, n, S, mutant=mutant).smooth(eta, cycles), ref[cycles])
            print(f"mutant {name:5s} n {n:2d} method {method} {mutant:6s} {cycles} from zero {d:.3e} = {d / cr.fp32_bar():.0f} bars")
            if not d > cr.fp32_bar():
                short.append((method, mutant, d))
    assert not short, (cr.fp32_bar(), short)


def test_the_recorded_spreads_are_the_largest_and_the_bars_lie_below_the_old_ones():
    for name, n in cr.CASES:
        fresh = (name, n) not in _SPREAD
        spreads(name, n)
        if fresh:
            cr.forget(name, n)
    largest = max(max(v.values()) for v in _SPREAD.values()); largest64 = max(max(v.values()) for v in _SPREAD64.values())
    print(f"largest spread {largest:.4e}, recorded {cr.LARGEST_SPREAD:.4e}, fp32 bar {cr.fp32_bar():.3e}, TOL_SWEEP {cr.TOL_SWEEP:.1e}; "
          f"permuted fp64 orders {largest64:.4e}, recorded {cr.LARGEST_SPREAD_FP64:.4e}, fp64 bar {cr.fp64_bar():.1e}")
    assert abs(largest / cr.LARGEST_SPREAD - 1) < 1e-3 and abs(largest64 / cr.LARGEST_SPREAD_FP64 - 1) < 1e-3
    assert cr.fp32_bar() <= cr.TOL_SWEEP
    assert cr.fp64_bar() == 1e-11


def test_the_shapes_reach_every_branch_of_the_block_solver():
    """by the Python restatement of CoarseOp<T>::block_minres: it names the path every case is expected to take"""
    p32 = {c: cr.path(cr.geometry(*c)[0], c[1], 32) for c in cr.CASES}
    p64 = {c: cr.path(cr.geometry(*c)[0], c[1], 64) for c in cr.CASES}
    for c in cr.CASES:
        print(f"{c[0]:5s} n {c[1]:2d}: fp32 {cr.path_name(cr.geometry(*c)[0], c[1], 32)}; fp64 {cr.path_name(cr.geometry(*c)[0], c[1], 64)}")
    f32 = [p for p in p32.values() if p["fused"]]; f64 = [p for p in p64.values() if p["fused"]]
    for fused in (f32, f64):
        assert {p["NT"] for p in fused} == set(range(1, 9))                     # every instantiation
        assert {p["resident"] for p in fused} == {True, False}
        assert {p["items_in_lds"] for p in fused} == {True, False}
        assert {p["padded"] for p in fused} == {True, False}
    assert {p["trips"] for p in f32} == {1, 2, 3, 4}
    assert any(p["fused"] and p["NT"] <= 6 and p["nitems"] < 16 for p in p32.values())       # BS < 8: hopping items among the first eight
    assert any(p["NT"] == 7 and cr.block_sites(c[0]) == 8 for c, p in p32.items())
    # the step-by-step form for either reason, in either precision, and the largest fused launches
    for pp in (p32, p64):
        assert any(p["by_size"] for p in pp.values())
    assert any(p["by_lds"] and not p["by_size"] for p in p64.values())
    assert p64[("24", 48)]["lds"] == 150 * 1024 + 384 and p64[("24", 40)]["fused"]
    assert p64[("16", 64)]["fused"] and p64[("16", 64)]["lds"] == 131456
    assert p32[("64", 32)]["fused"] and p32[("64", 32)]["lds"] == 147840 and p32[("64", 32)]["nitems"] == 224
    assert not p32[("64", 34)]["fused"] and p64[("64", 16)]["fused"] and not p64[("64", 24)]["fused"]
    assert p32[("32-x", 64)]["fused"] and p32[("32-x", 64)]["trips"] == 4 and p32[("32-x", 64)]["nitems"] == 104
    assert not p64[("32-x", 64)]["fused"] and not p64[("32-x", 40)]["fused"] and p64[("32-x", 32)]["fused"]
    assert p32[("24", 64)]["fused"] and p32[("24", 64)]["trips"] == 3
    assert p32[("128", 8)]["fused"] and not p32[("128", 16)]["fused"] and not p64[("128", 8)]["fused"]
    # the 16-bit kernel: two, one and no resident self couplings per wavefront; all of a block, 8 or 16 of them resident
    half = {(p["half"], p["nres"]) for c, p in p32.items() if p["fused"] and cr.block_sites(c[0]) in (2, 8, 16, 32) and c[1] in (16, 40, 48, 56)}
    assert {h for h, _ in half} == {0, 1, 2} and {r for _, r in half} >= {2, 8, 16}
