"""The numpy multi-shift CG the GPU tests compare with (multishift_reference.py), checked on the CPU against dense solves: 4^4,
the Schur complement S of the oracle's matrix, Q = S^dagger S, seven shifts over five decades, at two masses.

Bars.  A shift stops on |zeta_s| ||r|| <= tol ||b||, the recursed residual of (Q + sigma_s) x_s = b, so the error of x_s against
the dense solution is at most cond(Q + sigma_s) tol.  Ritz values are eigenvalues of an orthogonal projection of Q (plus the base
shift, which is subtracted), so they lie inside [lambda_min, lambda_max] of Q; the slack 1e-10 (relative to lambda_max) is for the
orthogonality the recurrence loses in fp64.  The iteration counts are pinned as found: they are what the GPU tests take to +- 1."""
import os, sys
import numpy as np
import pytest
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import synth
from oracle import orc, mg_oracle as mo
import multishift_reference as ms

L = [4, 4, 4, 4]
SHIFTS = [0.0, 1e-3, 1e-2, 0.1, 1.0, 10.0, 100.0]
TOL = 1e-10
COUNTS = {0.3: [34, 34, 34, 33, 30, 18, 9], -0.1: [44, 44, 44, 43, 37, 19, 9]}
_system = {}


def system(m0):
    """(Q, b) at the mass, made once"""
    if m0 not in _system:
        V = int(np.prod(L))
        U = synth.synth_gauge(list(L), 0.35, 5).reshape(V, 4, 9, 2)
        D, cl, _ = orc.gauge_to_operator(L, U, 1, m0, 1.0)
        Q, _ = ms.dense_normal_operator(mo.fine_matrix(L, D, cl), L)
        rng = np.random.default_rng(3)
        b = rng.uniform(-0.5, 0.5, Q.shape[0]) + 1j * rng.uniform(-0.5, 0.5, Q.shape[0])
        _system[m0] = (Q, b)
    return _system[m0]


@pytest.mark.parametrize("m0", [0.3, -0.1])
def test_every_shift_against_the_dense_solution(m0):
    Q, b = system(m0)
    x, its, al, be, hist, T = ms.multishift_cg(lambda v: Q @ v, b, SHIFTS, TOL)
    ev = np.linalg.eigvalsh(Q)
    print("m0", m0, "lambda", ev[0], ev[-1], "iterations", list(its))
    assert list(its) == COUNTS[m0]
    assert len(al) == len(be) == len(hist) == max(its) and T.shape == (max(its), max(its))
    for s, sigma in enumerate(SHIFTS):
        A = Q + sigma * np.eye(len(b))
        want = np.linalg.solve(A, b)
        err = np.linalg.norm(x[s] - want) / np.linalg.norm(want)
        true = np.linalg.norm(b - A @ x[s]) / np.linalg.norm(b)
        cond = (ev[-1] + sigma) / (ev[0] + sigma)
        print(" shift", sigma, "error", err, "bar", cond * TOL, "true residual", true)
        assert err <= cond * TOL and true <= 2 * TOL
    lo, hi = ms.ritz_extremes(T, min(SHIFTS))
    rayleigh = (np.vdot(b, Q @ b) / np.vdot(b, b)).real
    print(" ritz", lo, hi, "rayleigh", rayleigh)
    slack = 1e-10 * ev[-1]
    assert ev[0] - slack <= lo <= rayleigh <= hi <= ev[-1] + slack


def test_the_sparse_operator_is_the_dense_one():
    """sparse_normal_operator, which the GPU tests use on the larger lattices, against S^dagger S of the dense Schur complement"""
    V = int(np.prod(L))
    U = synth.synth_gauge(list(L), 0.35, 5).reshape(V, 4, 9, 2)
    D, cl, _ = orc.gauge_to_operator(L, U, 1, -0.1, 1.0)
    A = mo.fine_matrix(L, D, cl)
    op, even = ms.sparse_normal_operator(A, L)
    Q, even2 = system(-0.1)[0], ms.dense_normal_operator(A, L)[1]
    b = system(-0.1)[1]
    assert np.array_equal(even, even2)
    assert np.linalg.norm(op(b) - Q @ b) <= 1e-13 * np.linalg.norm(Q @ b)


def test_freezing_order_and_tolerances():
    """a frozen shift is left alone: stopping the whole run at its count gives its bits; the position of a shift and its company do not
    matter; looser tolerances stop earlier; a starved run reports the length of the loop; b = 0"""
    Q, b = system(0.3)
    op = lambda v: Q @ v
    x, its, *_ = ms.multishift_cg(op, b, SHIFTS, TOL)
    y, jts, *_ = ms.multishift_cg(op, b, SHIFTS, TOL, max_iterations=int(its[-1]))
    assert np.array_equal(y[-1], x[-1]) and list(jts) == [its[-1]] * len(SHIFTS)
    z, kts, *_ = ms.multishift_cg(op, b, [100.0, 0.0, 1.0, 1.0], TOL)
    assert np.array_equal(z[0], x[6]) and np.array_equal(z[1], x[0]) and np.array_equal(z[2], x[4]) and np.array_equal(z[3], z[2])
    assert list(kts) == [its[6], its[0], its[4], its[4]]
    tols = [1e-10, 1e-6, 1e-10, 1e-4, 1e-10, 1e-8, 1e-10]
    w, lts, *_ = ms.multishift_cg(op, b, SHIFTS, tols)
    assert all(lts[s] < its[s] for s in (1, 3, 5)) and all(lts[s] == its[s] for s in (0, 2, 4, 6))
    zero, nts, al, be, hist, T = ms.multishift_cg(op, 0 * b, SHIFTS, TOL)
    assert not zero.any() and not nts.any() and hist == [] and T.shape == (0, 0)
