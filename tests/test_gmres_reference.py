"""Pins tests/gmres_reference.py (the fp64 numpy GMRES the device solver is compared with) against numpy.linalg.  No GPU."""
import numpy as np
import pytest
import gmres_reference as gr

N = 1546


def krylov_basis(A, b, j):
    """orthonormal basis of span{b, A b, .., A^(j-1) b}: Arnoldi with Gram-Schmidt applied twice (independent of the solver)"""
    Q = np.zeros((len(b), j), complex)
    Q[:, 0] = b / np.linalg.norm(b)
    for k in range(1, j):
        w = A @ Q[:, k - 1]
        for _ in range(2):
            w = w - Q[:, :k] @ (Q[:, :k].conj().T @ w)
        Q[:, k] = w / np.linalg.norm(w)
    return Q


@pytest.fixture(scope="module")
def system():
    return gr.dense_op(N), gr.right_hand_side(N)


def test_operator_matches_its_definition(system):
    A, _ = system
    k = 5
    d5 = 3 + ((7 * k) % 11) / 11 + 1j * (((5 * k) % 13) / 13 - 0.5)
    assert A[k, k] == d5 and A[k, k + 1] == 0.4 - 0.3j and A[k, k - 1] == -0.2 + 0.5j
    assert A[N - 1, 0] == 0.4 - 0.3j and A[0, N - 1] == -0.2 + 0.5j
    assert np.count_nonzero(A) == 3 * N


def test_residual_is_the_least_squares_minimum(system):
    """after j steps of the first cycle the recurrence's residual is min ||b - A K y|| over the Krylov space, to 1e-12"""
    A, b = system
    out = gr.gmres(b, 1e-10, restart=10, num_restart=1)
    assert out["iter"] == 10
    Q = krylov_basis(A, b, 10)
    for j in range(1, 11):
        y = np.linalg.lstsq(A @ Q[:, :j], b, rcond=None)[0]
        best = np.linalg.norm(b - A @ Q[:, :j] @ y) / np.linalg.norm(b)
        assert abs(out["history"][j - 1] - best) < 1e-12, (j, out["history"][j - 1], best)


def test_flexible_residual_is_the_minimum_over_the_kept_iterates(system):
    """right preconditioning with a preconditioner that changes at every call: the residual after j steps of a cycle is the
    minimum of ||r0 - A Z y|| over the kept Z_0..Z_j, in the restarted cycles too"""
    A, b = system
    trace = []
    out = gr.gmres(b, 1e-10, prec=gr.VariableJacobi(N), trace=trace)
    assert len(trace) == out["iter"] == len(out["history"]) and out["iter"] > 10
    for (ol, j, Z, r0, x0), h in zip(trace, out["history"]):
        y = np.linalg.lstsq(A @ Z, r0, rcond=None)[0]
        best = np.linalg.norm(r0 - A @ Z @ y) / out["norm_r0"]
        assert abs(h - best) < 1e-12, (ol, j, h, best)


@pytest.mark.parametrize("prec", [False, True])
@pytest.mark.parametrize("tol", [1e-10, 1e-5])
@pytest.mark.parametrize("guess", [False, True])
def test_solution_matches_a_direct_solve(system, prec, tol, guess):
    A, b = system
    xs = np.linalg.solve(A, b)
    x0 = 0.25 * gr.right_hand_side(N, seed=12) if guess else None
    out = gr.gmres(b, tol, prec=gr.VariableJacobi(N) if prec else None, x0=x0)
    assert 0 < out["iter"] < 80 and out["history"][-1] < tol
    assert np.linalg.norm(A @ out["x"] - b) / out["norm_r0"] < 1.01 * tol
    assert np.linalg.norm(out["x"] - xs) / np.linalg.norm(xs) < np.linalg.cond(A) * tol
    # no entry of the residual history sits so close to the tolerance that a rounding error could move the iteration count
    assert np.all(np.abs(out["history"] / tol - 1) > 0.05)


@pytest.mark.parametrize("form", ["single", "pipelined"])
def test_other_arnoldi_forms_are_the_same_algorithm(system, form):
    """norm from sqrt(<w,w> - sum |h_i|^2): the same residuals while the difference is well conditioned (the first steps), the
    same solution at the end"""
    A, b = system
    ref = gr.gmres(b, 1e-10)
    out = gr.gmres(b, 1e-10, form=form)
    assert out["iter"] == ref["iter"]
    assert np.allclose(out["history"][:5], ref["history"][:5], rtol=1e-8, atol=0)
    assert np.linalg.norm(A @ out["x"] - b) / out["norm_r0"] < 1.01e-10
    assert np.linalg.norm(out["x"] - ref["x"]) / np.linalg.norm(ref["x"]) < 1e-10


def test_negative_norm_ends_the_cycle():
    """fp32 vectors in the pipelined form drive <w,w> - sum |h_i|^2 negative on this problem: the cycle ends with the columns
    completed so far, the step is not counted, and the next cycle still converges"""
    b = gr.right_hand_side(N)
    out = gr.gmres(b, 1e-5, form="pipelined", fp32=True)
    ref = gr.gmres(b, 1e-5, form="pipelined")
    assert ref["iter"] == 8 and out["iter"] == 11 and len(out["history"]) == 11
    assert np.linalg.norm(gr.apply_op(out["x"]) - b) / out["norm_r0"] < 2e-5


def test_zero_right_hand_side_and_breakdown():
    out = gr.gmres(np.zeros(N, complex), 1e-10)
    assert out["iter"] == 0 and out["gamma_jp1"] == 0 and not out["x"].any()
    e = np.zeros(N, complex); e[17] = 2.0
    out = gr.gmres(e, 1e-10, diag_only=True)
    assert out["iter"] == 1 and len(out["history"]) == 0
    assert np.allclose(out["x"], e / gr.diagonal(N), rtol=1e-15, atol=0)
