"""tests/galerkin_reference.py against oracle/mg_oracle.py (no GPU): the couplings read off the oracle's apply are its sparse fine
matrix, and the part-wise restriction gives mo.galerkin_coarse_operator and the dense P^H A P -- on 4^4 over 2^4, where the forward
and the backward neighbour aggregate coincide in every direction, and on 4x4x4x8 over 2x2x2x4, where the last direction has
distinct ones.  Every input is a multiple of 1/2 or an integer, so every comparison is np.array_equal."""
import numpy as np
import pytest
import scipy.sparse as sp
import galerkin_reference as gr
from coarse_reference import IntegerOperator
from oracle import mg_oracle as mo, orc

CASES = {"4x4x4x4": ([4, 4, 4, 4], [2, 2, 2, 2]), "4x4x4x8": ([4, 4, 4, 8], [2, 2, 2, 4])}
N = 3
_fine = {}


def fine(lat):
    if lat not in _fine:
        L, Lc = CASES[lat]; V = int(np.prod(L))
        D, _, _ = orc.gauge_to_operator(L, gr.monomial_gauge(L, 11), 1, -1.0, 0.0)
        cl = gr.integer_clover(V, 12)
        A = mo.fine_matrix(L, D, cl)
        mats = gr.fine_couplings(L, D, cl)
        P = np.random.default_rng(13).integers(-2, 3, size=(N, V, 12, 2)).astype(np.float64)
        _fine[lat] = (D, cl, A, mats, P, gr.PartwiseGalerkin(L, Lc, mats, gr.interpolation_blocks(P, 12), unit=2))
    return _fine[lat]


def sparse_of(L, mats):
    """(site term, [forward hops of mu], [backward hops of mu]) as sparse matrices, index n x + dof"""
    V, n = mats.shape[1], mats.shape[2]
    src = gr.neighbours(L)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    out = []
    for m in range(9):
        rows = (n * np.arange(V)[:, None, None] + i).ravel(); cols = (n * src[m][:, None, None] + j).ravel()
        out.append(sp.csr_matrix((mats[m].ravel(), (rows, cols)), shape=(n * V, n * V)))
    return out[0], out[1:5], out[5:9]


@pytest.mark.parametrize("lat", CASES)
def test_couplings_from_the_oracle_are_its_fine_matrix(lat):
    L, _ = CASES[lat]
    D, cl, A, mats, _, _ = fine(lat)
    selfp, fwd, bwd = sparse_of(L, mats)
    B = selfp + sum(fwd) + sum(bwd)
    assert (A - B).count_nonzero() == 0 and A.nnz > 0
    assert np.array_equal(2 * mats, np.rint(2 * mats)) and np.abs(mats[1:]).max() == 0.5       # links 0, +-1/2, +-i/2
    assert np.array_equal(cl[..., 0] + 1j * cl[..., 1], gr_clover_of(mats[0]))


def gr_clover_of(M):
    """the 42 stored numbers of the site terms: diagonal, then the strict upper triangles of the two 6x6 blocks row by row"""
    iu = np.triu_indices(6, 1)
    return np.concatenate([np.diagonal(M, axis1=1, axis2=2), M[:, iu[0], iu[1]], M[:, 6 + iu[0], 6 + iu[1]]], axis=1)


@pytest.mark.parametrize("lat", CASES)
def test_fine_level_against_the_oracle(lat):
    L, Lc = CASES[lat]
    D, cl, A, mats, P, g = fine(lat)
    Pm = mo.interpolation_matrix(L, Lc, P)
    assert np.array_equal(g.dense(), (Pm.conj().T @ A @ Pm).toarray())
    Dref, clref = mo.galerkin_coarse_operator(L, Lc, sparse_of(L, mats), Pm, 2 * N)
    Dg, clg = g.storage()
    assert np.array_equal(Dg[..., 0] + 1j * Dg[..., 1], Dref) and np.array_equal(clg[..., 0] + 1j * clg[..., 1], clref)
    # the storage decodes to the same operator (mo.coarse_matrix derives the backward couplings from the forward links)
    assert np.array_equal(mo.coarse_matrix(Lc, Dg, clg, 2 * N).toarray(), g.dense())
    g5 = np.concatenate([np.ones(N), -np.ones(N)])
    for mu in range(4):
        assert np.array_equal(g.Bk[:, mu], g5[None, :, None] * g.U[g.src[5 + mu], mu].conj().transpose(0, 2, 1) * g5[None, None, :])
    if Lc[3] == 4:
        assert not np.array_equal(g.src[4], g.src[8])
    # the bound is one: no entry exceeds it, and it is the largest sum of absolute values of a restriction done by hand
    assert 2 * max(np.abs(M.real).max() for M in g.mats) <= g.bound < 2 ** 24
    x = np.random.default_rng(3).integers(-1, 2, size=(g.V, g.n, 2)).astype(np.float64)
    y, mag = g.apply(x)
    assert np.array_equal(y[..., 0] + 1j * y[..., 1], (g.dense() @ (x[..., 0] + 1j * x[..., 1]).ravel()).reshape(g.V, g.n))
    assert mag < 2 ** 24


def test_bound_against_the_undivided_sum_of_absolute_values():
    """|P|^T |A| |P| of the whole matrix is, entry by entry, the sum of the nine parts' (they partition the entries of A)"""
    lat = "4x4x4x4"; L, Lc = CASES[lat]
    D, cl, A, mats, P, g = fine(lat)
    Pm = mo.interpolation_matrix(L, Lc, P)
    aA = abs(A.real) + abs(A.imag); aP = abs(Pm.real) + abs(Pm.imag)
    whole = 2 * (aP.T @ aA @ aP).toarray()
    # the parts partition the entries of A, so their largest sum lies between the largest entry of a block row's share and the whole
    assert whole.max() / 9 <= g.bound <= whole.max()


@pytest.mark.parametrize("lat", CASES)
def test_between_coarse_levels_against_the_oracle(lat):
    L1, L2 = CASES[lat]; n1, N1 = 8, 3
    op = IntegerOperator(n1, L1, seed=21)
    P1 = np.random.default_rng(22).integers(-1, 2, size=(N1, op.V, n1, 2)).astype(np.float64)
    g = gr.PartwiseGalerkin(L1, L2, gr.coarse_couplings(op), gr.interpolation_blocks(P1, n1), unit=1)
    Pm = mo.coarse_interpolation_matrix(L1, L2, P1, n1)
    A = mo.coarse_matrix(L1, op.D, op.cl, n1)
    assert np.array_equal(g.dense(), (Pm.conj().T @ A @ Pm).toarray())
    Dref, clref = mo.galerkin_coarse_operator(L1, L2, mo.coarse_matrix(L1, op.D, op.cl, n1, parts=True), Pm, 2 * N1)
    Dg, clg = g.storage()
    assert np.array_equal(Dg[..., 0] + 1j * Dg[..., 1], Dref) and np.array_equal(clg[..., 0] + 1j * clg[..., 1], clref)
    assert max(np.abs(M.real).max() for M in g.mats) <= g.bound < 2 ** 24
