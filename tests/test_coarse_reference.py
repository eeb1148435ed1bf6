"""tests/coarse_reference.py against itself and against a brute-force dense matrix (no GPU): pack() is the inverse of the
decoding in CoarseMatrices, and CoarseMatrices.apply / IntegerOperator.apply are the level's operator
    D_c = M0 - sum_mu [ U_mu(x) delta_{x+mu} + G5 U_mu(x-mu)^H G5 delta_{x-mu} ]."""
import numpy as np
import pytest
from coarse_reference import CoarseMatrices, HostOperator, IntegerOperator, integer_operator, pack

LC = [2, 4, 4, 6]       # in the first direction the forward and the backward neighbour coincide; one extent is no power of two


@pytest.mark.parametrize("n", [4, 20, 64])
def test_decoding_of_pack_returns_the_dense_couplings(n):
    M0, U = integer_operator(n, LC, seed=100 + n)
    V = int(np.prod(LC)); N = n // 2
    assert np.all(np.abs(M0.real) <= 3) and np.all(np.abs(M0.imag) <= 3) and np.all(np.abs(U.real) <= 3) and np.all(np.abs(U.imag) <= 3)
    assert np.all(np.diagonal(M0, axis1=1, axis2=2).imag == 0)
    assert len({M0[x].tobytes() for x in range(V)}) == V and len({U[x, mu].tobytes() for x in range(V) for mu in range(4)}) == 4 * V
    D, cl = pack(M0, U, LC)
    assert D.shape == (V, 4, n * n, 2) and cl.shape == (V, n * (n + 1) // 2, 2)
    cm = CoarseMatrices(HostOperator(D, cl, n, LC))
    assert np.array_equal(cm.mats[0], M0)
    for mu in range(4):
        assert np.array_equal(cm.mats[1 + mu], U[:, mu])
    # the storage itself, entry by entry, as CoarseOp::import_reference reads it: blocks A, C, B, D of a link column-major
    x, mu, i, j = V - 1, 2, N - 1, 1 % N
    for q, (bi, bj) in enumerate([(0, 0), (1, 0), (0, 1), (1, 1)]):
        e = q * N * N + j * N + i
        assert D[x, mu, e, 0] + 1j * D[x, mu, e, 1] == U[x, mu, bi * N + i, bj * N + j]
    tri = N * (N + 1) // 2
    k = j * (j + 1) // 2 + 0                                         # element (0, j) of the packed upper triangles
    assert cl[x, k, 0] + 1j * cl[x, k, 1] == M0[x, 0, j] and cl[x, tri + k, 0] + 1j * cl[x, tri + k, 1] == M0[x, N, N + j]
    assert cl[x, 2 * tri + j * N + i, 0] + 1j * cl[x, 2 * tri + j * N + i, 1] == M0[x, i, N + j]


def test_pack_refuses_couplings_the_storage_cannot_hold():
    M0, U = integer_operator(4, LC, seed=1)
    bad = M0.copy(); bad[0, 0, 1] += 1
    with pytest.raises(AssertionError):
        pack(bad, U, LC)
    bad = M0.copy(); bad[0, 2, 0] += 1
    with pytest.raises(AssertionError):
        pack(bad, U, LC)


@pytest.mark.parametrize("n", [4, 20])
def test_apply_equals_the_dense_matrix_of_the_whole_level(n):
    op = IntegerOperator(n, LC, seed=7 + n)
    V, N = op.V, n // 2
    M0, U = integer_operator(n, LC, seed=7 + n)                      # the same couplings, dense
    g5 = np.diag(np.concatenate([np.ones(N), -np.ones(N)]))
    big = np.zeros((V * n, V * n), dtype=complex)
    coords = np.stack(np.unravel_index(np.arange(V), LC), axis=1)
    for x in range(V):
        big[x * n:(x + 1) * n, x * n:(x + 1) * n] += M0[x]
        for mu in range(4):
            c = coords[x].copy(); c[mu] = (c[mu] + 1) % LC[mu]
            y = int(np.ravel_multi_index(c, LC))
            big[x * n:(x + 1) * n, y * n:(y + 1) * n] -= U[x, mu]                               # x <- x + mu
            big[y * n:(y + 1) * n, x * n:(x + 1) * n] -= g5 @ U[x, mu].conj().T @ g5            # x + mu <- x
    rng = np.random.default_rng(5)
    xs = rng.integers(-4, 5, size=(3, V, n, 2)).astype(np.float64)
    ref = np.einsum("ab,cb->ca", big, (xs[..., 0] + 1j * xs[..., 1]).reshape(3, V * n)).reshape(3, V, n)
    cm = CoarseMatrices(HostOperator(op.D, op.cl, n, LC))
    for c in range(3):
        y = cm.apply(xs[c])
        assert np.array_equal(y[..., 0], ref[c].real) and np.array_equal(y[..., 1], ref[c].imag)     # integers: exact in fp64
        yi, mag = op.apply(xs[c])
        assert mag < 2 ** 24 and np.array_equal(yi, y)
    ymany, _ = op.apply(xs)
    assert np.array_equal(ymany[1], op.apply(xs[1])[0])
    # the pieces the parity-wise entry points return
    hop, _ = op.terms(xs[0], range(1, 9)); self_, _ = op.terms(xs[0], [0])
    assert np.array_equal(self_ - hop, op.apply(xs[0])[0])
    assert op.odd.sum() * 2 == V and not op.odd[0]
