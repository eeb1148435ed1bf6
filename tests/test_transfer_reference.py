"""Pins tests/transfer_reference.py on the CPU: against a dense interpolation matrix of the whole level built entry by entry from the
definition, against the oracle's interpolation matrices, against numpy.linalg.qr, and the device layouts against their index
formulas written out."""
import numpy as np
import pytest
import transfer_reference as tr
from oracle import mg_oracle as mo

L, A = [4, 4, 4, 8], [2, 2, 2, 4]
LC = tr.coarse_lattice(L, A)
V, VC = int(np.prod(L)), int(np.prod(LC))


def rand_c(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def dense_P(P, L_, A_):
    """(nd V) x (2N Vc), entry by entry: row nd x + d, column 2N a + h N + j with a the aggregate of x from its coordinates"""
    N, V_, nd = P.shape
    Lc = [l // a for l, a in zip(L_, A_)]
    M = np.zeros((nd * V_, 2 * N * int(np.prod(Lc))), dtype=complex)
    for x in range(V_):
        c = np.unravel_index(x, L_)
        a = np.ravel_multi_index([ci // ai for ci, ai in zip(c, A_)], Lc)
        for d in range(nd):
            h = 0 if d < nd // 2 else 1
            for j in range(N):
                M[nd * x + d, 2 * N * a + h * N + j] = P[j, x, d]
    return M


@pytest.mark.parametrize("nd,N", [(12, 3), (8, 2), (20, 5)])
def test_restrict_and_interpolate_against_a_dense_matrix(nd, N):
    rng = np.random.default_rng(nd)
    L_, A_ = [2, 4, 2, 4], [1, 2, 2, 2]
    V_ = int(np.prod(L_)); Vc = V_ // int(np.prod(A_))
    P = rand_c(rng, N, V_, nd)
    M = dense_P(P, L_, A_)
    phi, phic, phi0 = rand_c(rng, 3, V_, nd), rand_c(rng, 3, Vc, 2 * N), rand_c(rng, V_, nd)
    for w in range(3):
        ref_r = (M.conj().T @ phi[w].reshape(-1)).reshape(Vc, 2 * N)
        ref_i = (M @ phic[w].reshape(-1)).reshape(V_, nd)
        assert np.abs(tr.restrict(P, phi[w], L_, A_) - ref_r).max() < 1e-12
        assert np.abs(tr.interpolate(P, phic[w], L_, A_) - ref_i).max() < 1e-12
        assert np.abs(tr.interpolate(P, phic[w], L_, A_, phi0) - ref_i - phi0).max() < 1e-12
    assert np.array_equal(tr.restrict(P, phi, L_, A_)[1], tr.restrict(P, phi[1], L_, A_))
    assert np.array_equal(tr.interpolate(P, phic, L_, A_)[2], tr.interpolate(P, phic[2], L_, A_))
    # integer input: exact, and the bound covers every result
    Pi = rng.integers(-3, 4, (N, V_, nd)) + 1j * rng.integers(-3, 4, (N, V_, nd))
    fi = rng.integers(-4, 5, (V_, nd)) + 1j * rng.integers(-4, 5, (V_, nd))
    r = tr.restrict(Pi, fi, L_, A_)
    assert np.array_equal(r, (dense_P(Pi, L_, A_).conj().T @ fi.reshape(-1)).reshape(Vc, 2 * N))
    assert max(np.abs(r.real).max(), np.abs(r.imag).max()) <= tr.restrict_bound(Pi, fi, L_, A_)


def test_against_the_oracles_interpolation_matrices():
    rng = np.random.default_rng(5)
    N = 4
    P = rand_c(rng, N, V, 12)
    M = mo.interpolation_matrix(L, LC, tr.reim(P))
    phi, phic = rand_c(rng, V, 12), rand_c(rng, VC, 2 * N)
    assert np.abs(tr.restrict(P, phi, L, A) - (M.conj().T @ phi.reshape(-1)).reshape(VC, 2 * N)).max() < 1e-12
    assert np.abs(tr.interpolate(P, phic, L, A) - (M @ phic.reshape(-1)).reshape(V, 12)).max() < 1e-12
    assert np.array_equal(tr.aggregate_of(L, A), mo.aggregate_of(L, LC))
    n1 = 8
    Pc = rand_c(rng, N, V, n1)
    Mc = mo.coarse_interpolation_matrix(L, LC, tr.reim(Pc), n1)
    phi = rand_c(rng, V, n1)
    assert np.abs(tr.restrict(Pc, phi, L, A) - (Mc.conj().T @ phi.reshape(-1)).reshape(VC, 2 * N)).max() < 1e-12
    assert np.abs(tr.interpolate(Pc, phic, L, A) - (Mc @ phic.reshape(-1)).reshape(V, n1)).max() < 1e-12


def test_face_compacted_form():
    rng = np.random.default_rng(6)
    N = 3
    P, W5 = rand_c(rng, N, V, 12), rand_c(rng, 2, 5, V, 12)
    res = tr.restrict5_compact(P, W5, L, A)
    assert res.shape == (2, 5, VC, 2 * N)
    S = int(np.prod(A))
    order = tr.members(L, A).reshape(-1)          # a site order with contiguous aggregates
    parts = tr.compact_sites(order, L, A, 0, VC)
    assert [len(p) for p in parts] == [V] + [V // A[mu] for mu in range(4)]
    co = tr.coords(L)
    for mu in range(4):
        # a face site: its +mu neighbour has another coarse coordinate, or wraps around
        nxt = co[parts[1 + mu]].copy(); nxt[:, mu] += 1
        assert np.all(nxt[:, mu] // A[mu] != co[parts[1 + mu]][:, mu] // A[mu])
        only = np.zeros((V, 12), dtype=complex); only[parts[1 + mu]] = W5[1, 1 + mu][parts[1 + mu]]
        assert np.array_equal(res[1, 1 + mu], tr.restrict(P, only, L, A))
    assert np.array_equal(res[0, 0], tr.restrict(P, W5[0, 0], L, A))
    slab = tr.compact_sites(order, L, A, 1, 2)
    assert len(slab[0]) == 2 * S and set(tr.aggregate_of(L, A)[slab[0]]) == {1, 2}


def test_tile_layout():
    nt, n = 3, 20
    M = np.arange(nt * nt * 64).reshape(nt, nt, 8, 8)           # [tile row][tile column][row in tile][column in tile]
    for row in range(n):
        for col in range(n):
            assert tr.tile_offset(row, col, nt) == M[row // 8, col // 8, row % 8, col % 8]
    rng = np.random.default_rng(7)
    res = rand_c(rng, 3, 5, 2, n)
    csite = np.array([1, 0])
    out = tr.matrices_with_columns(res, csite, nt, nt * nt * 64, 9, -2.5)
    touched = np.zeros(out.shape[:3], dtype=bool)
    for c in range(3):
        for p in range(5):
            for xl in range(2):
                for row in range(n):
                    o = M[row // 8, (9 + c) // 8, row % 8, (9 + c) % 8]
                    assert out[csite[xl], p, o, 0] == res[c, p, xl, row].real and out[csite[xl], p, o, 1] == res[c, p, xl, row].imag
                    touched[csite[xl], p, o] = True
    assert np.all(out[~touched] == -2.5)


def test_device_layouts():
    rng = np.random.default_rng(8)
    L_, A_ = [2, 2, 2, 4], [1, 2, 2, 2]
    V_, S = 32, 8
    site_of_lex = rng.permutation(V_)
    x = rng.standard_normal((V_, 24))
    P = rng.standard_normal((3, V_, 24))
    for CH in (4, 2):
        dv = tr.fine_device_vector(x, site_of_lex, CH)
        dP = tr.fine_device_P(P, site_of_lex, S, CH)
        for xl in range(V_):
            s = site_of_lex[xl]
            a, i = s // S, s % S
            for r in range(24):
                assert dv[((r // CH) * V_ + s) * CH + r % CH] == x[xl, r]
                for j in range(3):
                    assert dP[(a * 3 + j) * 24 * S + ((r // CH) * S + i) * CH + r % CH] == P[j, xl, r]


@pytest.mark.parametrize("passes", [1, 2])
@pytest.mark.parametrize("nd,N", [(12, 5), (8, 4)])
def test_gram_schmidt_against_qr(passes, nd, N):
    rng = np.random.default_rng(9 + nd)
    L_, A_ = [4, 4, 2, 4], [2, 2, 2, 2]
    tv = rand_c(rng, N, int(np.prod(L_)), nd)
    Pq = tr.gram_schmidt(tv, L_, A_, passes)
    Bq, Bt = tr.blocks(Pq, L_, A_), tr.blocks(tv, L_, A_)
    for a in range(Bq.shape[0]):
        for h in range(2):
            Q, R = np.linalg.qr(Bt[a, h])
            ph = np.diag(R) / np.abs(np.diag(R))               # the phase convention: R with a positive real diagonal
            assert np.abs(Bq[a, h] - Q * ph[None, :]).max() < 1e-13
    assert tr.orthonormality(Pq, L_, A_).max() < 1e-14
    R = tr.coefficients(Pq, tv, L_, A_)
    assert np.abs(np.tril(R, -1)).max() < 1e-13
    d = np.diagonal(R, axis1=2, axis2=3)
    assert np.all(d.real > 0) and np.abs(d.imag).max() < 1e-13
    # the summation order changes nothing beyond rounding, in fp64 and in the fp32 model
    perm = rng.permutation(Bq.shape[2])
    assert np.abs(tr.gram_schmidt(tv, L_, A_, passes, order=perm) - Pq).max() < 1e-13
    P32 = tr.gram_schmidt(tv, L_, A_, passes, dtype=np.float32)
    assert P32.dtype == np.complex64 and 1e-9 < np.abs(P32 - Pq).max() < 1e-5
