"""A coarse operator in numpy, matrix by matrix, and the way back into the reference's storage.

CoarseMatrices decodes what ddamg_hip_get_coarse_operator returns into the nine dense couplings of every site; pack() is the
inverse direction, dense couplings -> the storage CoarseOp::import_reference reads; integer_operator() makes couplings whose
products with integer vectors are exact in fp32 in any summation order (tests/test_gpu_many_rhs_kernels.py)."""
import numpy as np


def _triu_column_major(N):
    """row and column index of triu(.) packed column by column: (0,0) (0,1) (1,1) (0,2) ..."""
    iu = np.triu_indices(N)
    order = np.lexsort((iu[0], iu[1]))
    return iu[0][order], iu[1][order]


def pack(M0, U, Lc):
    """dense couplings -> (D_lex [V][4][n*n][2], clover_lex [V][n(n+1)/2][2]), the reference's storage that
    CoarseOp::import_reference reads: per link the blocks A, C, B, D column-major; per site triu(A), triu(D) packed column by
    column, then B column-major.  M0 [V][n][n] must be [[A, B], [-B^H, D]] with Hermitian A and D; U [V][4][n][n]."""
    M0 = np.asarray(M0); U = np.asarray(U)
    V, n = M0.shape[0], M0.shape[1]; N = n // 2
    assert V == int(np.prod(Lc)) and M0.shape == (V, n, n) and U.shape == (V, 4, n, n) and n % 2 == 0
    A, B, C, Dd = M0[:, :N, :N], M0[:, :N, N:], M0[:, N:, :N], M0[:, N:, N:]
    assert np.array_equal(A, A.conj().transpose(0, 2, 1)) and np.array_equal(Dd, Dd.conj().transpose(0, 2, 1)), "A and D must be Hermitian"
    assert np.array_equal(C, -B.conj().transpose(0, 2, 1)), "the lower left block must be -B^H"
    ti, tj = _triu_column_major(N)
    clc = np.concatenate([A[:, ti, tj], Dd[:, ti, tj], B.transpose(0, 2, 1).reshape(V, N * N)], axis=1)
    Dc = np.empty((V, 4, 4, N, N), dtype=complex)
    for q, (bi, bj) in enumerate([(0, 0), (1, 0), (0, 1), (1, 1)]):
        Dc[:, :, q] = U[:, :, bi * N:(bi + 1) * N, bj * N:(bj + 1) * N].transpose(0, 1, 3, 2)
    Dc = Dc.reshape(V, 4, n * n)
    return np.stack([Dc.real, Dc.imag], axis=-1), np.stack([clc.real, clc.imag], axis=-1)


def integer_operator(n, Lc, seed, lo=-3, hi=3):
    """(M0, U) with integer real and imaginary parts in [lo, hi], seeded, different on every site and direction; M0 of the form
    [[A, B], [-B^H, D]], A and D Hermitian with a real diagonal"""
    rng = np.random.default_rng(seed)
    V = int(np.prod(Lc)); N = n // 2

    def ints(*shape):
        return rng.integers(lo, hi + 1, size=shape).astype(np.float64) + 1j * rng.integers(lo, hi + 1, size=shape).astype(np.float64)

    def hermitian():
        up = np.triu(ints(V, N, N), 1)
        return up + up.conj().transpose(0, 2, 1) + np.eye(N) * rng.integers(lo, hi + 1, size=(V, N, 1))

    M0 = np.zeros((V, n, n), dtype=complex)
    B = ints(V, N, N)
    M0[:, :N, :N] = hermitian(); M0[:, N:, N:] = hermitian()
    M0[:, :N, N:] = B; M0[:, N:, :N] = -B.conj().transpose(0, 2, 1)
    return M0, ints(V, 4, n, n)


class CoarseMatrices:
    """the nine couplings of every site of level 1 from ddamg_hip_get_coarse_operator (lexicographic sites, the reference's
    storage): mats[m][x] with m = 0 the self coupling, 1 + mu the forward link U_mu(x), 5 + mu the backward coupling
    G5 U_mu(x - mu)^H G5; src[m][x] the site whose vector entries matrix m of site x multiplies; sign[m] its sign in D_c"""

    def __init__(self, ctx):
        D, cl = ctx.get_coarse_operator()
        n = ctx.ndof(1); N = n // 2
        Lc = [int(v) for v in ctx.params.local_lattice[1]]
        V = int(np.prod(Lc))
        Dc = (D[..., 0] + 1j * D[..., 1]).reshape(V, 4, 4, N, N)       # [site][mu][block A, C, B, D][column][row]
        clc = cl[..., 0] + 1j * cl[..., 1]
        tri = N * (N + 1) // 2
        iu = np.triu_indices(N)
        order = np.lexsort((iu[0], iu[1]))                             # packed column by column: (0,0) (0,1) (1,1) (0,2) ...
        ti, tj = iu[0][order], iu[1][order]
        M0 = np.zeros((V, n, n), dtype=complex)
        for b in range(2):
            blk = np.zeros((V, N, N), dtype=complex)
            blk[:, tj, ti] = np.conj(clc[:, b * tri:(b + 1) * tri])
            blk[:, ti, tj] = clc[:, b * tri:(b + 1) * tri]
            M0[:, b * N:(b + 1) * N, b * N:(b + 1) * N] = blk
        B = clc[:, 2 * tri:2 * tri + N * N].reshape(V, N, N).transpose(0, 2, 1)
        M0[:, :N, N:] = B
        M0[:, N:, :N] = -B.conj().transpose(0, 2, 1)
        U = np.zeros((V, 4, n, n), dtype=complex)
        for q, (bi, bj) in enumerate([(0, 0), (1, 0), (0, 1), (1, 1)]):
            U[:, :, bi * N:(bi + 1) * N, bj * N:(bj + 1) * N] = Dc[:, :, q].transpose(0, 1, 3, 2)
        g5 = np.concatenate([np.ones(N), -np.ones(N)])
        coords = np.stack(np.unravel_index(np.arange(V), Lc), axis=1)
        self.mats, self.src, self.sign = [M0], [np.arange(V)], [1.0]
        fwd = []
        for mu in range(4):
            c = coords.copy(); c[:, mu] = (c[:, mu] + 1) % Lc[mu]
            fwd.append(np.ravel_multi_index(c.T, Lc))
            self.mats.append(U[:, mu]); self.src.append(fwd[mu]); self.sign.append(-1.0)
        for mu in range(4):
            c = coords.copy(); c[:, mu] = (c[:, mu] - 1) % Lc[mu]
            bwd = np.ravel_multi_index(c.T, Lc)
            self.mats.append(g5[None, :, None] * U[bwd, mu].conj().transpose(0, 2, 1) * g5[None, None, :])
            self.src.append(bwd); self.sign.append(-1.0)
        self.V, self.n = V, n

    def apply(self, x):
        """D_c x in fp64; x: [V][n][2]"""
        xc = x[..., 0] + 1j * x[..., 1]
        y = sum(s * np.einsum("xij,xj->xi", M, xc[src]) for M, src, s in zip(self.mats, self.src, self.sign))
        return np.stack([y.real, y.imag], axis=-1)

    def bound(self, x, first=0):
        """B of the module docstring, [V][n] (the same for the real and the imaginary part of a component); first = 1: the sums
        over the eight hopping terms only"""
        ax = np.abs(x[..., 0]) + np.abs(x[..., 1])
        B = np.zeros((self.V, self.n))
        for M, src in zip(self.mats[first:], self.src[first:]):
            s = np.maximum(np.abs(M.real).max(axis=(1, 2)), np.abs(M.imag).max(axis=(1, 2)))
            B += 2.0 ** -10 * np.einsum("xij,xj->xi", np.abs(M.real) + np.abs(M.imag), ax[src])
            B += 2.0 ** -23 * (s * ax[src].sum(axis=1))[:, None]
        return B


class HostOperator:
    """what CoarseMatrices needs of a context, for a coarse operator that exists on the host only: the storage of pack() on the
    lattice Lc with n dof per site"""

    class _Params:
        pass

    def __init__(self, D, cl, n, Lc):
        self._D, self._cl, self._n = D, cl, n
        self.params = HostOperator._Params()
        self.params.local_lattice = [None, list(Lc)]

    def get_coarse_operator(self):
        return self._D, self._cl

    def ndof(self, level=1):
        return self._n


class IntegerOperator:
    """integer couplings on the lattice Lc, their storage for set_coarse_operator, and the operator in int64:
    mats / src / sign as CoarseMatrices has them, real and imaginary parts as integer arrays"""

    def __init__(self, n, Lc, seed):
        self.n, self.Lc, self.V = n, [int(v) for v in Lc], int(np.prod(Lc))
        M0, U = integer_operator(n, self.Lc, seed)
        self.D, self.cl = pack(M0, U, self.Lc)
        cm = CoarseMatrices(HostOperator(self.D, self.cl, n, self.Lc))
        self.src, self.sign = cm.src, [int(s) for s in cm.sign]
        self.re = [np.rint(M.real).astype(np.int8) for M in cm.mats]        # parts in [-3, 3]: a byte each
        self.im = [np.rint(M.imag).astype(np.int8) for M in cm.mats]
        assert all(np.array_equal(r, M.real) and np.array_equal(i, M.imag) for r, i, M in zip(self.re, self.im, cm.mats))
        self.odd = np.stack(np.unravel_index(np.arange(self.V), self.Lc), axis=1).sum(axis=1) % 2 == 1

    def terms(self, x, which):
        """sum over the couplings `which` (indices into mats, without their signs) of M x[src] as int64, and the largest
        magnitude any partial sum can reach, max sum |M| |x|; x: [V][n][2] or [cols][V][n][2] of integers.
        The products run as fp64 matrix products: every operand is an integer and every sum stays below 2^53 by many orders of
        magnitude (it is asserted below 2^24 by the callers), so they are exact, and the result converts to int64 as it is"""
        x = np.asarray(x, dtype=np.float64)
        assert np.array_equal(x, np.rint(x))
        many = x.ndim == 4
        xs = x if many else x[None]
        xr, xi = xs[..., 0].transpose(1, 2, 0), xs[..., 1].transpose(1, 2, 0)          # [V][n][cols]
        yr = np.zeros(xr.shape); yi = np.zeros(xr.shape); mag = np.zeros(xr.shape)
        for m in which:
            re, im = self.re[m].astype(np.float64), self.im[m].astype(np.float64)
            sr, si = xr[self.src[m]], xi[self.src[m]]
            yr += re @ sr - im @ si
            yi += re @ si + im @ sr
            mag += (np.abs(re) + np.abs(im)) @ (np.abs(sr) + np.abs(si))
        y = np.stack([yr, yi], axis=-1).transpose(2, 0, 1, 3)                           # [cols][V][n][2]
        assert mag.max() < 2.0 ** 53 and np.array_equal(y, np.rint(y))
        y = y.astype(np.int64)
        return (y if many else y[0]), int(mag.max())

    def apply(self, x):
        """D_c x = M0 x - hopping terms, int64, with the bound on every partial sum"""
        s, m0 = self.terms(x, [0])
        h, m1 = self.terms(x, range(1, 9))
        return s - h, m0 + m1
