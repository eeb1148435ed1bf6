"""The Galerkin construction D_c = P^H D P in numpy, part by part, on numbers fp64 holds exactly (tests/test_gpu_galerkin_exact.py;
pinned by tests/test_galerkin_reference.py against oracle/mg_oracle.py).  Not a test module.

A level's operator is nine couplings per site, D v(x) = sum_m mats[m][x] v(src[m][x]) with the signs folded into the matrices:
m = 0 the site's own term, 1 + mu the coupling to x + mu, 5 + mu the coupling to x - mu.  fine_couplings() reads them off the
pinned C oracle; coarse_couplings() takes them from coarse_reference.IntegerOperator.  PartwiseGalerkin splits them by
COORDINATES into the part that stays inside an aggregate, the four parts that leave it through the +mu face and the four that
leave it through the -mu face, and restricts every part by itself with P per chirality -- so the forward and the backward coupling
of an aggregate never mix, also where the coarse extent is 2 and both lead to the same neighbour.

Every input has real and imaginary parts that are multiples of `1 / unit` (unit = 2 on the fine level: links 0, +-1/2, +-i/2;
unit = 1 between coarse levels), P is integer, and all sums stay many orders of magnitude below 2^53: fp64 is exact here.
`bound` is the largest sum |P| |part| |P| over all entries of all parts (|z| = |re z| + |im z|), in units of 1 / unit: no partial
sum of any entry, in any order of summation, exceeds it.  Below 2^24 it makes fp32 exact as well."""
import numpy as np


def coords_of(L):
    """[V][4] coordinates of the lexicographic sites (T, Z, Y, X; X fastest)"""
    return np.stack(np.unravel_index(np.arange(int(np.prod(L))), L), axis=1)


def neighbours(L):
    """src[m] of the nine couplings: the site itself, x + mu for m = 1 + mu, x - mu for m = 5 + mu"""
    c = coords_of(L)
    src = [np.arange(len(c))]
    for sgn in (+1, -1):
        for mu in range(4):
            d = c.copy(); d[:, mu] = (d[:, mu] + sgn) % L[mu]
            src.append(np.ravel_multi_index(d.T, L))
    return src


def monomial_gauge(L, seed):
    """[V][4][9][2]: every link one of the 96 SU(3) matrices with entries 0, +-1, +-i (link_pivot_form.monomial_su3), a draw per
    link and direction"""
    from link_pivot_form import monomial_su3
    M = monomial_su3()
    V = int(np.prod(L))
    U = M[np.random.default_rng(seed).integers(0, len(M), V * 4)].reshape(V, 4, 9)
    return np.ascontiguousarray(np.stack([U.real, U.imag], -1))


def integer_clover(V, seed):
    """[V][42][2], the storage of set_operator (12 diagonal entries, then the strict upper triangles of the two 6x6 blocks row by
    row): diagonal 8 or 9, off-diagonal parts in [-1, 1] -- Hermitian by the storage, diagonally dominant (8 > 5 * 2^(1/2)), so
    the inverses of the blocks exist"""
    rng = np.random.default_rng(seed)
    cl = np.zeros((V, 42, 2))
    cl[:, :12, 0] = rng.integers(8, 10, size=(V, 12))
    cl[:, 12:] = rng.integers(-1, 2, size=(V, 30, 2))
    return cl


def fine_couplings(L, D, clover):
    """mats [9][V][12][12] complex of the Wilson-Clover operator (D [V][36][2], clover [V][42][2]) from the pinned C oracle's apply:
    the clover term with the links zeroed (12 applies), then every direction by itself with the other links and the clover term
    zeroed -- the operator is linear in them --, sources on every fourth plane of that direction (4 x 12 applies): the plane before
    a source plane receives the forward coupling, the plane behind it the backward one"""
    from oracle import orc
    L = [int(v) for v in L]
    assert all(v % 4 == 0 for v in L), "four planes between two sources of a colour"
    V = int(np.prod(L))
    D = np.asarray(D, dtype=np.float64).reshape(V, 4, 9, 2)
    c = coords_of(L); src = neighbours(L)
    mats = np.zeros((9, V, 12, 12), dtype=complex)
    zero_cl = np.zeros((V, 42, 2))

    def apply(Dm, cl, e):
        y = orc.dirac_apply(L, Dm.reshape(V, 36, 2), cl, e, 64)
        return y[..., 0] + 1j * y[..., 1]

    for d in range(12):
        e = np.zeros((V, 12, 2)); e[:, d, 0] = 1.0
        mats[0, :, :, d] = apply(np.zeros_like(D), clover, e)
    for mu in range(4):
        Dm = np.zeros_like(D); Dm[:, mu] = D[:, mu]
        for col in range(4):
            on = c[:, mu] % 4 == col
            before = c[:, mu] % 4 == (col - 1) % 4; behind = c[:, mu] % 4 == (col + 1) % 4
            assert np.all(on[src[1 + mu][before]]) and np.all(on[src[5 + mu][behind]])
            for d in range(12):
                e = np.zeros((V, 12, 2)); e[on, d, 0] = 1.0
                y = apply(Dm, zero_cl, e)
                assert not np.any(y[~(before | behind)])
                mats[1 + mu, before, :, d] = y[before]
                mats[5 + mu, behind, :, d] = y[behind]
    return mats


def coarse_couplings(op):
    """mats [9][V][n][n] complex of a coarse_reference.IntegerOperator, its signs folded in"""
    return np.stack([s * (r.astype(np.float64) + 1j * i.astype(np.float64)) for s, r, i in zip(op.sign, op.re, op.im)])


def interpolation_blocks(P, n):
    """Pd [V][n][2 N] complex from interpolation vectors P [N][V][n][2]: column h N + j holds the dofs of chirality h (the first or
    the second half of a site's n) of vector j"""
    P = np.asarray(P, dtype=np.float64)
    N, V = P.shape[0], P.shape[1]
    Pc = (P[..., 0] + 1j * P[..., 1]).transpose(1, 2, 0)          # [V][n][N]
    Pd = np.zeros((V, n, 2 * N), dtype=complex)
    Pd[:, :n // 2, :N] = Pc[:, :n // 2]
    Pd[:, n // 2:, N:] = Pc[:, n // 2:]
    return Pd


def _a(z):
    return np.abs(z.real) + np.abs(z.imag)


class PartwiseGalerkin:
    """The next level's operator from the couplings `mats` of the lattice L, aggregates L / Lc and the interpolation blocks Pd:
    M0 [Vc][nc][nc], U [Vc][4][nc][nc] (the reference's forward links: D_c y(X) = M0 y(X) - sum_mu U_mu(X) y(X + mu) - ...) and
    Bk [Vc][4][nc][nc], the backward couplings restricted by themselves, not derived from U.  mats / src / sign as
    coarse_reference.IntegerOperator has them, for terms() and apply()."""

    def __init__(self, L, Lc, mats, Pd, unit):
        L = [int(v) for v in L]; Lc = [int(v) for v in Lc]
        V, Vc = int(np.prod(L)), int(np.prod(Lc))
        nf, nc = Pd.shape[1], Pd.shape[2]
        assert mats.shape == (9, V, nf, nf) and Pd.shape[0] == V and all(l % k == 0 for l, k in zip(L, Lc))
        ext = [l // k for l, k in zip(L, Lc)]
        c = coords_of(L)
        agg = np.ravel_multi_index((c // np.array(ext)).T, Lc)
        order = np.argsort(agg, kind="stable")                   # the sites aggregate by aggregate
        src = neighbours(L)
        self.L, self.Lc, self.V, self.n, self.unit = L, Lc, Vc, nc, unit
        self.src, self.sign = neighbours(Lc), [1] + [-1] * 8
        self.odd = coords_of(Lc).sum(axis=1) % 2 == 1
        aPd = _a(Pd)

        def restrict(S):
            """sum over the sites of every aggregate of Pd(x)^H S(x)"""
            k = (V // Vc) * nf
            return np.matmul(Pd[order].reshape(Vc, k, nc).conj().transpose(0, 2, 1), S[order].reshape(Vc, k, nc))

        def restrict_abs(S):
            k = (V // Vc) * nf
            return np.matmul(aPd[order].reshape(Vc, k, nc).transpose(0, 2, 1), S[order].reshape(Vc, k, nc))

        S = np.matmul(mats[0], Pd); aS = np.matmul(_a(mats[0]), aPd)
        parts, bound = [None] * 9, 0.0
        for m in range(1, 9):
            mu = (m - 1) % 4
            leaves = c[:, mu] % ext[mu] == (ext[mu] - 1 if m < 5 else 0)          # through the +mu (-mu) face of the aggregate
            assert Lc[mu] >= 2 and np.array_equal(leaves, agg[src[m]] != agg)
            T = np.matmul(mats[m], Pd[src[m]]); aT = np.matmul(_a(mats[m]), aPd[src[m]])
            S[~leaves] += T[~leaves]; aS[~leaves] += aT[~leaves]
            T[~leaves] = 0; aT[~leaves] = 0
            parts[m] = restrict(T)
            bound = max(bound, float(restrict_abs(aT).max()))
            # the part couples aggregate X to one aggregate only, the neighbour of X in that direction
            assert np.array_equal(np.unique(np.stack([agg[leaves], agg[src[m]][leaves]], 1), axis=0)[:, 1], self.src[m])
        parts[0] = restrict(S)
        bound = max(bound, float(restrict_abs(aS).max()))
        self.bound = int(round(bound * unit))
        self.M0 = parts[0]
        self.U = -np.stack(parts[1:5], axis=1)
        self.Bk = -np.stack(parts[5:9], axis=1)
        self.mats = [self.M0] + [self.U[:, mu] for mu in range(4)] + [self.Bk[:, mu] for mu in range(4)]
        for M in self.mats:
            assert np.array_equal(M * unit, np.rint(M * unit))

    def storage(self):
        """(D_lex, clover_lex) as get_coarse_operator returns them"""
        from coarse_reference import pack
        return pack(self.M0, self.U, self.Lc)

    def dense(self):
        """the whole level as one dense matrix, index n X + dof"""
        n, V = self.n, self.V
        G = np.zeros((V * n, V * n), dtype=complex)
        for M, src, s in zip(self.mats, self.src, self.sign):
            for X in range(V):
                Y = src[X]
                G[n * X:n * (X + 1), n * Y:n * (Y + 1)] += s * M[X]
        return G

    def terms(self, x, which):
        """sum over the couplings `which` (without their signs) of M x[src], [V][n][2] in fp64 (exact: multiples of 1 / unit), and
        the largest sum |M| |x| of a component in units of 1 / unit; x: [V][n][2] of integers"""
        x = np.asarray(x, dtype=np.float64)
        assert np.array_equal(x, np.rint(x))
        xc = x[..., 0] + 1j * x[..., 1]
        y = np.zeros(xc.shape, dtype=complex); mag = np.zeros(xc.shape)
        for m in which:
            y += np.einsum("xij,xj->xi", self.mats[m], xc[self.src[m]])
            mag += np.einsum("xij,xj->xi", _a(self.mats[m]), _a(xc[self.src[m]]))
        return np.stack([y.real, y.imag], axis=-1), int(round(mag.max() * self.unit))

    def apply(self, x):
        """D_c x and the bound on every partial sum"""
        s, m0 = self.terms(x, [0])
        h, m1 = self.terms(x, range(1, 9))
        return s - h, m0 + m1
