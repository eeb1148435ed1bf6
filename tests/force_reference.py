"""numpy restatement of the fermion force (include/ddamg_hip.h, "Forces") from links: hopping term, clover term and log det of the
clover blocks.  Independent of the library: it is pinned against finite differences of the oracle (test_force_reference.py) and is
what the GPU tests compare the kernels with.

Links: W_mu(x) = U_mu(x) with the anti-periodic sign on the T-links of the last time slice.  Varying W_mu(x) -> exp(eps Omega) W_mu(x),
a real function S changes by  sum Re tr(Omega_mu(x) M_mu(x)); the force is G = TA(M).  Fields are [T, Z, Y, X, ...] arrays, directions
and lexicographic order T, Z, Y, X with X fastest; spinors [V][12][2] reals, component 3 * spin + colour."""
import numpy as np

# gamma_mu in the basis of the operator (the reference's BASIS0): row i has one entry VAL[mu][i] in column COL[mu][i]
COL = [[2, 3, 0, 1], [3, 2, 1, 0], [3, 2, 1, 0], [2, 3, 0, 1]]
VAL = [[-1, -1, -1, -1], [-1j, -1j, 1j, 1j], [-1, 1, 1, -1], [-1j, 1j, 1j, -1j]]
GAMMA = np.zeros((4, 4, 4), dtype=np.complex128)
for _mu in range(4):
    for _i in range(4):
        GAMMA[_mu, _i, COL[_mu][_i]] = VAL[_mu][_i]
PLANES = [(mu, nu) for mu in range(4) for nu in range(mu + 1, 4)]
# the four leaves of Q_mu_nu at a corner y in the order of factors of the operator's field strength: (link: 0 = mu or 1 = nu, its site
# relative to y in steps of mu and of nu, daggered)
LEAVES = [[(0, 0, 0, 0), (1, 1, 0, 0), (0, 0, 1, 1), (1, 0, 0, 1)],
          [(1, 0, 0, 0), (0, -1, 1, 1), (1, -1, 0, 1), (0, -1, 0, 0)],
          [(0, -1, 0, 1), (1, -1, -1, 1), (0, -1, -1, 0), (1, 0, -1, 0)],
          [(1, 0, -1, 1), (0, 0, -1, 0), (1, 1, -1, 0), (0, 0, 0, 1)]]


def dag(m):
    return np.conj(np.swapaxes(m, -1, -2))


def ta(m):
    """the traceless anti-Hermitian part of 3x3 matrices"""
    a = 0.5 * (m - dag(m))
    return a - np.trace(a, axis1=-2, axis2=-1)[..., None, None] * np.eye(3) / 3.0


def links(L, U, anti_pbc):
    """[T, Z, Y, X, 4, 3, 3] complex from the caller's [V][4][9][2] reals, the sign applied"""
    W = (np.asarray(U, dtype=np.float64).reshape(*L, 4, 3, 3, 2)[..., 0] + 1j * np.asarray(U, dtype=np.float64).reshape(*L, 4, 3, 3, 2)[..., 1]).copy()
    if anti_pbc:
        W[L[0] - 1, :, :, :, 0] *= -1.0
    return W


def spinor(L, v):
    v = np.asarray(v, dtype=np.float64).reshape(*L, 4, 3, 2)
    return v[..., 0] + 1j * v[..., 1]


def parity(L):
    t, z, y, x = np.meshgrid(*[np.arange(n) for n in L], indexing="ij")
    return (t + z + y + x) % 2


def at(f, mu, d):
    """the field at x + d * mu"""
    return np.roll(f, -d, axis=mu) if d else f


def factor(W, mu, nu, step):
    """one factor of a leaf as a field over the leaf's corner"""
    w, dm, dn, dg = step
    m = at(at(W[..., mu if w == 0 else nu, :, :], mu, dm), nu, dn)
    return dag(m) if dg else m


def field_strength(W):
    """F_p = (Q_p - Q_p^dagger) / 16 for the six planes, [6][T, Z, Y, X, 3, 3]"""
    out = []
    for mu, nu in PLANES:
        Q = 0
        for leaf in LEAVES:
            f = [factor(W, mu, nu, s) for s in leaf]
            Q = Q + f[0] @ f[1] @ f[2] @ f[3]
        out.append((Q - dag(Q)) / 16.0)
    return out


def clover_term(L, W, m0, csw, scale=(1.0, 1.0)):
    """C(x) as [T, Z, Y, X, 12, 12] complex, row and column 3 * spin + colour"""
    C = np.zeros((*L, 4, 3, 4, 3), dtype=np.complex128)
    for s in range(4):
        for a in range(3):
            C[..., s, a, s, a] = 4.0 + m0
    for (mu, nu), F in zip(PLANES, field_strength(W)):
        C -= csw * np.einsum("st,...ab->...satb", GAMMA[mu] @ GAMMA[nu], F)
    s = np.where(parity(L) == 1, scale[1], scale[0])
    return C.reshape(*L, 12, 12) * s[..., None, None]


def clover_derivative(W, A):
    """M_mu(x) of  sum_x sum_p Re tr[Q_p(x) A_p(x)]  (A: six fields of 3x3 matrices), [T, Z, Y, X, 4, 3, 3]: every factor of every
    leaf in turn, the rotation of the leaf that starts at it, moved from the leaf's corner to the site of the link"""
    M = np.zeros(W.shape, dtype=np.complex128)
    for (mu, nu), Ap in zip(PLANES, A):
        for leaf in LEAVES:
            f = [factor(W, mu, nu, s) for s in leaf]
            for k, (w, dm, dn, dg) in enumerate(leaf):
                first = k + 1 if dg else k
                R = Ap
                for j in range(3, first - 1, -1):
                    R = f[j] @ R
                for j in range(first):
                    R = R @ f[j]
                M[..., mu if w == 0 else nu, :, :] += (-1.0 if dg else 1.0) * at(at(R, mu, -dm), nu, -dn)
    return M


def hopping_derivative(L, W, Y, X):
    """M_mu(x) of the hopping part of Re <Y, D X>"""
    M = np.zeros(W.shape, dtype=np.complex128)
    one = np.eye(4)
    for mu in range(4):
        Xn, Yn = at(X, mu, 1), at(Y, mu, 1)
        P = np.einsum("st,...tc,...sa->...ca", one - GAMMA[mu], Xn, np.conj(Y))
        Pb = np.einsum("st,...tc,...sa->...ca", one + GAMMA[mu], X, np.conj(Yn))
        Wm = W[..., mu, :, :]
        M[..., mu, :, :] = -0.5 * Wm @ P + 0.5 * Pb @ dag(Wm)
    return M


def force_bilinear(L, U, anti_pbc, m0, csw, y, x, scale=(1.0, 1.0), parts="both"):
    """the force of Re <y, D x>, [V][4][9][2] reals; parts: "both", "hopping" or "clover" """
    W, X, Y = links(L, U, anti_pbc), spinor(L, x), spinor(L, y)
    M = np.zeros(W.shape, dtype=np.complex128)
    if parts in ("both", "hopping"):
        M += hopping_derivative(L, W, Y, X)
    if parts in ("both", "clover") and csw != 0.0:
        s = np.where(parity(L) == 1, scale[1], scale[0])[..., None, None]
        A = []
        for mu, nu in PLANES:
            lam = np.einsum("st,...tb,...sa->...ba", GAMMA[mu] @ GAMMA[nu], X, np.conj(Y))
            A.append(-csw * s * (lam - dag(lam)) / 16.0)
        M += clover_derivative(W, A)
    return as_reals(ta(M))


def force_logdet(L, U, anti_pbc, m0, csw, par, scale=(1.0, 1.0)):
    """the force of the sum over the sites of parity `par` of log|det C(x)|"""
    W = links(L, U, anti_pbc)
    M = np.zeros(W.shape, dtype=np.complex128)
    if csw != 0.0:
        inv = np.linalg.inv(clover_term(L, W, m0, csw, scale)).reshape(*L, 4, 3, 4, 3)
        s = np.where(parity(L) == 1, scale[1], scale[0])[..., None, None]
        keep = (parity(L) == par)[..., None, None]
        A = []
        for mu, nu in PLANES:
            lam = np.einsum("st,...tbsa->...ba", GAMMA[mu] @ GAMMA[nu], inv)
            A.append(np.where(keep, -csw * s * (lam - dag(lam)) / 16.0, 0.0))
        M += clover_derivative(W, A)
    return as_reals(ta(M))


def as_reals(G):
    return np.stack([G.real, G.imag], axis=-1).reshape(-1, 4, 9, 2)


def as_matrices(g):
    g = np.asarray(g).reshape(-1, 4, 3, 3, 2)
    return g[..., 0] + 1j * g[..., 1]


def random_algebra(rng, shape):
    """traceless anti-Hermitian 3x3 matrices, entries of order one"""
    return ta(rng.standard_normal((*shape, 3, 3)) + 1j * rng.standard_normal((*shape, 3, 3)))


def exp_algebra(omega, eps):
    """exp(eps * omega) of anti-Hermitian matrices, through the eigenvectors of the Hermitian -i omega"""
    lam, v = np.linalg.eigh(-1j * omega)
    return (v * np.exp(1j * eps * lam)[..., None, :]) @ dag(v)


def perturbed(U, omega, eps):
    """exp(eps Omega_mu(x)) U_mu(x) for every link, as [V][4][9][2] reals; omega: [V][4][3][3]"""
    u = as_matrices(U)
    w = exp_algebra(omega, eps) @ u
    return np.stack([w.real, w.imag], axis=-1).reshape(-1, 4, 9, 2)


def pairing(omega, g):
    """sum_{x,mu} tr(Omega_mu(x) G_mu(x)): the derivative of S along omega, real"""
    return float(np.einsum("vmab,vmba->", omega, as_matrices(g)).real)


def richardson(S, h):
    """the central difference of S at step h extrapolated with that at 2 h: (4 d(h) - d(2h)) / 3, error O(h^4)"""
    d = lambda e: (S(e) - S(-e)) / (2.0 * e)
    return (4.0 * d(h) - d(2.0 * h)) / 3.0
