"""oracle/site_ops.py -- TEST INFRASTRUCTURE ONLY: the Wilson-Clover operator at a list of sites, in fp64, straight from the
gauge field.

(D phi)(x) = C(x) phi(x) - 1/2 sum_mu [ (1 - gamma_mu) (x) U_mu(x) phi(x+mu) + (1 + gamma_mu) (x) U_mu(x-mu)^H phi(x-mu) ]
C(x)       = (4 + m0) - csw sum_{mu<nu} (gamma_mu gamma_nu) (x) (Q_mu,nu(x) - Q_nu,mu(x)),   Q = four plaquette leaves / 16

in the conventions of oracle/ddamg_oracle.c: lexicographic sites (T,Z,Y,X; X fastest), dof = 3 spin + colour, the same gamma
basis, and the anti-periodic time boundary as a minus sign on the T links of the last time slice (hopping and clover alike).

Nothing here builds the whole operator: every function gathers the links and spinors of the sites it needs only, so the
operator can be checked at sampled sites of a 64^4 lattice, where the gauge field alone is 9.6 GB.  `U` and `phi` may be full
arrays or callables idx -> values (`Patch` holds a field on a subset of sites).
"""
import numpy as np

# gamma matrices: row s has the single entry GV[mu][s] in column GC[mu][s] (the basis of oracle/ddamg_oracle.c)
GC = [[2, 3, 0, 1], [3, 2, 1, 0], [3, 2, 1, 0], [2, 3, 0, 1]]
GV = [[-1, -1, -1, -1], [-1j, -1j, 1j, 1j], [-1, 1, 1, -1], [-1j, 1j, 1j, -1j]]
GAMMA = np.zeros((4, 4, 4), dtype=complex)
for _mu in range(4):
    for _s in range(4):
        GAMMA[_mu, _s, GC[_mu][_s]] = GV[_mu][_s]


def coords_of(L, sites):
    s = np.asarray(sites, dtype=np.int64)
    c = np.empty(s.shape + (4,), dtype=np.int64)
    for mu in (3, 2, 1, 0):
        c[..., mu] = s % L[mu]; s = s // L[mu]
    return c


def lex_of(L, c):
    return ((c[..., 0] * L[1] + c[..., 1]) * L[2] + c[..., 2]) * L[3] + c[..., 3]


def _shift(L, c, steps):
    """coordinates c moved by steps {mu: delta}, periodic"""
    c = c.copy()
    for mu, d in steps.items():
        c[..., mu] = (c[..., mu] + d) % L[mu]
    return c


def link_sites(L, sites):
    """every site whose links (D phi)(x) reads, for x in `sites`: x, x-mu, and the corners of the clover leaves"""
    c = coords_of(L, sites)
    out = [np.asarray(sites, dtype=np.int64)]
    for mu in range(4):
        out.append(lex_of(L, _shift(L, c, {mu: -1})))
        for nu in range(4):
            if nu != mu:
                for dm, dn in ((1, 0), (1, -1), (-1, 1), (-1, -1)):
                    out.append(lex_of(L, _shift(L, c, {mu: dm, nu: dn})))
    return np.unique(np.concatenate([o.ravel() for o in out]))


def spinor_sites(L, sites):
    """every site whose spinor (D phi)(x) reads: x and x +- mu"""
    c = coords_of(L, sites)
    out = [np.asarray(sites, dtype=np.int64)]
    for mu in range(4):
        for d in (1, -1):
            out.append(lex_of(L, _shift(L, c, {mu: d})))
    return np.unique(np.concatenate([o.ravel() for o in out]))


class Patch:
    """a field known on the sorted lexicographic sites `idx` only; called with site indices like a full array is indexed"""

    def __init__(self, field, idx):
        self.idx = np.unique(np.asarray(idx, dtype=np.int64))
        self.val = np.ascontiguousarray(field[self.idx])

    def __call__(self, sites):
        sites = np.asarray(sites, dtype=np.int64)
        k = np.searchsorted(self.idx, sites)
        k = np.minimum(k, len(self.idx) - 1)
        if not np.all(self.idx[k] == sites):
            raise KeyError("Patch: site outside the stored set")
        return self.val[k]


def _getter(a):
    return a if callable(a) else (lambda idx: a[idx])


def _cplx(a):
    a = np.asarray(a)
    return a if np.iscomplexobj(a) else a[..., 0] + 1j * a[..., 1]


def _links(U, L, c, mu, anti_pbc, steps=None):
    """U_mu at the sites c + steps, [n][3][3] complex, with the anti-periodic sign on the last time slice"""
    cc = _shift(L, c, steps) if steps else c
    u = _cplx(U(lex_of(L, cc))).reshape(cc.shape[:-1] + (4, 3, 3))[..., mu, :, :]
    if anti_pbc and mu == 0:
        u = np.where((cc[..., 0] == L[0] - 1)[..., None, None], -u, u)
    return u


def _leaves(U, L, c, mu, nu, anti_pbc):
    """Q_mu,nu(x): the four plaquette leaves in the (mu, nu) plane at x, / 16"""
    H = lambda a: np.conj(np.swapaxes(a, -1, -2))
    at = lambda m, dm, dn: _links(U, L, c, m, anti_pbc, {mu: dm, nu: dn})
    q = at(mu, 0, 0) @ at(nu, 1, 0) @ H(at(mu, 0, 1)) @ H(at(nu, 0, 0))
    q = q + at(nu, 0, 0) @ H(at(mu, -1, 1)) @ H(at(nu, -1, 0)) @ at(mu, -1, 0)
    q = q + H(at(mu, -1, 0)) @ H(at(nu, -1, -1)) @ at(mu, -1, -1) @ at(nu, 0, -1)
    q = q + H(at(nu, 0, -1)) @ at(mu, 0, -1) @ at(nu, 1, -1) @ H(at(mu, 0, 0))
    return q / 16.0


def clover_sites(L, U, sites, m0, csw, anti_pbc=True):
    """the 12x12 site matrices C(x) of `sites`, [n][12][12] complex (index 3 spin + colour)"""
    U = _getter(U)
    c = coords_of(L, sites)
    C = np.zeros(c.shape[:-1] + (12, 12), dtype=complex)
    C[..., np.arange(12), np.arange(12)] = 4.0 + m0
    if csw != 0.0:
        for mu in range(4):
            for nu in range(mu + 1, 4):
                qd = _leaves(U, L, c, mu, nu, anti_pbc) - _leaves(U, L, c, nu, mu, anti_pbc)
                gg = GAMMA[mu] @ GAMMA[nu]
                C -= csw * np.einsum("ab,...ij->...aibj", gg, qd).reshape(qd.shape[:-2] + (12, 12))
    return C


def dirac_sites(L, U, phi, sites, m0, csw, anti_pbc=True):
    """(D phi)(x) for x in `sites`, fp64: [n][12] complex, or [n][12][k] when phi(idx) returns [m][12][k] (k right-hand sides).
    U: [V][4][9][2] (or complex [V][4][9]) or a callable of site indices; phi: [V][12][2] (or complex) or a callable."""
    U = _getter(U); phi = _getter(phi)
    sites = np.asarray(sites, dtype=np.int64)
    c = coords_of(L, sites)
    ph = lambda cc: _cplx(phi(lex_of(L, cc)))
    p0 = ph(c)
    multi = p0.ndim == 3
    sp = lambda a: a.reshape(a.shape[0], 4, 3, *a.shape[2:])          # [n][spin][colour](k)
    out = np.einsum("nij,nj...->ni...", clover_sites(L, U, sites, m0, csw, anti_pbc), p0)
    out = sp(out)
    for mu in range(4):
        fw = sp(ph(_shift(L, c, {mu: 1})))
        bw = sp(ph(_shift(L, c, {mu: -1})))
        Uf = _links(U, L, c, mu, anti_pbc)
        Ub = np.conj(np.swapaxes(_links(U, L, c, mu, anti_pbc, {mu: -1}), -1, -2))
        Pm = np.eye(4) - GAMMA[mu]; Pp = np.eye(4) + GAMMA[mu]
        out -= 0.5 * np.einsum("st,nij,ntj...->nsi...", Pm, Uf, fw)
        out -= 0.5 * np.einsum("st,nij,ntj...->nsi...", Pp, Ub, bw)
    return out.reshape(len(sites), 12, *out.shape[3:]) if multi else out.reshape(len(sites), 12)


def per_site_error(got, ref):
    """max |got - ref| at a site / max |ref| at that site, for every site (rows of [n][12] complex or [n][12][2] real)"""
    got = _cplx(got).reshape(len(got), -1); ref = _cplx(ref).reshape(len(ref), -1)
    return np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)
