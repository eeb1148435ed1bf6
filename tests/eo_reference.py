"""numpy restatement of the even-odd preconditioned system, from existing pieces only: the oracle's D (orc.dirac_apply) and a numpy
inverse of the per-site 6x6 clover blocks.  Vectors are [V][12][2] real arrays in lexicographic order, as the library takes them;
the operator arrays are those of Context.get_operator()."""
import numpy as np
from oracle import orc

G5 = np.array([-1.0] * 6 + [1.0] * 6)[None, :, None]


def parity(L):
    """(t+z+y+x) mod 2 of every site in lexicographic order (T,Z,Y,X; X fastest)"""
    t, z, y, x = np.meshgrid(*[np.arange(n) for n in L], indexing="ij")
    return ((t + z + y + x) % 2).ravel()


def clover_blocks(cl):
    """[V][2][6][6] complex: the two Hermitian blocks of every site from the reference's packing ([V][42] complex: 12 diagonal
    entries, then the 15 strict-upper entries of block 0 in row-major order, then those of block 1)"""
    c = cl[..., 0] + 1j * cl[..., 1]
    V = c.shape[0]
    B = np.zeros((V, 2, 6, 6), dtype=np.complex128)
    iu = np.triu_indices(6, 1)
    for b in range(2):
        up = c[:, 12 + 15 * b:12 + 15 * (b + 1)]
        B[:, b, iu[0], iu[1]] = up
        B[:, b, iu[1], iu[0]] = up.conj()
        B[:, b, np.arange(6), np.arange(6)] = c[:, 6 * b:6 * (b + 1)].real
    return B


def blocks_mul(B, v):
    """(block 0 on spin-colour components 0..5, block 1 on 6..11) of every site"""
    z = (v[..., 0] + 1j * v[..., 1]).reshape(-1, 2, 6)
    w = np.einsum("vbij,vbj->vbi", B, z).reshape(-1, 12)
    return np.stack([w.real, w.imag], axis=-1)


def schur(L, D, cl, phi, dagger=False, rounded=False):
    """(Dhat phi_e on the even sites and 0 on the odd ones, the odd part of D (phi_e, psi_o) which must vanish, psi_o): psi_o =
    -D_oo^-1 [D (phi_e, 0)]_o, Dhat phi_e = [D (phi_e, psi_o)]_e.  dagger: gamma5 around it.  rounded: operator, input, the two
    intermediate vectors and the result rounded to fp32, the products in fp64 (what an fp32 kernel cannot do better than)."""
    r = (lambda a: a.astype(np.float32).astype(np.float64)) if rounded else (lambda a: a)
    odd = parity(L)[:, None, None] == 1
    inv = np.linalg.inv(clover_blocks(cl))
    D, cl = r(D), r(cl)
    inv = r(inv.real) + 1j * r(inv.imag)
    x = np.where(odd, 0.0, r(G5 * phi if dagger else phi))
    h = r(np.where(odd, orc.dirac_apply(L, D, cl, x, 64), 0.0))         # D_oe phi_e
    psi = r(-blocks_mul(inv, h))
    full = orc.dirac_apply(L, D, cl, x + psi, 64)
    out, rest = r(np.where(odd, 0.0, full)), np.where(odd, full, 0.0)
    return (G5 * out if dagger else out), rest, (G5 * psi if dagger else psi)


def schur_matrix(A, L):
    """(dense Dhat = A_ee - A_eo A_oo^-1 A_oe of a sparse full matrix A, the indices of the even unknowns): no library code and none
    of the functions above"""
    even = np.flatnonzero(np.repeat(parity(L), 12) == 0)
    odd = np.flatnonzero(np.repeat(parity(L), 12) == 1)
    A = A.tocsr()
    Aee, Aeo, Aoe, Aoo = (A[r][:, c].toarray() for r, c in ((even, even), (even, odd), (odd, even), (odd, odd)))
    return Aee - Aeo @ np.linalg.solve(Aoo, Aoe), even
