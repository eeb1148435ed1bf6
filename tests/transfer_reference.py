"""The transfers between two levels in plain numpy, from coordinates alone (tests/test_gpu_transfer_kernels.py compares the
kernels of transfer.hip and of the transfer half of coarse_mg.hip with them; tests/test_transfer_reference.py pins them on the CPU).

Sites are lexicographic (T, Z, Y, X; X fastest).  A vector of a level is complex [V][nd]: nd = 12 on the fine level, n = 2 Nvec of
the level below on a coarse one; the first half of a site's dofs is chirality 0.  Aggregate a is the box of extent A whose coarse
coordinates are coord // A, numbered lexicographically on the coarse lattice L / A.  P is [N][V][nd]; coarse dof h * N + j of
aggregate a couples to the chirality-h dofs of vector j on the sites of a.

Every function works on whatever numbers it is given: with integer-valued float64 input all sums are exact integers (far below
2^53), which is what the exact part of the GPU tests compares with bit for bit."""
import numpy as np


def cplx(a):
    a = np.asarray(a)
    return a[..., 0] + 1j * a[..., 1]


def reim(z):
    return np.stack([z.real, z.imag], axis=-1)


def coords(L):
    """[V][4] coordinates of the lexicographic sites"""
    return np.indices(L).reshape(4, -1).T


def lex(c, L):
    return ((c[..., 0] * L[1] + c[..., 1]) * L[2] + c[..., 2]) * L[3] + c[..., 3]


def coarse_lattice(L, A):
    assert all(l % a == 0 for l, a in zip(L, A))
    return [l // a for l, a in zip(L, A)]


def aggregate_of(L, A):
    """[V] the aggregate (lexicographic coarse site) of every lexicographic site"""
    return lex(coords(L) // np.array(A), coarse_lattice(L, A))


def members(L, A):
    """[aggregates][sites of an aggregate] lexicographic sites, ascending inside an aggregate"""
    agg = aggregate_of(L, A)
    return np.argsort(agg, kind="stable").reshape(int(agg.max()) + 1, -1)


def face_mask(L, A, mu):
    """[V] True where the +mu neighbour of a site lies outside its aggregate (a wrap-around into the same aggregate counts as
    leaving it)"""
    return coords(L)[:, mu] % A[mu] == A[mu] - 1


def _by_aggregate(x, mem):
    """[..][V][nd] -> [..][aggregate][site][chirality][nd / 2]"""
    nd = x.shape[-1]
    return x[..., mem, :].reshape(x.shape[:-2] + mem.shape + (2, nd // 2))


def restrict(P, phi, L, A):
    """phi_c[a][h N + j] = sum over the sites x of a and the dofs d of chirality h of conj(P_j(x, d)) phi(x, d);
    phi [V][nd] -> [Vc][2N], or [w][V][nd] -> [w][Vc][2N]"""
    mem = members(L, A)
    Pa, fa = _by_aggregate(np.asarray(P), mem), _by_aggregate(np.asarray(phi), mem)
    many = fa.ndim == 5
    if not many:
        fa = fa[None]
    pr, pi, fr, fi = Pa.real, Pa.imag, fa.real, fa.imag
    e = lambda p, f: np.einsum("jashd,washd->wahj", p, f, optimize=True)
    out = (e(pr, fr) + e(pi, fi)) + 1j * (e(pr, fi) - e(pi, fr))
    out = out.reshape(out.shape[0], out.shape[1], -1)
    return out if many else out[0]


def restrict_bound(P, phi, L, A):
    """the largest value any partial sum of restrict(P, phi) can reach in any order: max over results of sum |P| |phi| with
    |z| = |re| + |im|"""
    mem = members(L, A)
    Pa, fa = _by_aggregate(np.asarray(P), mem), _by_aggregate(np.asarray(phi), mem)
    if fa.ndim == 4:
        fa = fa[None]
    ab = lambda z: np.abs(z.real) + np.abs(z.imag)
    return float(np.einsum("jashd,washd->wahj", ab(Pa), ab(fa), optimize=True).max())


def interpolate(P, phic, L, A, phi0=None):
    """phi(x, d) = [phi0(x, d) +] sum_j P_j(x, d) phi_c[a(x)][h(d) N + j]; phic [Vc][2N] -> [V][nd] or [w][Vc][2N] -> [w][V][nd]"""
    P = np.asarray(P); phic = np.asarray(phic)
    N, V, nd = P.shape
    many = phic.ndim == 3
    pc = phic if many else phic[None]
    agg = aggregate_of(L, A)
    c = pc[:, agg].reshape(pc.shape[0], V, 2, N)                       # [w][x][h][j]
    Ph = P.reshape(N, V, 2, nd // 2)
    e = lambda p, q: np.einsum("jxhd,wxhj->wxhd", p, q, optimize=True)
    out = (e(Ph.real, c.real) - e(Ph.imag, c.imag)) + 1j * (e(Ph.real, c.imag) + e(Ph.imag, c.real))
    out = out.reshape(pc.shape[0], V, nd)
    if phi0 is not None:
        out = out + np.asarray(phi0)
    return out if many else out[0]


def restrict5_compact(P, W5, L, A):
    """The Galerkin construction's five fields per column, face-compacted: the self part W5[c][0] counts on all sites, the forward
    part W5[c][1 + mu] only on the sites whose +mu neighbour leaves the aggregate.  W5 [c][5][V][nd] -> [c][5][Vc][2N]"""
    W5 = np.asarray(W5)
    out = [restrict(P, W5[:, 0], L, A)]
    for mu in range(4):
        out.append(restrict(P, W5[:, 1 + mu] * face_mask(L, A, mu)[None, :, None], L, A))
    return np.stack(out, axis=1)


def compact_sites(lex_of_site, L, A, agg0, naggs):
    """the sites (lexicographic) a face-compacted column holds, in its order: part 0 all sites of the aggregates
    [agg0, agg0 + naggs) in the level's own site order, part 1 + mu those of them on the +mu face, in the same order"""
    S = int(np.prod(A))
    sl = np.asarray(lex_of_site)[agg0 * S:(agg0 + naggs) * S]
    return [sl] + [sl[face_mask(L, A, mu)[sl]] for mu in range(4)]


def tile_offset(row, col, nt):
    """where entry (row, col) of a coupling matrix lies in the 8x8-tile layout of CoarseOp, in complex numbers: tiles row-major
    with nt tiles per row, entries row-major inside a tile"""
    return ((row >> 3) * nt + (col >> 3)) * 64 + (row & 7) * 8 + (col & 7)


def matrices_with_columns(res, csite_of_lex, nt, msize, col_base, sentinel):
    """The next level's coupling matrices [Vc][5][msize][2] (filled with `sentinel`) after the columns col_base .. of the five
    parts were stored: res [c][5][Vc][2N] complex, coarse sites lexicographic; csite_of_lex: the coarse level's own site order"""
    ncols, _, Vc, n2 = res.shape
    M = np.full((Vc, 5, msize, 2), float(sentinel))
    rows = np.arange(n2)
    for c in range(ncols):
        o = tile_offset(rows, col_base + c, nt)
        assert o.max() < msize
        for p in range(5):
            M[csite_of_lex[:, None], p, o[None, :], 0] = res[c, p].real
            M[csite_of_lex[:, None], p, o[None, :], 1] = res[c, p].imag
    return M


# ---- the layouts a vector and the interpolation operator have on the device (the raw read-back of set_column) ------------------
def fine_device_vector(x, site_of_lex, CH):
    """[V][24] reals in lexicographic order -> the chunked layout [24 / CH][V][CH] in the level's site order (CH = 4 reals per
    chunk in fp32, 2 in fp64)"""
    V = x.shape[0]
    dev = np.empty_like(x)
    dev[np.asarray(site_of_lex)] = x
    return dev.reshape(V, 24 // CH, CH).transpose(1, 0, 2).reshape(-1)


def fine_device_P(P, site_of_lex, S, CH):
    """[N][V][24] -> P as Interpolation<T> stores it: [aggregate][vector][24 / CH][site of the aggregate][CH]; aggregate a is the
    site range [a S, (a + 1) S) of the level's order"""
    N, V, _ = P.shape
    dev = np.empty_like(P)
    dev[:, np.asarray(site_of_lex)] = P
    return dev.reshape(N, V // S, S, 24 // CH, CH).transpose(1, 0, 3, 2, 4).reshape(-1)


# ---- Gram-Schmidt per aggregate and chirality ----------------------------------------------------------------------------------
def gram_schmidt(tv, L, A, passes=1, dtype=np.float64, order=None):
    """Modified Gram-Schmidt of the columns tv [N][V][nd] (complex) on every aggregate and chirality, `passes` sweeps, in the
    kernels' order: column k is projected on the finished columns 0 .. k-1 one after the other, then normalised.
    dtype = float32: vectors, coefficients and the scale are rounded to fp32 after every step as the kernels do, products and
    sums run in fp64 (the kernels sum fp32 products in double).  order: a permutation of the elements of an (aggregate,
    chirality) block in which the sums run."""
    tv = np.asarray(tv)
    N, V, nd = tv.shape
    mem = members(L, A)
    ct = np.complex64 if dtype == np.float32 else np.complex128
    X = _by_aggregate(tv, mem).transpose(1, 3, 0, 2, 4).reshape(mem.shape[0], 2, N, -1).astype(ct)    # [a][h][N][elements]
    if order is not None:
        X = X[..., order]
    rnd = (lambda z: z.astype(np.complex64)) if dtype == np.float32 else (lambda z: z)
    for _ in range(passes):
        for k in range(N):
            v = X[:, :, k].astype(np.complex128)
            for k2 in range(k):
                u = X[:, :, k2].astype(np.complex128)
                al = rnd(np.sum(rnd(np.conj(u) * v).astype(np.complex128), axis=-1, keepdims=True)).astype(np.complex128)
                v = rnd(v - al * u).astype(np.complex128)
            nr = np.sum(rnd(np.abs(v) ** 2 + 0j).real.astype(np.float64), axis=-1, keepdims=True)
            sc = 1.0 / np.sqrt(nr)
            if dtype == np.float32:
                sc = sc.astype(np.float32).astype(np.float64)
            X[:, :, k] = rnd(v * sc)
    if order is not None:
        inv = np.empty_like(order); inv[order] = np.arange(order.size)
        X = X[..., inv]
    S = mem.shape[1]
    out = np.empty((N, V, nd), dtype=ct)
    out[:, mem.reshape(-1)] = X.reshape(mem.shape[0], 2, N, S, nd // 2).transpose(2, 0, 3, 1, 4).reshape(N, V, nd)
    return out


def blocks(P, L, A):
    """[N][V][nd] -> [aggregate][chirality][elements][N]: the matrix of every (aggregate, chirality) block, columns = vectors"""
    mem = members(L, A)
    N = P.shape[0]
    return _by_aggregate(np.asarray(P), mem).transpose(1, 3, 2, 4, 0).reshape(mem.shape[0], 2, -1, N)


def orthonormality(P, L, A):
    """max |P^H P - 1| over the entries of every (aggregate, chirality) block: [aggregate][2]"""
    B = blocks(np.asarray(P, dtype=np.complex128), L, A)
    G = np.einsum("ahek,ahel->ahkl", np.conj(B), B, optimize=True)
    return np.abs(G - np.eye(G.shape[-1])).max(axis=(2, 3))


def coefficients(P, tv, L, A):
    """R = P^H tv of every block ([aggregate][2][N][N]): tv = P R, upper triangular with a positive real diagonal for a
    Gram-Schmidt result"""
    Bp, Bt = blocks(np.asarray(P, dtype=np.complex128), L, A), blocks(np.asarray(tv, dtype=np.complex128), L, A)
    return np.einsum("ahek,ahel->ahkl", np.conj(Bp), Bt, optimize=True)
