"""numpy statement of multi-shift conjugate gradients (B. Jegerlehner, hep-lat/9612014) on A_s = Q + sigma_s for a Hermitian positive
definite Q given as a callable, with the library's conventions: the smallest shift is the base system and runs plain CG; shift s
is converged at the first iteration k with |zeta_s^k| ||r_k|| <= tol_s ||b|| and is frozen from then on (x_s, p_s and zeta_s are
left alone); a zeta_s that leaves the normal range of fp64 freezes its shift without that step.  Dense helpers for the even-odd
system are built on eo_reference.schur_matrix."""
import sys
import numpy as np
import eo_reference as eo

TINY = sys.float_info.min


def multishift_cg(op, b, shifts, tols, max_iterations=2000):
    """op(v) = Q v on complex vectors.  Returns (x [nshift][n], iterations per shift, alpha history, beta history, the residual norms
    ||r_k|| / ||b||, the Lanczos matrix of the base system)"""
    shifts = np.asarray(shifts, dtype=np.float64)
    n = len(shifts)
    tols = np.full(n, float(tols)) if np.isscalar(tols) else np.asarray(tols, dtype=np.float64)
    base = int(np.argmin(shifts))
    ds = shifts - shifts[base]
    x = np.zeros((n, len(b)), dtype=np.complex128)
    p = np.tile(b, (n, 1))
    r = b.copy()
    zeta, zeta_old = np.ones(n), np.ones(n)
    alpha_old, beta_old = 1.0, 0.0
    rr = np.vdot(r, r).real
    nb = np.sqrt(rr)
    its = np.zeros(n, dtype=int)
    alphas, betas, hist = [], [], []
    if not nb > 0:
        return x, its, alphas, betas, hist, np.zeros((0, 0))
    active = np.array([not nb <= t * nb for t in tols])
    k = 0
    while active.any() and k < max_iterations:
        q = p[base]
        Ap = op(q) + shifts[base] * q
        pAp = np.vdot(q, Ap).real
        if not pAp > 0:
            break
        alpha = rr / pAp
        r = r - alpha * Ap
        rr_new = np.vdot(r, r).real
        beta = rr_new / rr
        k += 1
        for s in np.flatnonzero(active):
            zn = zeta[s] * zeta_old[s] * alpha_old / (alpha * beta_old * (zeta_old[s] - zeta[s]) + zeta_old[s] * alpha_old * (1.0 + ds[s] * alpha))
            its[s] = k
            if not (np.isfinite(zn) and abs(zn) >= TINY):
                active[s] = False
                continue
            ratio = zn / zeta[s]
            x[s] += (alpha * ratio) * p[s]
            p[s] = zn * r + (beta * ratio * ratio) * p[s]
            zeta_old[s], zeta[s] = zeta[s], zn
            if abs(zn) * np.sqrt(rr_new) <= tols[s] * nb:
                active[s] = False
        if not active[base]:
            # the base system's direction goes on for the others: p = r + beta p, with zeta = 1
            p[base] = r + beta * p[base]
        alphas.append(alpha); betas.append(beta); hist.append(np.sqrt(rr_new) / nb)
        alpha_old, beta_old, rr = alpha, beta, rr_new
    return x, its, alphas, betas, hist, lanczos_matrix(alphas, betas)


def lanczos_matrix(alphas, betas):
    """the tridiagonal matrix whose eigenvalues are the Ritz values of the base system's operator (shift included)"""
    k = len(alphas)
    T = np.zeros((k, k))
    for j in range(k):
        T[j, j] = 1.0 / alphas[j] + (betas[j - 1] / alphas[j - 1] if j else 0.0)
        if j + 1 < k:
            T[j, j + 1] = T[j + 1, j] = np.sqrt(betas[j]) / alphas[j]
    return T


def ritz_extremes(T, base_shift):
    ev = np.linalg.eigvalsh(T)
    return ev[0] - base_shift, ev[-1] - base_shift


def sparse_normal_operator(A, L):
    """(v -> S^dagger S v on the even unknowns without forming S, the indices of the even unknowns): the blocks of the sparse full
    matrix A by parity and a sparse LU of the block-diagonal A_oo, for lattices whose dense Schur complement is too large"""
    from scipy.sparse.linalg import splu
    even = np.flatnonzero(np.repeat(eo.parity(L), 12) == 0)
    odd = np.flatnonzero(np.repeat(eo.parity(L), 12) == 1)
    A = A.tocsr()
    Aee, Aeo, Aoe = A[even][:, even].tocsr(), A[even][:, odd].tocsr(), A[odd][:, even].tocsr()
    lu = splu(A[odd][:, odd].tocsc())
    S = lambda v: Aee @ v - Aeo @ lu.solve(Aoe @ v)
    SH = lambda v: Aee.conj().T @ v - Aoe.conj().T @ lu.solve(Aeo.conj().T @ v, trans="H")
    return (lambda v: SH(S(v))), even


def dense_normal_operator(A, L):
    """(Q = S^dagger S of the Schur complement S of the sparse full matrix A, the indices of the even unknowns)"""
    S, even = eo.schur_matrix(A, L)
    return S.conj().T @ S, even
