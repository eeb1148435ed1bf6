"""Plain fp64 numpy restatement of krylov.h's restarted flexible GMRES, and the operator of the native GMRES tests.

Same control flow as Gmres<T>::solve: classical Gram-Schmidt with a separate norm, Givens rotations, restart from the true
residual, right preconditioning that keeps Z_j, the breakdown exit on |H(j+1,j)| <= tol/10, the zero right-hand side.
tests/test_gmres_reference.py pins it against numpy.linalg; tests/test_gpu_gmres_driver.py compares the device solver with it.

Two variants exist only to measure how far a correct implementation may differ from it: modified Gram-Schmidt (gs="mgs"),
and fp32=True, which imitates fp32 vectors with fp64 inner products.  The two other Arnoldi forms of krylov.h (form=) are
restated as well: they are the same algorithm in exact arithmetic but not in floating point (their norm comes out of a
difference), so each device form is compared with its own restatement.
"""
import numpy as np

A_UP = 0.4 - 0.3j     # coefficient of z_{k+1}
B_DOWN = -0.2 + 0.5j  # coefficient of z_{k-1}


def diagonal(n):
    k = np.arange(n)
    return 3.0 + ((7 * k) % 11) / 11.0 + 1j * (((5 * k) % 13) / 13.0 - 0.5)


def apply_op(z, diag_only=False):
    out = diagonal(len(z)) * z
    if not diag_only:
        out = out + A_UP * np.roll(z, -1) + B_DOWN * np.roll(z, 1)
    return out


def dense_op(n, diag_only=False):
    return np.stack([apply_op(e, diag_only) for e in np.eye(n, dtype=complex)], axis=1)


class VariableJacobi:
    """z = v / d * (1 + 0.1 * (call mod 3)): a different preconditioner at every call"""
    def __init__(self, n, post=None):
        self.d, self.calls, self.post = diagonal(n), 0, post

    def __call__(self, v):
        z = v / self.d * (1.0 + 0.1 * (self.calls % 3))
        self.calls += 1
        return self.post(z) if self.post else z


def round_fp32(v):
    return v.astype(np.complex64).astype(np.complex128)


def round_scalar_fp32(c):
    return complex(np.complex64(c))


def permuted_dot(n, seed):
    """<a, b> as a plain fp64 sum by a tree (numpy's pairwise sum) over a permuted order: what legitimately differs between two
    implementations of one reduction, and the shape of the device's two-stage sums"""
    p = np.random.default_rng(seed).permutation(n)
    return lambda a, b: complex(np.sum(np.conj(a[p]) * b[p]))


def accurate_dot(a, b):
    """<a, b> with the products and their sum in extended precision, rounded once: the reference's own inner product.  (np.vdot
    sums 3092 products serially in fp64; its error, a few 1e-15 of the sum, is amplified by the norm-from-a-difference forms
    until it decides whether a cycle ends in the negative-norm restart.  The device's tree sums are ten times closer to this.)"""
    return complex(np.sum(np.conj(a.astype(np.clongdouble)) * b.astype(np.clongdouble)))


def gmres(b, tol, restart=10, num_restart=8, prec=None, x0=None, gs="cgs", form="classical", fp32=False, diag_only=False, trace=None,
          dot=accurate_dot):
    """Returns dict(iter, history, x, V, gamma_jp1, norm_r0); V: the basis vectors of the last cycle as columns.

    form: how the new vector's norm is found, as krylov.h's three Arnoldi forms find it.  "classical": the norm of the projected
    vector.  "single": sqrt(<w,w> - sum |h_i|^2) from the same reduction as the h_i (-1 for a negative difference: the cycle ends
    with the columns completed so far).  "pipelined": that, with V_k and A V_k both obtained by the same combination of earlier
    vectors (Gmres::arnoldi_pipelined).  All three are the same algorithm in exact arithmetic.
    fp32: every vector is rounded to fp32 after each vector operation, and so is every scalar that the kernels of blas.hip
    round to the vectors' type: the coefficients of an update and the reciprocal of a norm (inner products stay fp64).
    dot: the inner product (accurate_dot; np.vdot and permuted_dot: plain fp64 sums in one order or another).
    trace: a list that receives (cycle, j, Z_0..Z_j as columns, r0 of the cycle, x at the start of the cycle) per step."""
    rnd = round_fp32 if fp32 else (lambda v: v)
    rs = round_scalar_fp32 if fp32 else (lambda c: c)
    A = lambda v: rnd(apply_op(v, diag_only))
    scale_inv = lambda v, s: rnd(v * rs(1.0 / s)) if abs(s) > 1e-15 else v

    def project(w, h, basis):
        for i in range(len(h)):
            w = rnd(w - rs(h[i]) * basis[i])
        return w

    def norm_from_dots(ww, h):
        d = ww - sum(abs(t) ** 2 for t in h)
        return -1.0 if d < 0 else float(np.sqrt(d))

    n, m = len(b), restart
    x = np.zeros(n, complex) if x0 is None else np.array(x0, complex)
    it, finish, gamma_jp1, norm_r0, history = 0, False, 1.0, 1.0, []
    V = []
    for ol in range(num_restart):
        if finish:
            break
        fresh = ol == 0 and x0 is None
        r = b.copy() if fresh else rnd(b - A(x))
        gamma0 = float(np.sqrt(dot(r, r).real))
        if ol == 0:
            norm_r0 = gamma0
        if not gamma0 > 0:
            if fresh:
                x[:] = 0
            gamma_jp1 = 0.0
            break
        V, Z = [rnd(r * rs(1.0 / gamma0))], []
        H = np.zeros((m + 2, m + 1), complex)
        gamma = np.zeros(m + 2, complex); c = np.zeros(m + 2, complex); s = np.zeros(m + 2, complex)
        gamma[0] = gamma0
        if form == "pipelined":      # P[k] = A V[k-1] in the basis built so far; P[0] = V[0]
            P = [V[0]]
            d0 = norm_from_dots(dot(V[0], V[0]).real, [])
            P.append(A(P[0]))
            V[0] = scale_inv(V[0], d0); P[1] = scale_inv(P[1], d0)
        j = -1
        for il in range(m):
            j = il; it += 1
            if form == "pipelined":
                k = j + 1
                V.append(P[k])
                h = [dot(V[i], V[k]) for i in range(k)]
                hn = norm_from_dots(dot(V[k], V[k]).real, h)
                P.append(A(P[k]))
                V[k] = scale_inv(project(V[k], h, V), hn)
                P[k + 1] = scale_inv(project(P[k + 1], h, P[1:]), hn)
                Z.append(V[j])
            else:
                Z.append(rnd(prec(V[j])) if prec else V[j])
                w = A(Z[j])
                ww = dot(w, w).real
                if gs == "cgs":
                    h = [dot(V[i], w) for i in range(j + 1)]
                    w = project(w, h, V)
                else:
                    h = []
                    for i in range(j + 1):
                        h.append(dot(V[i], w))
                        w = rnd(w - rs(h[i]) * V[i])
                hn = float(np.sqrt(dot(w, w).real)) if form == "classical" else norm_from_dots(ww, h)
                V.append(scale_inv(w, hn))
            if hn < 0:               # the reference restarts then
                j -= 1; it -= 1
                V.pop()
                break
            H[:j + 1, j] = h; H[j + 1, j] = hn
            if trace is not None:
                trace.append((ol, j, np.stack(Z, axis=1), r, x.copy()))
            if abs(H[j + 1, j]) > tol / 10:
                for i in range(j):
                    beta = -s[i] * H[i, j] + c[i] * H[i + 1, j]
                    H[i, j] = np.conj(c[i]) * H[i, j] + np.conj(s[i]) * H[i + 1, j]
                    H[i + 1, j] = beta
                beta = np.sqrt(abs(H[j, j]) ** 2 + abs(H[j + 1, j]) ** 2)
                s[j] = H[j + 1, j] / beta; c[j] = H[j, j] / beta
                gamma[j + 1] = -s[j] * gamma[j]; gamma[j] = np.conj(c[j]) * gamma[j]
                H[j, j] = beta; H[j + 1, j] = 0
                gamma_jp1 = abs(gamma[j + 1])
                history.append(gamma_jp1 / norm_r0)
                if gamma_jp1 / norm_r0 < tol or gamma_jp1 / norm_r0 > 1e5:
                    finish = True
                    break
            else:
                finish = True
                break
        y = np.zeros(j + 1, complex)
        for i in range(j, -1, -1):
            y[i] = (gamma[i] - H[i, i + 1:j + 1] @ y[i + 1:]) / H[i, i]
        if fresh and j >= 0:
            x[:] = 0
        for i in range(j + 1):
            x = rnd(x + rs(y[i]) * Z[i])
    return dict(iter=it, history=np.array(history), x=x, V=np.stack(V, axis=1) if V else np.zeros((n, 0), complex),
                gamma_jp1=gamma_jp1, norm_r0=norm_r0)


def right_hand_side(n, seed=11):
    """deterministic complex right-hand side with entries in (-0.5, 0.5), exactly representable in fp32"""
    from conftest import splitmix_uniform
    u = splitmix_uniform(2 * n, seed).astype(np.float32).astype(np.float64)
    return u[0::2] + 1j * u[1::2]
