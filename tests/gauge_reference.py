"""numpy restatement of the gauge sector of the molecular dynamics (include/ddamg_hip.h, "Gauge sector"): plaquette and rectangle
sums, the gauge action and its force, the exponential of an algebra element, the reunitarisation and a leapfrog trajectory.
Independent of the library: path products over np.roll-shifted fields, written from the definitions.  test_gauge_reference.py pins
it; the GPU tests compare the kernels with it.

Links U are the caller's, [V][4][9][2] reals, lexicographic T, Z, Y, X with X fastest, WITHOUT the anti-periodic sign: every closed
loop crosses the time boundary an even number of times, so the sign drops out of every number here.
  S = beta sum_x [ c0 sum_{mu<nu} (1 - 1/3 Re tr P_mu_nu(x)) + c1 sum_{mu!=nu} (1 - 1/3 Re tr R_mu_nu(x)) ],   c0 = 1 - 8 c1
  G_mu(x) = TA(M_mu(x)),  M_mu(x) = -(beta/3) U_mu(x) [c0 sum(6 plaquette staples) + c1 sum(18 rectangle staples)]
  dU/dt = P U,  dP/dt = G,  H = 1/2 |P|^2 + S   (the convention of the issue; see the header for why it conserves H)"""
import numpy as np
from force_reference import dag, ta, at, as_reals, as_matrices, exp_algebra

WILSON, SYMANZIK, IWASAKI = 0.0, -1.0 / 12.0, -0.331


def links(L, U):
    """[T, Z, Y, X, 4, 3, 3] complex from the caller's [V][4][9][2] reals"""
    u = np.asarray(U, dtype=np.float64).reshape(*L, 4, 3, 3, 2)
    return u[..., 0] + 1j * u[..., 1]


def path(W, steps, start=(0, 0, 0, 0)):
    """the ordered product of links along a path, as a field over the site x the path is attached to: the path starts at
    x + start and takes the steps in turn; a step +1 + mu walks forward along mu (factor U_mu(y)), -1 - mu backward
    (factor U_mu(y - mu)^dagger)"""
    pos = list(start)
    out = None
    for s in steps:
        mu = s - 1 if s > 0 else -s - 1
        if s < 0:
            pos[mu] -= 1
        m = W[..., mu, :, :]
        for d in range(4):
            m = at(m, d, pos[d])
        if s < 0:
            m = dag(m)
        else:
            pos[mu] += 1
        out = m if out is None else out @ m
    return out


def fwd(mu):
    return mu + 1


def bwd(mu):
    return -mu - 1


def retr(m):
    return float(np.trace(m, axis1=-2, axis2=-1).real.sum())


def loops(L, U):
    """(sum_x sum_{mu<nu} Re tr P_mu_nu(x), sum_x sum_{mu!=nu} Re tr R_mu_nu(x)); R_mu_nu: two steps along mu, one along nu"""
    W = links(L, U)
    plaq = rect = 0.0
    for mu in range(4):
        for nu in range(4):
            if nu == mu:
                continue
            if mu < nu:
                plaq += retr(path(W, [fwd(mu), fwd(nu), bwd(mu), bwd(nu)]))
            rect += retr(path(W, [fwd(mu), fwd(mu), fwd(nu), bwd(mu), bwd(mu), bwd(nu)]))
    return plaq, rect


def action_from_sums(V, beta, c1, plaq, rect):
    c0 = 1.0 - 8.0 * c1
    return beta * (c0 * (6.0 * V - plaq / 3.0) + c1 * (12.0 * V - rect / 3.0))


def action(L, U, beta, c1):
    return action_from_sums(int(np.prod(L)), beta, c1, *loops(L, U))


def staples(L, U):
    """(sum of the 6 plaquette staples, sum of the 18 rectangle staples) of every link, [T, Z, Y, X, 4, 3, 3] each: a staple is
    the rest of a closed loop that starts with the link U_mu(x), a path from x + mu back to x"""
    W = links(L, U)
    SP = np.zeros(W.shape, dtype=np.complex128)
    SR = np.zeros(W.shape, dtype=np.complex128)
    for mu in range(4):
        e = [0, 0, 0, 0]
        e[mu] = 1
        f, b = fwd(mu), bwd(mu)
        for nu in range(4):
            if nu == mu:
                continue
            u, d = fwd(nu), bwd(nu)
            for s in (u, d):       # above and below
                r = -s
                SP[..., mu, :, :] += path(W, [s, b, r], e)
                SR[..., mu, :, :] += path(W, [s, s, b, r, r], e)      # the nu-long rectangle
                SR[..., mu, :, :] += path(W, [f, s, b, b, r], e)      # the mu-long one, the link first
                SR[..., mu, :, :] += path(W, [s, b, b, r, f], e)      # the mu-long one, the link second
    return SP, SR


def force(L, U, beta, c1, parts="both"):
    """G = TA(M) as [V][4][9][2] reals; parts: "both", "plaquette" (G with c0 = 1, c1 = 0) or "rectangle" (c0 = 0, c1 = 1)"""
    W = links(L, U)
    SP, SR = staples(L, U)
    c0, cr = {"both": (1.0 - 8.0 * c1, c1), "plaquette": (1.0, 0.0), "rectangle": (0.0, 1.0)}[parts]
    return as_reals(ta(-(beta / 3.0) * (W @ (c0 * SP + cr * SR))))


def update_links(U, P, eps):
    """exp(eps P) U for every link; U, P: [V][4][9][2] reals"""
    w = exp_algebra(as_matrices(P), eps) @ as_matrices(U)
    return np.stack([w.real, w.imag], axis=-1).reshape(-1, 4, 9, 2)


def unitarity_deviation(U):
    """max over all links of max |U U^dagger - 1|"""
    u = as_matrices(U)
    return float(np.abs(u @ dag(u) - np.eye(3)).max())


def reunitarize(U):
    """row 0 normalised, row 1 orthogonalised against row 0 and normalised, row 2 = conj(row 0 x row 1)"""
    u = as_matrices(U).copy()
    r0 = u[..., 0, :] / np.linalg.norm(u[..., 0, :], axis=-1, keepdims=True)
    r1 = u[..., 1, :] - np.sum(np.conj(r0) * u[..., 1, :], axis=-1, keepdims=True) * r0
    r1 = r1 / np.linalg.norm(r1, axis=-1, keepdims=True)
    r2 = np.conj(np.cross(r0, r1))
    w = np.stack([r0, r1, r2], axis=-2)
    return np.stack([w.real, w.imag], axis=-1).reshape(-1, 4, 9, 2)


def kinetic(P):
    """1/2 sum |P_ij|^2 = -1/2 sum tr P^2"""
    return 0.5 * float(np.sum(np.asarray(P, dtype=np.float64) ** 2))


def leapfrog(L, U, P, beta, c1, tau, n):
    """n leapfrog steps of length tau / n: half a momentum step, then link and momentum steps in turn, half a momentum step at
    the end.  Returns (U, P) at the end"""
    dt = tau / n
    U = np.array(U, dtype=np.float64); P = np.array(P, dtype=np.float64)
    P = P + 0.5 * dt * force(L, U, beta, c1)
    for k in range(n):
        U = update_links(U, P, dt)
        P = P + (dt if k < n - 1 else 0.5 * dt) * force(L, U, beta, c1)
    return U, P


def hamiltonian(L, U, P, beta, c1):
    return kinetic(P) + action(L, U, beta, c1)
