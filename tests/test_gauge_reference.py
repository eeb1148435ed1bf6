"""tests/gauge_reference.py pinned (no GPU needed): the yardstick of the gauge sector's GPU tests.

  unit links          the sums are 18 V and 36 V (6 plaquettes and 12 rectangles per site, trace 3 each) and the force is zero
  invariance          both sums do not change under a random gauge transformation, nor under the sign flip of the T-links of the
                      last time slice (every loop crosses the boundary an even number of times): relative 1e-13
  finite differences  sum tr(Omega G) against the central difference of the action extrapolated once, (4 d(h) - d(2h)) / 3, h = 2^-8,
                      within ten times its spread between h and 2h, as test_force_reference.py argues
  exponential         exp_algebra (eigh) against a Taylor series summed after scaling by 2^-k and squared k times in extended
                      precision (np.longdouble), for small, degenerate (diag(ia, ia, -2ia)) and norm-10 arguments

Measured (4^4, beta 5.6, links exp(0.35 algebra)): global directions, spread 8.9e-5 .. 3.9e-4, difference 6.0e-6 .. 2.6e-5; single
links, spread 2.2e-9 .. 1.1e-7, difference 9.4e-11 .. 8.1e-9, a fifteenth of the spread throughout; the exponential within 1.7e-15 of
the series (norm 10; 7e-16 below); leapfrog, c1 = -1/12: Delta H(10) / Delta H(20) = 3.949, reversibility 1.7e-14."""
import numpy as np
import pytest
import force_reference as fr
import gauge_reference as gr

BETA = 5.6
C1 = [gr.WILSON, gr.SYMANZIK, gr.IWASAKI]
H = 2.0 ** -8
_fields = {}


def field(L, seed=5):
    key = (tuple(L), seed)
    if key not in _fields:
        V = int(np.prod(L))
        one = np.zeros((V, 4, 9, 2)); one[:, :, [0, 4, 8], 0] = 1.0
        _fields[key] = fr.perturbed(one, fr.random_algebra(np.random.default_rng(seed), (V, 4)), 0.35)
    return _fields[key]


def lex(L, c):
    return ((c[0] * L[1] + c[1]) * L[2] + c[2]) * L[3] + c[3]


def test_unit_links():
    L = [4, 6, 4, 6]; V = int(np.prod(L))
    one = np.zeros((V, 4, 9, 2)); one[:, :, [0, 4, 8], 0] = 1.0
    assert gr.loops(L, one) == (18.0 * V, 36.0 * V)
    for c1 in C1:
        assert gr.action(L, one, BETA, c1) == 0.0
        assert not gr.force(L, one, BETA, c1).any()


def test_the_sums_are_gauge_invariant_and_blind_to_the_antiperiodic_sign():
    L = [4, 6, 4, 8]; V = int(np.prod(L))
    U = field(L)
    plaq, rect = gr.loops(L, U)
    assert abs(plaq) < 18.0 * V and abs(rect) < 36.0 * V
    g = fr.exp_algebra(fr.random_algebra(np.random.default_rng(7), tuple(L)), 1.3)          # g(x), [T, Z, Y, X, 3, 3]
    W = gr.links(L, U)
    Wg = np.stack([g @ W[..., mu, :, :] @ fr.dag(fr.at(g, mu, 1)) for mu in range(4)], axis=-3)
    pg, rg = gr.loops(L, fr.as_reals(Wg.reshape(V, 4, 3, 3)))
    flipped = U.reshape(*L, 4, 9, 2).copy()
    flipped[L[0] - 1, :, :, :, 0] *= -1.0
    pf, rf = gr.loops(L, flipped.reshape(V, 4, 9, 2))
    print(f"sums {plaq:.6e} {rect:.6e}; gauge transformed {abs(pg - plaq) / abs(plaq):.1e} {abs(rg - rect) / abs(rect):.1e}; "
          f"sign flipped {abs(pf - plaq) / abs(plaq):.1e} {abs(rf - rect) / abs(rect):.1e}")
    for a, b in ((pg, plaq), (rg, rect), (pf, plaq), (rf, rect)):
        assert abs(a - b) <= 1e-13 * abs(b)
    # the force transforms covariantly: G'(x) = g(x) G(x) g(x)^dagger
    G = fr.as_matrices(gr.force(L, U, BETA, gr.IWASAKI)).reshape(*L, 4, 3, 3)
    Gg = fr.as_matrices(gr.force(L, fr.as_reals(Wg.reshape(V, 4, 3, 3)), BETA, gr.IWASAKI)).reshape(*L, 4, 3, 3)
    assert np.abs(Gg - g[..., None, :, :] @ G @ fr.dag(g)[..., None, :, :]).max() <= 1e-13 * np.abs(G).max()


def check(L, U, c1, G, omega, what):
    S = lambda e: gr.action(L, fr.perturbed(U, omega, e), BETA, c1)
    fine, coarse = fr.richardson(S, H), fr.richardson(S, 2 * H)
    spread = abs(fine - coarse)
    mine = fr.pairing(omega, G)
    print(f"{what}: derivative {fine:+.12e} reference {mine:+.12e} spread {spread:.2e} difference {abs(mine - fine):.2e}")
    assert abs(fine) > 1e-6, what
    assert abs(mine - fine) <= 10 * spread, what


@pytest.mark.parametrize("c1", C1)
def test_force_against_finite_differences_of_the_action(c1):
    L = [4, 4, 4, 4]; V = 256
    U = field(L)
    G = gr.force(L, U, BETA, c1)
    g = fr.as_matrices(G)
    assert np.abs(g + fr.dag(g)).max() < 1e-15 and np.abs(np.trace(g, axis1=-2, axis2=-1)).max() < 1e-14
    for k in range(2):
        check(L, U, c1, G, fr.random_algebra(np.random.default_rng(400 + k), (V, 4)), f"c1 {c1:+.4f} global direction {k}")
    for mu in range(4):      # single links: an interior one, and one on the boundary of its own direction (the wrap-around)
        for site in ([1, 2, 1, 2], [3 if mu == 0 else 0, 3 if mu == 1 else 1, 3 if mu == 2 else 0, 3 if mu == 3 else 2]):
            omega = np.zeros((V, 4, 3, 3), dtype=np.complex128)
            omega[lex(L, site), mu] = fr.random_algebra(np.random.default_rng(100 + mu), ())
            check(L, U, c1, G, omega, f"c1 {c1:+.4f} link {mu} at {site}")


def test_force_on_a_lattice_of_four_extents():
    L = [4, 6, 8, 10]; V = int(np.prod(L))
    U = field(L)
    G = gr.force(L, U, BETA, gr.SYMANZIK)
    for mu in range(4):
        omega = np.zeros((V, 4, 3, 3), dtype=np.complex128)
        omega[lex(L, [1, 3, 3, 8]), mu] = fr.random_algebra(np.random.default_rng(200 + mu), ())
        check(L, U, gr.SYMANZIK, G, omega, f"4x6x8x10 link {mu}")
    # the parts add up
    parts = (1.0 - 8.0 * gr.SYMANZIK) * gr.force(L, U, BETA, 0.0, "plaquette") + gr.SYMANZIK * gr.force(L, U, BETA, 0.0, "rectangle")
    assert np.abs(parts - G).max() <= 1e-13 * np.abs(G).max()


def series_exp(a, squarings=6, terms=30):
    """exp of one 3x3 matrix: Taylor series of a / 2^squarings in extended precision, squared back"""
    re, im = np.asarray(a.real, dtype=np.longdouble) / 2.0 ** squarings, np.asarray(a.imag, dtype=np.longdouble) / 2.0 ** squarings

    def mul(x, y):
        return x[0] @ y[0] - x[1] @ y[1], x[0] @ y[1] + x[1] @ y[0]
    one = (np.eye(3, dtype=np.longdouble), np.zeros((3, 3), dtype=np.longdouble))
    out = one
    for k in range(terms, 0, -1):      # Horner: 1 + a/1 (1 + a/2 (1 + ...))
        t = mul((re, im), out)
        out = (one[0] + t[0] / k, t[1] / k)
    for _ in range(squarings):
        out = mul(out, out)
    return np.asarray(out[0], dtype=np.float64) + 1j * np.asarray(out[1], dtype=np.float64)


def exponential_arguments():
    """(name, 3x3 traceless anti-Hermitian matrix): small, degenerate and of Frobenius norm 10"""
    rng = np.random.default_rng(11)
    a = fr.random_algebra(rng, ())
    v = fr.exp_algebra(fr.random_algebra(rng, ()), 1.0)
    deg = v @ np.diag([0.7j, 0.7j, -1.4j]) @ fr.dag(v)
    return [("small 1e-9", a * (1e-9 / np.linalg.norm(a))), ("small 1e-3", a * (1e-3 / np.linalg.norm(a))), ("zero", a * 0.0),
            ("degenerate diagonal", np.diag([0.7j, 0.7j, -1.4j])), ("degenerate rotated", deg), ("norm 1", a / np.linalg.norm(a)),
            ("norm 10", a * (10.0 / np.linalg.norm(a))), ("norm 10 degenerate", deg * (10.0 / np.linalg.norm(deg)))]


@pytest.mark.parametrize("name,a", exponential_arguments(), ids=[n for n, _ in exponential_arguments()])
def test_exponential(name, a):
    e = fr.exp_algebra(a, 1.0)
    ref = series_exp(a)
    err = np.abs(e - ref).max()
    print(f"{name}: |exp - series| {err:.2e}, |e e^dagger - 1| {np.abs(e @ fr.dag(e) - np.eye(3)).max():.2e}")
    assert err <= 1e-14      # both are unitary matrices of entries at most one: 45 eps
    assert abs(np.linalg.det(e) - 1.0) <= 1e-14


def test_reunitarisation_and_kinetic_energy():
    L = [4, 4, 4, 4]
    U = field(L)
    rng = np.random.default_rng(3)
    off = U + 1e-6 * rng.standard_normal(U.shape)
    dev = gr.unitarity_deviation(off)
    assert 1e-6 < dev < 1e-5
    back = gr.reunitarize(off)
    assert gr.unitarity_deviation(back) <= 4 * np.finfo(float).eps
    assert np.abs(np.linalg.det(fr.as_matrices(back)) - 1.0).max() <= 8 * np.finfo(float).eps
    assert np.abs(back - off).max() < 1e-5
    again = gr.reunitarize(back)
    assert np.abs(again - back).max() <= 4 * np.finfo(float).eps
    P = fr.as_reals(fr.random_algebra(rng, (256, 4)))
    p = fr.as_matrices(P)
    assert abs(gr.kinetic(P) + 0.5 * np.einsum("vmab,vmba->", p, p).real) <= 1e-13 * gr.kinetic(P)


def test_leapfrog_conserves_the_hamiltonian_at_second_order_and_is_reversible():
    L = [4, 4, 4, 4]
    U = field(L)
    P = fr.as_reals(fr.random_algebra(np.random.default_rng(21), (256, 4)))
    c1 = gr.SYMANZIK
    H0 = gr.hamiltonian(L, U, P, BETA, c1)
    dH = {}
    for n in (10, 20):
        U1, P1 = gr.leapfrog(L, U, P, BETA, c1, 0.5, n)
        dH[n] = gr.hamiltonian(L, U1, P1, BETA, c1) - H0
    print(f"H0 {H0:.6e} dH(10) {dH[10]:+.4e} dH(20) {dH[20]:+.4e} ratio {dH[10] / dH[20]:.3f}")
    assert 3.5 <= dH[10] / dH[20] <= 4.5
    Ub, Pb = gr.leapfrog(L, U1, -P1, BETA, c1, 0.5, 20)
    print(f"reversibility: U {np.abs(Ub - U).max():.1e} P {np.abs(Pb + P).max():.1e}")
    assert np.abs(Ub - U).max() <= 1e-12 and np.abs(Pb + P).max() <= 1e-12
