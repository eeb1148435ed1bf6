"""tests/force_reference.py against finite differences of the oracle (no GPU needed).

S(eps) is formed by existing pieces only: the links exp(eps Omega) U go through orc.gauge_to_operator; the bilinear function is the
real part of <Y, orc.dirac_apply X>, the determinant numpy's slogdet of eo_reference.clover_blocks.  Its derivative along Omega is the
central difference extrapolated once, (4 d(h) - d(2h)) / 3, which converges at fourth order; it is compared with
sum tr(Omega G) of the reference force G.  The bar is not fixed in advance: for every direction it is ten times the spread of the
extrapolated difference between its two finest steps, h = 2^-7 and 2^-8, measured here -- ten times, because the spread estimates the
truncation error of the coarser of the two.

Measured spreads, relative to the derivative (synthetic field synth_gauge(L, 0.35, 5), m0 = -0.1, anti-periodic):
  single links, 4^4:        csw 1: 1.2e-11 .. 2.4e-8     csw 0: 8.5e-12 .. 2.5e-8
  single links, 4x6x8x10:   csw 1: 9.3e-10 .. 1.6e-8
  global directions, 4^4:   csw 1: 3.9e-10 .. 3.0e-7     csw 0: 5.2e-9 .. 1.4e-7     scaled clover term: 1.1e-7
  determinant, 4^4:         single links 7.6e-11 .. 8.6e-8, global directions 6.9e-7 and 4.2e-6
The reference lay between 0.001 and 0.14 of its bar, mostly at 0.007: a fifteenth of the spread, which is what fourth-order
convergence leaves at the finer step."""
import os, sys
import numpy as np
import pytest
from conftest import splitmix_uniform
from oracle import orc
import eo_reference as eo
import force_reference as fr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
M0 = -0.1
H = 2.0 ** -8
_fields = {}


def field(L):
    """(links, X, Y) of a lattice, made once"""
    key = tuple(L)
    if key not in _fields:
        import synth
        V = int(np.prod(L))
        U = synth.synth_gauge(list(L), 0.35, 5).reshape(V, 4, 9, 2)
        _fields[key] = (U, splitmix_uniform(V * 24, 9).reshape(V, 12, 2), splitmix_uniform(V * 24, 10).reshape(V, 12, 2))
    return _fields[key]


def lex(L, c):
    return ((c[0] * L[1] + c[1]) * L[2] + c[2]) * L[3] + c[3]


def single_link(L, site, mu, seed):
    omega = np.zeros((int(np.prod(L)), 4, 3, 3), dtype=np.complex128)
    omega[lex(L, site), mu] = fr.random_algebra(np.random.default_rng(seed), ())
    return omega


def global_direction(L, seed):
    return fr.random_algebra(np.random.default_rng(seed), (int(np.prod(L)), 4))


def bilinear(L, csw, scale=(1.0, 1.0)):
    U, X, Y = field(L)
    s = np.where(eo.parity(L) == 1, scale[1], scale[0])[:, None, None]

    def S(omega, eps):
        D, cl, _ = orc.gauge_to_operator(L, fr.perturbed(U, omega, eps), 1, M0, csw)
        if scale != (1.0, 1.0):
            cl = cl * s
        return float(np.sum(Y * orc.dirac_apply(L, D, cl, X, 64)))
    return S, fr.force_bilinear(L, U, 1, M0, csw, Y, X, scale)


def determinant(L, csw, par):
    U = field(L)[0]
    keep = eo.parity(L) == par

    blocks = lambda u: np.linalg.slogdet(eo.clover_blocks(orc.gauge_to_operator(L, u, 1, M0, csw)[1])[keep])[1]
    at_zero = blocks(U)

    def S(omega, eps):
        # less the constant S(0), block by block: the blocks a link does not reach cancel exactly instead of adding their rounding
        return float(np.sum(blocks(fr.perturbed(U, omega, eps)) - at_zero))
    return S, fr.force_logdet(L, U, 1, M0, csw, par)


def check(S, G, omega, what):
    """the reference's derivative along omega against the extrapolated difference, within ten times its spread between h and 2h"""
    fine = fr.richardson(lambda e: S(omega, e), H)
    coarse = fr.richardson(lambda e: S(omega, e), 2 * H)
    spread = abs(fine - coarse)
    mine = fr.pairing(omega, G)
    print(f"{what}: derivative {fine:+.12e} reference {mine:+.12e} spread {spread:.2e} (relative {spread / abs(fine):.2e}) "
          f"difference {abs(mine - fine):.2e}")
    assert abs(fine) > 1e-6, what                         # the direction tests something
    assert abs(mine - fine) <= 10 * spread, what


def interior(L):
    return [1, L[1] // 2, L[2] // 2 - 1, L[3] - 2]


@pytest.mark.parametrize("csw", [0.0, 1.0])
def test_single_links_at_an_interior_site(csw):
    L = [4, 4, 4, 4]
    S, G = bilinear(L, csw)
    for mu in range(4):
        check(S, G, single_link(L, interior(L), mu, 100 + mu), f"csw {csw} interior link {mu}")


def test_single_links_on_a_lattice_of_four_extents():
    L = [4, 6, 8, 10]
    S, G = bilinear(L, 1.0)
    for mu in range(4):
        check(S, G, single_link(L, interior(L), mu, 200 + mu), f"4x6x8x10 interior link {mu}")


@pytest.mark.parametrize("csw", [0.0, 1.0])
def test_single_links_at_the_boundaries(csw):
    """the link in direction d at coordinate 0 and at L - 1 of direction d: the wrap-around, and on the last time slice the sign"""
    L = [4, 4, 4, 4]
    S, G = bilinear(L, csw)
    for d in range(4):
        for c in (0, L[d] - 1):
            site = interior(L); site[d] = c
            check(S, G, single_link(L, site, d, 300 + 2 * d + (c > 0)), f"csw {csw} link {d} at coordinate {c}")
    site = [L[0] - 1, 0, L[2] - 1, 0]
    for mu in (1, 3):                                      # the other links of the last time slice, in a corner
        check(S, G, single_link(L, site, mu, 320 + mu), f"csw {csw} link {mu} in a corner of the last time slice")


@pytest.mark.parametrize("csw", [0.0, 1.0])
def test_global_directions(csw):
    L = [4, 4, 4, 4]
    S, G = bilinear(L, csw)
    for k in range(4):
        check(S, G, global_direction(L, 400 + k), f"csw {csw} global direction {k}")


def test_scaled_clover_term():
    L = [4, 4, 4, 4]
    S, G = bilinear(L, 1.0, scale=(1.1, 0.9))
    check(S, G, global_direction(L, 500), "scale (1.1, 0.9) global direction")


@pytest.mark.parametrize("par", [0, 1])
def test_determinant(par):
    L = [4, 4, 4, 4]
    S, G = determinant(L, 1.0, par)
    for mu in range(4):
        check(S, G, single_link(L, interior(L), mu, 600 + mu), f"parity {par} interior link {mu}")
    check(S, G, single_link(L, [L[0] - 1, 0, 3, 0], 0, 610), f"parity {par} time link of the last slice")
    check(S, G, global_direction(L, 620 + par), f"parity {par} global direction")
    # every link's force is traceless anti-Hermitian, and without a clover term C is a constant
    g = fr.as_matrices(G)
    assert np.abs(g + fr.dag(g)).max() < 1e-15 and np.abs(np.trace(g, axis1=-2, axis2=-1)).max() < 1e-15
    assert not fr.force_logdet(L, field(L)[0], 1, M0, 0.0, par).any()
