"""The gauge sector of the molecular dynamics on the device (-m gpu): ddamg_hip_gauge_loops_device, _gauge_force_device,
_links_update_device, _links_reunitarize_device, _momentum_update_device and _momentum_kinetic_device against the numpy restatement
tests/gauge_reference.py (which test_gauge_reference.py pins), against finite differences of the action the library itself returns,
and in a pure-gauge leapfrog trajectory that runs through the six entry points only.

Lattices (test_gpu_dagger.LATTICES, those of test_gpu_force.py): 4^4, where the 8 x 8 plane tile is larger than the lattice and the
two-deep neighbourhood wraps onto itself; 4x6x8x10, four extents and tile tails; 8^4, exactly one tile; 4x4x12x12, two tiles in a
direction, the second a tail.  Actions: c1 = 0 (the one-site neighbourhood), -1/12 and -0.331.  Links exp(0.35 algebra), beta 5.6.

Bars.  Against the reference: 1e-13 of the field's norm or of the sum, the project's fp64 bar (an entry is a sum of at most 24 products
of five matrices).  plaquette_sum / (6 V) against the plaquette ddamg_hip_set_gauge_device returns: 1e-13 (the sum runs over the six
planes, so it is 6 V times that average; 18 V for unit links).  Finite differences: (4 d(h) - d(2h)) / 3 at h = 2^-8 within ten times
its spread between h and 2h.  Link update: 1e-13 against the eigh exponential; after ONE update of unitary links with |eps P| <= 1,
|U U^dagger - 1| <= 1e-14.  Reunitarisation: 4 eps and 8 eps.  Trajectory: both ratios of Delta H in [3.5, 4.5]; Delta H(10) within
1e-6 of the reference's; reversibility 1e-12.  The reference itself gives 3.931 / 3.983 (c1 0), 3.949 / 3.987 (-1/12) and
4.000 / 4.000 (-0.331) on these fields.
Measured on the MI355X: sums against the reference 0 to 2.9e-16, force 1.8e-16 to 2.4e-16 on all four lattices; |tr G| one to two
eps of max |G|; finite differences: global direction, spread 9.8e-5 / 1.7e-4 / 3.9e-4 and difference 6.5e-6 / 1.2e-5 / 2.6e-5 for the
three actions, a corner T-link 3.9e-9 .. 1.2e-8 and 1.9e-10 .. 9.8e-10; link update 4.4e-16 to 5.3e-16 (norm <= 1) and 1.7e-15 to
2.0e-15 (norm 10), |U U^dagger - 1| 8.9e-16 to 1.1e-15 after one update; reunitarisation: deviation as numpy's to seven digits, then
6.7e-16 (3 eps), |det - 1| 7.8e-16, fixed point 4.4e-16; Delta H ratios 3.931 / 3.983, 3.949 / 3.987, 4.000 / 4.000, Delta H(10)
against the reference 0 to 1.1e-13, reversibility 1.9e-15 to 5.8e-15.  Every case takes 0.3 s at most.
Times at 32^4: docs/design/04_kernels.md, "Gauge force"."""
import numpy as np
import pytest
from conftest import relerr
from ddalphaamg_amd import api
import ddalphaamg_amd as dd
import force_reference as fr
import gauge_reference as gr
from test_gpu_device_interface import Hip, params
from test_gpu_dagger import LATTICES

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
LATS = ["4^4", "4x6x8x10", "8^4", "4x4x12x12"]
C1 = [gr.WILSON, gr.SYMANZIK, gr.IWASAKI]
BETA = 5.6
H = 2.0 ** -8
_fields, _reference = {}, {}


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.free_all()


def unit_links(V):
    one = np.zeros((V, 4, 9, 2)); one[:, :, [0, 4, 8], 0] = 1.0
    return one


def links(lat):
    """the links of a lattice, exp(0.35 algebra), made once"""
    if lat not in _fields:
        V = int(np.prod(LATTICES[lat][0]))
        _fields[lat] = fr.perturbed(unit_links(V), fr.random_algebra(np.random.default_rng(5), (V, 4)), 0.35)
    return _fields[lat]


def reference(lat):
    """(plaquette sum, rectangle sum, G of the plaquette part, G of the rectangle part) of the lattice's links, computed once"""
    if lat not in _reference:
        L = LATTICES[lat][0]
        _reference[lat] = gr.loops(L, links(lat)) + (gr.force(L, links(lat), BETA, 0.0, "plaquette"), gr.force(L, links(lat), BETA, 0.0, "rectangle"))
    return _reference[lat]


def reference_force(lat, c1):
    _, _, gp, gq = reference(lat)
    return (1.0 - 8.0 * c1) * gp + c1 * gq


def context(lat, grid=(1, 1, 1, 1)):
    L, B = LATTICES[lat]
    return dd.Context(params(L, [B] * 4, -0.1, 1.0, grid=grid))


def nbytes(lat):
    return int(np.prod(LATTICES[lat][0])) * 72 * 8


def shape(lat):
    return (int(np.prod(LATTICES[lat][0])), 4, 9, 2)


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lat", LATS)
def test_loops_and_force_against_the_reference(lat, hip):
    V = shape(lat)[0]
    U = links(lat)
    plaq, rect, _, _ = reference(lat)
    ctx = context(lat)
    dU = hip.upload(U); out = hip.alloc(nbytes(lat))
    p, r = ctx.gauge_loops_device(dU)
    p1, none = ctx.gauge_loops_device(dU, rectangles=False)
    print(f"{lat}: plaquette sum {p:.12e} (reference: {abs(p - plaq) / abs(plaq):.1e}), rectangle sum {r:.12e} ({abs(r - rect) / abs(rect):.1e}), "
          f"without rectangles {abs(p1 - plaq) / abs(plaq):.1e}")
    assert none is None
    assert abs(p - plaq) <= 1e-13 * abs(plaq) and abs(p1 - plaq) <= 1e-13 * abs(plaq) and abs(r - rect) <= 1e-13 * abs(rect)
    assert ctx.gauge_loops_device(dU) == (p, r)                     # deterministic
    for c1 in C1:
        assert ctx.gauge_force_device(out, dU, BETA, c1) == out
        err = relerr(hip.download(out, shape(lat)), reference_force(lat, c1))
        print(f"{lat} c1 {c1:+.4f}: force against the reference {err:.1e}")
        assert err < 1e-13
    assert np.array_equal(hip.download(dU, U.shape), U)               # the links are read only
    # the plaquette of the operator's path: the same links, with the anti-periodic sign, which drops out
    average = ctx.set_gauge_device(dU, anti_pbc=True)
    print(f"{lat}: plaquette_sum / (6 V) {p / (6 * V):.15f}, set_gauge_device {average:.15f}")
    assert 0.0 <= average <= 3.0 and abs(p / (6 * V) - average) <= 1e-13 * average
    # unit links: 18 V and 36 V, and no force
    dI = hip.upload(unit_links(V))
    assert ctx.gauge_loops_device(dI) == (18.0 * V, 36.0 * V)
    assert not hip.download(ctx.gauge_force_device(out, dI, BETA, gr.IWASAKI), shape(lat)).any()
    ctx.close()


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lat", ["4^4", "4x4x12x12"])
def test_force_properties(lat, hip):
    U = links(lat)
    ctx = context(lat)
    dU = hip.upload(U); out = hip.alloc(nbytes(lat)); acc = hip.alloc(nbytes(lat))
    G = {}
    for c1 in C1:
        ctx.gauge_force_device(out, dU, BETA, c1)
        G[c1] = hip.download(out, shape(lat))
        g = fr.as_matrices(G[c1])
        trace = np.abs(np.trace(g, axis1=-2, axis2=-1)).max()
        print(f"{lat} c1 {c1:+.4f}: max |G| {np.abs(g).max():.3e}, |G + G^dagger| {np.abs(g + fr.dag(g)).max():.1e}, |tr G| {trace:.1e}")
        assert np.array_equal(g, -fr.dag(g))                          # exactly anti-Hermitian
        assert trace <= 4 * EPS * np.abs(g).max()
        ctx.gauge_force_device(acc, dU, BETA, c1)
        assert np.array_equal(hip.download(acc, shape(lat)), G[c1])   # two calls, the same bits
        assert np.array_equal(hip.download(dU, U.shape), U)
    # coeff and accumulate: G is linear in c1, G(c1) = G(0) + c1 / c1' (G(c1') - G(0)); and against c0 G_plaq + c1 G_rect of the reference
    ratio = gr.IWASAKI / gr.SYMANZIK
    ctx.gauge_force_device(acc, dU, BETA, gr.WILSON, coeff=1.0 - ratio)
    ctx.gauge_force_device(acc, dU, BETA, gr.SYMANZIK, coeff=ratio, accumulate=True)
    combined = hip.download(acc, shape(lat))
    print(f"{lat}: (1 - r) G(0) + r G(-1/12) against G(-0.331) {relerr(combined, G[gr.IWASAKI]):.1e}, against the reference "
          f"{relerr(combined, reference_force(lat, gr.IWASAKI)):.1e}")
    assert relerr(combined, G[gr.IWASAKI]) < 1e-13 and relerr(combined, reference_force(lat, gr.IWASAKI)) < 1e-13
    ctx.gauge_force_device(acc, dU, BETA, gr.SYMANZIK, coeff=-2.5)
    assert relerr(hip.download(acc, shape(lat)), -2.5 * G[gr.SYMANZIK]) < 1e-15
    ctx.close()


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c1", C1)
def test_force_against_finite_differences_of_the_librarys_own_action(c1, hip):
    lat = "4^4"
    L = LATTICES[lat][0]; V = 256
    U = links(lat)
    ctx = context(lat)
    dU = hip.upload(U); out = hip.alloc(nbytes(lat))
    G = hip.download(ctx.gauge_force_device(out, dU, BETA, c1), shape(lat))

    def S(omega, e):
        d = hip.upload(fr.perturbed(U, omega, e))
        return gr.action_from_sums(V, BETA, c1, *ctx.gauge_loops_device(d))
    single = np.zeros((V, 4, 3, 3), dtype=np.complex128)
    single[((3 * L[1] + 0) * L[2] + 3) * L[3] + 0, 0] = fr.random_algebra(np.random.default_rng(31), ())     # a T-link of the last slice, in a corner
    for what, omega in (("global direction", fr.random_algebra(np.random.default_rng(400), (V, 4))), ("corner T-link", single)):
        fine, coarse = fr.richardson(lambda e: S(omega, e), H), fr.richardson(lambda e: S(omega, e), 2 * H)
        spread, mine = abs(fine - coarse), fr.pairing(omega, G)
        print(f"c1 {c1:+.4f} {what}: derivative {fine:+.12e} force {mine:+.12e} spread {spread:.2e} difference {abs(mine - fine):.2e}")
        assert abs(fine) > 1e-6 and abs(mine - fine) <= 10 * spread
    ctx.close()


# 4 ------------------------------------------------------------------------------------------------------------------------
def update_arguments(n, rng):
    """n arguments eps P of the exponential, [n][3][3], in turn: Frobenius norm 1e-9, 1e-3, 1 and 10 of a random algebra element, zero,
    and the degenerate v diag(ia, ia, -2ia) v^dagger of norm 1 and 10, the first of them diagonal"""
    a = fr.random_algebra(rng, (n,))
    v = fr.exp_algebra(fr.random_algebra(rng, (n,)), 1.0)
    deg = v @ np.diag([1j, 1j, -2j]) @ fr.dag(v)
    deg[5] = np.diag([1j, 1j, -2j])
    norms = np.array([1e-9, 1e-3, 1.0, 10.0, 0.0, 1.0, 10.0])[np.arange(n) % 7]
    a = np.where((np.arange(n) % 7 >= 5)[:, None, None], deg, a)
    return a * (norms / np.linalg.norm(a, axis=(-2, -1)))[:, None, None]


def deviation(x):
    """max |U U^dagger - 1| of a list of links [n][9][2]"""
    u = x.reshape(-1, 3, 3, 2)[..., 0] + 1j * x.reshape(-1, 3, 3, 2)[..., 1]
    return float(np.abs(u @ fr.dag(u) - np.eye(3)).max())


def test_link_update_against_the_reference_exponential(hip):
    lat = "4x6x8x10"
    V = shape(lat)[0]
    U = gr.reunitarize(links(lat))      # unitary to 4 eps; exp_algebra leaves 16 eps
    ctx = context(lat)
    for eps in (1.0, -0.37):
        arg = update_arguments(4 * V, np.random.default_rng(41))
        P = fr.as_reals((arg / eps).reshape(V, 4, 3, 3))
        dU = hip.upload(U); dP = hip.upload(P)
        assert ctx.links_update_device(dU, dP, eps) == dU
        got, want = hip.download(dU, U.shape), gr.update_links(U, P, eps)
        assert np.array_equal(hip.download(dP, P.shape), P)
        for k, name in enumerate(("norm 1e-9", "norm 1e-3", "norm 1", "norm 10", "zero", "degenerate norm 1", "degenerate norm 10")):
            sel = np.arange(4 * V) % 7 == k
            g, w = got.reshape(-1, 9, 2)[sel], want.reshape(-1, 9, 2)[sel]
            print(f"eps {eps:+.2f} {name}: relative error {relerr(g, w):.1e}, |U U^dagger - 1| {deviation(g):.1e}")
            assert relerr(g, w) < 1e-13
            if k in (0, 1, 2, 4, 5):     # |eps P| <= 1 and unitary links: one update keeps them unitary
                assert deviation(g) <= 1e-14
        assert np.array_equal(got.reshape(-1, 9, 2)[np.arange(4 * V) % 7 == 4], U.reshape(-1, 9, 2)[np.arange(4 * V) % 7 == 4])     # exp(0) = 1
    ctx.close()


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_reunitarisation(hip):
    """4^4, 1024 links in four workgroups.  The bars of 4 eps and 8 eps sit at the rounding of the projection AND of the measurement:
    an entry of U U^dagger is a sum of three products of numbers that each carry half an eps.  The numpy projection of this very
    field comes back at 3.5 eps and 4.0 eps (8^4 and 4x6x8x10 with the same seed: 4.002 and 4.0004 eps, the more links the further
    into the tail), so the lattice is the one of the reference's own prototype."""
    lat = "4^4"
    U = links(lat)
    off = U + 1e-6 * np.random.default_rng(3).standard_normal(U.shape)
    ctx = context(lat)
    dU = hip.upload(off)
    dev = ctx.links_reunitarize_device(dU)
    back = hip.download(dU, U.shape)
    det = np.abs(np.linalg.det(fr.as_matrices(back)) - 1.0).max()
    print(f"deviation {dev:.6e} (numpy {gr.unitarity_deviation(off):.6e}), then |U U^dagger - 1| {gr.unitarity_deviation(back):.1e}, |det - 1| {det:.1e}, "
          f"against the reference projection {np.abs(back - gr.reunitarize(off)).max():.1e}")
    assert abs(dev - gr.unitarity_deviation(off)) <= 0.1 * gr.unitarity_deviation(off)
    assert gr.unitarity_deviation(back) <= 4 * EPS and det <= 8 * EPS
    assert np.abs(back - gr.reunitarize(off)).max() <= 16 * EPS      # an entry of at most one behind some ten roundings, ordered differently
    # a projected field is a fixed point, and its deviation is rounding
    again = ctx.links_reunitarize_device(dU)
    moved = np.abs(hip.download(dU, U.shape) - back).max()
    print(f"fixed point: moved {moved:.1e}, deviation {again:.1e}")
    assert moved <= 4 * EPS and again <= 4 * EPS
    ctx.close()


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_momentum_update_and_kinetic_energy(hip):
    lat = "4x6x8x10"
    V = shape(lat)[0]
    rng = np.random.default_rng(17)
    P = fr.as_reals(fr.random_algebra(rng, (V, 4))); F = fr.as_reals(fr.random_algebra(rng, (V, 4)))
    ctx = context(lat)
    dP = hip.upload(P); dF = hip.upload(F)
    kin = ctx.momentum_kinetic_device(dP)
    assert abs(kin - gr.kinetic(P)) <= 1e-13 * kin and ctx.momentum_kinetic_device(dP) == kin
    assert ctx.momentum_update_device(dP, dF, -0.3) == dP
    got = hip.download(dP, P.shape)
    print(f"kinetic energy {kin:.12e} (numpy: {abs(kin - gr.kinetic(P)) / kin:.1e}), P + eps F {np.abs(got - (P - 0.3 * F)).max():.1e}")
    assert np.abs(got - (P - 0.3 * F)).max() <= 2 * EPS * (np.abs(P).max() + np.abs(F).max())      # two roundings or one fused
    assert np.array_equal(hip.download(dF, F.shape), F)
    ctx.close()


# 7 ------------------------------------------------------------------------------------------------------------------------
def leapfrog(ctx, dU, dP, dF, c1, tau, n):
    """n leapfrog steps through the entry points, as gauge_reference.leapfrog takes them"""
    dt = tau / n
    ctx.momentum_update_device(dP, ctx.gauge_force_device(dF, dU, BETA, c1), 0.5 * dt)
    for k in range(n):
        ctx.links_update_device(dU, dP, dt)
        ctx.momentum_update_device(dP, ctx.gauge_force_device(dF, dU, BETA, c1), dt if k < n - 1 else 0.5 * dt)


def hamiltonian(ctx, dU, dP, V, c1):
    return ctx.momentum_kinetic_device(dP) + gr.action_from_sums(V, BETA, c1, *ctx.gauge_loops_device(dU))


@pytest.mark.parametrize("c1", C1)
def test_a_pure_gauge_leapfrog_trajectory(c1, hip):
    lat = "4^4"
    L = LATTICES[lat][0]; V = 256
    U = links(lat)
    P = fr.as_reals(fr.random_algebra(np.random.default_rng(21), (V, 4)))
    ctx = context(lat)
    dF = hip.alloc(nbytes(lat))
    dH = {}
    for n in (10, 20, 40):
        dU = hip.upload(U); dP = hip.upload(P)
        H0 = hamiltonian(ctx, dU, dP, V, c1)
        leapfrog(ctx, dU, dP, dF, c1, 0.5, n)
        dH[n] = hamiltonian(ctx, dU, dP, V, c1) - H0
    Ur, Pr = gr.leapfrog(L, U, P, BETA, c1, 0.5, 10)
    want = gr.hamiltonian(L, Ur, Pr, BETA, c1) - gr.hamiltonian(L, U, P, BETA, c1)
    print(f"c1 {c1:+.4f}: H0 {H0:.6e}, Delta H {dH[10]:+.6e} {dH[20]:+.6e} {dH[40]:+.6e}, ratios {dH[10] / dH[20]:.3f} {dH[20] / dH[40]:.3f}, "
          f"Delta H(10) against the reference {abs(dH[10] - want) / abs(want):.1e}")
    assert 3.5 <= dH[10] / dH[20] <= 4.5 and 3.5 <= dH[20] / dH[40] <= 4.5
    assert abs(dH[10] - want) <= 1e-6 * abs(want)
    # backwards: the n = 40 trajectory with -P returns to the start
    end = hip.download(dP, P.shape)
    dM = hip.upload(-end)
    leapfrog(ctx, dU, dM, dF, c1, 0.5, 40)
    back_u, back_p = np.abs(hip.download(dU, U.shape) - U).max(), np.abs(hip.download(dM, P.shape) + P).max()
    print(f"c1 {c1:+.4f}: reversibility U {back_u:.1e} P {back_p:.1e}")
    assert back_u <= 1e-12 and back_p <= 1e-12
    ctx.close()


# 8 ------------------------------------------------------------------------------------------------------------------------
def refused(call, *words):
    with pytest.raises(api.DDAMGError) as e:
        call()
    assert all(w in str(e.value) for w in words), str(e.value)


def test_refusals(hip):
    lat = "8^4"
    V = shape(lat)[0]
    U = links(lat)
    dU = hip.upload(U); dP = hip.upload(np.ones(shape(lat))); dF = hip.upload(2.0 * np.ones(shape(lat)))
    host = np.zeros(V * 72)
    ctx = context(lat)
    calls = {"gauge_loops": lambda a: ctx.gauge_loops_device(a), "gauge_force (output)": lambda a: ctx.gauge_force_device(a, dU, BETA, gr.SYMANZIK),
             "gauge_force (links)": lambda a: ctx.gauge_force_device(dF, a, BETA, gr.SYMANZIK), "links_update (links)": lambda a: ctx.links_update_device(a, dP, 0.1),
             "links_update (momenta)": lambda a: ctx.links_update_device(dU, a, 0.1), "links_reunitarize": lambda a: ctx.links_reunitarize_device(a),
             "momentum_update (momenta)": lambda a: ctx.momentum_update_device(a, dF, 0.1), "momentum_update (force)": lambda a: ctx.momentum_update_device(dP, a, 0.1),
             "momentum_kinetic": lambda a: ctx.momentum_kinetic_device(a)}
    small = hip.alloc(nbytes(lat))
    for name, call in calls.items():
        refused(lambda: call(int(host.ctypes.data)), "not a pointer into device memory")
        refused(lambda: call(small + 64), "smaller than the array")
        refused(lambda: call(0), "null")
    refused(lambda: ctx.gauge_force_device(dU, dU, BETA, 0.0), "overlap")
    big = hip.alloc(2 * nbytes(lat))
    refused(lambda: ctx.links_update_device(big, big + 8, 0.1), "overlap")                 # the momenta one real into the links
    refused(lambda: ctx.momentum_update_device(big + nbytes(lat) - 8, big, 0.1), "overlap")   # the momenta's first real in the force's last
    refused(lambda: ctx.gauge_force_device(dF, dU, float("nan"), 0.0), "beta", "not finite")
    refused(lambda: ctx.links_update_device(dU, dP, float("inf")), "eps", "not finite")
    # nothing was written
    assert np.array_equal(hip.download(dU, U.shape), U) and (hip.download(dP, shape(lat)) == 1.0).all() and (hip.download(dF, shape(lat)) == 2.0).all()
    assert not host.any()
    ctx.close()
    # a process grid (the T direction exchanged with itself): all six are refused
    ctx = context(lat, grid=(-1, 1, 1, 1))
    for call in (lambda: ctx.gauge_loops_device(dU), lambda: ctx.gauge_force_device(dF, dU, BETA, 0.0), lambda: ctx.links_update_device(dU, dP, 0.1),
                 lambda: ctx.links_reunitarize_device(dU), lambda: ctx.momentum_update_device(dP, dF, 0.1), lambda: ctx.momentum_kinetic_device(dP)):
        refused(call, "process grid", "not built yet")
    assert np.array_equal(hip.download(dU, U.shape), U) and (hip.download(dP, shape(lat)) == 1.0).all()
    ctx.close()
