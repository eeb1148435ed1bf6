"""The fermion force on the device (-m gpu): ddamg_hip_force_bilinear_vec / _device and ddamg_hip_force_logdet against the numpy
restatement tests/force_reference.py (which test_force_reference.py pins against finite differences of the oracle), against finite
differences of the operator the library itself applies, and against finite differences of the even-odd preconditioned two-flavour
action through the library's own solves and log det.

Lattices (test_gpu_dagger.LATTICES): 4^4, where the 8 x 8 plane tile is larger than the lattice and the staged neighbourhood wraps onto
itself; 4x6x8x10, four different extents and tile tails of 6 and 10; 8^4, exactly one tile; 4x4x12x12, two tiles in a direction, the
second a tail, so that forward and backward neighbour tiles differ.

Bars.  Against the reference: 1e-13 of the field's norm, the project's fp64 bar (every entry is a sum of at most 50 products of five
numbers of order one).  Finite differences: the central difference extrapolated once, (4 d(h) - d(2h)) / 3 at h = 2^-8, within ten times
its spread between h and 2h, measured by the test (test_force_reference.py says why ten); with a solve in S, ten times the larger of
that spread and 1e-12 |S| / h, what a solve to 1e-12 leaves in the difference quotient.
Measured on the MI355X: against the reference 2.1e-16 to 2.5e-16 (bilinear) and 1.1e-15 to 1.2e-15 (determinant); the library's own
operator: derivative -19.87, spread 3.1e-6, difference 2.1e-7; the even-odd action: S = -4454, derivative -0.895, spread 9.1e-7,
1e-12 |S| / h = 1.1e-6, difference 6.1e-8.  Times: docs/design/04_kernels.md, "Fermion force"."""
import numpy as np
import pytest
from conftest import relerr, splitmix_uniform
from ddalphaamg_amd import api
import ddalphaamg_amd as dd
import eo_reference as eo
import force_reference as fr
from test_gpu_device_interface import Hip, params, synth_field
from test_gpu_dagger import LATTICES, FORMS, SWITCHES, M0, CSW, hierarchy, rhs

pytestmark = pytest.mark.gpu
G5 = np.array([-1.0] * 6 + [1.0] * 6)[None, :, None]
EPS = np.finfo(np.float64).eps
LATS = ["4^4", "4x6x8x10", "8^4", "4x4x12x12"]
# the link forms of the fp32 operator that a lattice can have (test_gpu_dagger.FORMS): the force must not depend on them
CASES = [(lat, form) for lat in LATS for form in (("pivot", "full") if LATTICES[lat][1] == 4 else ("table",))]
H = 2.0 ** -8
_fields, _reference = {}, {}


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.free_all()


def fields(lat):
    """(links, X, Y) of a lattice, made once"""
    if lat not in _fields:
        L = LATTICES[lat][0]
        V = int(np.prod(L))
        _fields[lat] = (synth_field(L, 5), splitmix_uniform(V * 24, 9).reshape(V, 12, 2), splitmix_uniform(V * 24, 10).reshape(V, 12, 2))
    return _fields[lat]


def reference(lat, csw, scale=(1.0, 1.0), m0=M0, par=None):
    """the reference force of the lattice's fields, computed once: bilinear (par None) or determinant"""
    key = (lat, csw, scale, m0, par)
    if key not in _reference:
        L = LATTICES[lat][0]
        U, X, Y = fields(lat)
        _reference[key] = fr.force_bilinear(L, U, 1, m0, csw, Y, X, scale) if par is None else fr.force_logdet(L, U, 1, m0, csw, par, scale)
    return _reference[key]


def context(lat, form, monkeypatch, csw=CSW, grid=(1, 1, 1, 1), device_links=None):
    """a one-level context on the lattice, the switches of the form set before it is created; the links from host memory, or from
    the device array `device_links`"""
    L, B = LATTICES[lat]
    env, reals = FORMS[form]
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    ctx = dd.Context(params(L, [B] * 4, M0, csw, grid=grid))
    if min(grid) < 0:
        ctx.comm_init_rccl(api.rccl_unique_id())
    if device_links is None:
        ctx.set_gauge(fields(lat)[0], anti_pbc=True)
    else:
        ctx.set_gauge_device(device_links, anti_pbc=True)
    assert ctx.link_reals() == reals
    return ctx


def nbytes(lat):
    return int(np.prod(LATTICES[lat][0])) * 72 * 8


def by_vec(ctx, hip, lat, y, x, coeff=1.0, accumulate=False, out=None):
    """the force through the _vec entry point, downloaded; the vectors are checked to be unchanged"""
    vy = ctx.vector(0, 64).upload(y); vx = ctx.vector(0, 64).upload(x)
    out = hip.alloc(nbytes(lat)) if out is None else out
    assert ctx.force_bilinear_vec(out, vy, vx, coeff, accumulate) == out
    assert np.array_equal(vy.download(), y) and np.array_equal(vx.download(), x)
    vy.free(); vx.free()
    return hip.download(out, (len(x), 4, 9, 2))


def by_device(ctx, hip, lat, y, x, coeff=1.0, accumulate=False, out=None):
    dy = hip.upload(y); dx = hip.upload(x)
    out = hip.alloc(nbytes(lat)) if out is None else out
    ctx.force_bilinear_device(out, dy, dx, coeff, accumulate)
    assert np.array_equal(hip.download(dy, y.shape), y) and np.array_equal(hip.download(dx, x.shape), x)
    return hip.download(out, (len(x), 4, 9, 2))


def logdet_force(ctx, hip, lat, par, coeff=1.0):
    out = hip.alloc(nbytes(lat))
    ctx.force_logdet(out, par, coeff)
    return hip.download(out, (int(np.prod(LATTICES[lat][0])), 4, 9, 2))


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("csw", [1.0, 0.0])
@pytest.mark.parametrize("lat,form", CASES, ids=[f"{a}-{b}" for a, b in CASES])
def test_bilinear_force_against_the_reference(lat, form, csw, monkeypatch, hip):
    _, X, Y = fields(lat)
    ctx = context(lat, form, monkeypatch, csw)
    ref = reference(lat, csw)
    got = by_vec(ctx, hip, lat, Y, X)
    err = relerr(got, ref)
    print(lat, form, "csw", csw, "norm", np.linalg.norm(ref), "relerr", err)
    assert err < 1e-13
    assert np.array_equal(by_device(ctx, hip, lat, Y, X), got)          # the same bits
    ctx.close()


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lat", LATS)
def test_the_force_is_in_the_algebra_and_nothing_else_is_written(lat, monkeypatch, hip):
    """links from device memory here; every matrix anti-Hermitian (exactly: it is unpacked from nine reals) and traceless to the
    rounding of the three-term sum; operator and links unchanged; two calls give the same bits"""
    U, X, Y = fields(lat)
    dU = hip.upload(U)
    ctx = context(lat, "pivot" if LATTICES[lat][1] == 4 else "table", monkeypatch, device_links=dU)
    D0, cl0 = ctx.get_operator()
    got = by_vec(ctx, hip, lat, Y, X)
    assert relerr(got, reference(lat, CSW)) < 1e-13
    g = fr.as_matrices(got)
    assert np.array_equal(g, -fr.dag(g))
    assert np.abs(np.trace(g, axis1=-2, axis2=-1)).max() <= 4 * EPS * np.abs(g).max()
    assert np.array_equal(by_vec(ctx, hip, lat, Y, X), got) and np.array_equal(by_device(ctx, hip, lat, Y, X), got)
    for par in (0, 1):
        ld = logdet_force(ctx, hip, lat, par)
        assert np.array_equal(logdet_force(ctx, hip, lat, par), ld)
        g = fr.as_matrices(ld)
        assert np.array_equal(g, -fr.dag(g)) and np.abs(np.trace(g, axis1=-2, axis2=-1)).max() <= 4 * EPS * np.abs(g).max()
    D1, cl1 = ctx.get_operator()
    assert np.array_equal(D0, D1) and np.array_equal(cl0, cl1) and np.array_equal(hip.download(dU, U.shape), U)
    ctx.close()


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_coeff_accumulate_and_linearity(monkeypatch, hip):
    lat = "4x6x8x10"
    L = LATTICES[lat][0]
    _, X, Y = fields(lat)
    X2 = splitmix_uniform(X.size, 11).reshape(X.shape)
    ctx = context(lat, "table", monkeypatch)
    f1 = by_vec(ctx, hip, lat, Y, X)
    f2 = by_vec(ctx, hip, lat, Y, X2)
    assert relerr(by_vec(ctx, hip, lat, Y, X, coeff=-2.0), -2.0 * f1) <= EPS          # coeff scales the result
    assert relerr(by_device(ctx, hip, lat, Y, X, coeff=0.7), 0.7 * f1) <= EPS
    # accumulate: what the array held plus coeff times the force, from both entry points and from the determinant's
    start = splitmix_uniform(f1.size, 12).reshape(f1.shape)
    out = hip.upload(start)
    assert relerr(by_vec(ctx, hip, lat, Y, X, coeff=0.7, accumulate=True, out=out), start + 0.7 * f1) <= 2 * EPS
    assert relerr(by_device(ctx, hip, lat, Y, X2, coeff=-1.5, accumulate=True, out=out), start + 0.7 * f1 - 1.5 * f2) <= 4 * EPS
    ld = logdet_force(ctx, hip, lat, 1)
    ctx.force_logdet(out, 1, -2.0, True)
    assert relerr(hip.download(out, f1.shape), start + 0.7 * f1 - 1.5 * f2 - 2.0 * ld) <= 6 * EPS
    # linear in X (complex-linear: a = 0.3 - 0.8 i), anti-linear in Y
    a = 0.3 - 0.8j
    Xc = X[..., 0] + 1j * X[..., 1]; X2c = X2[..., 0] + 1j * X2[..., 1]
    mix = a * Xc + X2c
    fa = by_vec(ctx, hip, lat, Y, np.stack([(a * Xc).real, (a * Xc).imag], axis=-1))
    fm = by_vec(ctx, hip, lat, Y, np.stack([mix.real, mix.imag], axis=-1))
    assert relerr(fm, fa + f2) < 1e-13
    assert relerr(by_vec(ctx, hip, lat, Y, 3.0 * X), 3.0 * f1) < 1e-13
    assert L == [4, 6, 8, 10]
    ctx.close()


# 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lat", ["4^4", "4x4x12x12"])
def test_exchanging_the_vectors(lat, monkeypatch, hip):
    """<Y, D X>* = <gamma5 X, D gamma5 Y> for every field: the force of (Y, X) is the force of (gamma5 X, gamma5 Y)"""
    _, X, Y = fields(lat)
    ctx = context(lat, "pivot" if LATTICES[lat][1] == 4 else "table", monkeypatch)
    a, b = by_vec(ctx, hip, lat, Y, X), by_vec(ctx, hip, lat, G5 * X, G5 * Y)
    print(lat, "relerr", relerr(b, a))
    assert relerr(b, a) < 1e-13 and not np.array_equal(by_vec(ctx, hip, lat, X, Y), a)
    ctx.close()


# 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lat", LATS)
def test_determinant_force_scale_and_mass(lat, monkeypatch, hip):
    _, X, Y = fields(lat)
    ctx = context(lat, "pivot" if LATTICES[lat][1] == 4 else "table", monkeypatch)
    plain = {}
    for par in (0, 1):
        plain[par] = logdet_force(ctx, hip, lat, par)
        err = relerr(plain[par], reference(lat, CSW, par=par))
        print(lat, "parity", par, "norm", np.linalg.norm(plain[par]), "relerr", err)
        assert err < 1e-13
    bilinear = by_vec(ctx, hip, lat, Y, X)
    # scale_clover: the factor cancels in log det up to a constant; the clover part of the bilinear force carries s(x)
    ctx.scale_clover(1.1, 0.9)
    for par in (0, 1):
        assert relerr(logdet_force(ctx, hip, lat, par), plain[par]) < 1e-13
    scaled = by_vec(ctx, hip, lat, Y, X)
    assert relerr(scaled, reference(lat, CSW, scale=(1.1, 0.9))) < 1e-13 and relerr(scaled, bilinear) > 1e-3
    ctx.scale_clover(1.0, 1.0)
    assert np.array_equal(by_vec(ctx, hip, lat, Y, X), bilinear)
    # shift_mass: <Y, D X> depends on the links through the hopping and the clover term, neither of which holds the mass: the same
    # bits; the determinant follows the new mass
    ctx.shift_mass(0.05)
    assert np.array_equal(by_vec(ctx, hip, lat, Y, X), bilinear)
    for par in (0, 1):
        shifted = logdet_force(ctx, hip, lat, par)
        assert relerr(shifted, reference(lat, CSW, m0=0.05, par=par)) < 1e-13 and relerr(shifted, plain[par]) > 1e-3
    ctx.close()


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_derivative_of_the_operator_the_library_applies(monkeypatch, hip):
    """no reference code: S(eps) = Re <Y, D X> through set_gauge_device on exp(eps Omega) U, dirac_apply in fp64 and vec_dot"""
    lat = "4^4"
    L = LATTICES[lat][0]
    U, X, Y = fields(lat)
    omega = fr.random_algebra(np.random.default_rng(31), (len(X), 4))
    ctx = context(lat, "table", monkeypatch, device_links=hip.upload(U))
    vy = ctx.vector(0, 64).upload(Y); vx = ctx.vector(0, 64).upload(X); vz = ctx.vector(0, 64)

    def S(eps):
        ctx.set_gauge_device(hip.upload(fr.perturbed(U, omega, eps)), anti_pbc=True)
        ctx.dirac_apply(vz, vx)
        return ctx.vec_dot(vy, vz)[0].real
    fine, coarse = fr.richardson(S, H), fr.richardson(S, 2 * H)
    ctx.set_gauge_device(hip.upload(U), anti_pbc=True)
    out = hip.alloc(nbytes(lat))
    ctx.force_bilinear_vec(out, vy, vx)
    mine = fr.pairing(omega, hip.download(out, (len(X), 4, 9, 2)))
    spread = abs(fine - coarse)
    print(f"derivative {fine:+.12e} force {mine:+.12e} spread {spread:.2e} difference {abs(mine - fine):.2e}")
    assert abs(fine) > 1.0 and abs(mine - fine) <= 10 * spread
    for v in (vy, vx, vz):
        v.free()
    assert L == [4] * 4
    ctx.close()


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_the_force_of_the_even_odd_action(hip):
    """S = phi_e^dagger (Dhat^dagger Dhat)^-1 phi_e - 2 log|det D_oo| through solve_schur_squared_device and clover_logdet on perturbed
    links, against force_bilinear(Y, X, -2) + force_logdet(1, -2) with X and Y formed as INTEGRATION.md ("Forces") says"""
    TOL = 1e-12
    ctx, L = hierarchy("4^4")
    V = int(np.prod(L)); n = V // 2
    U = synth_field(L, 2)
    odd = eo.parity(L) == 1
    phi = np.ascontiguousarray(rhs(L)[~odd])
    omega = fr.random_algebra(np.random.default_rng(32), (V, 4))
    dphi = hip.upload(phi)
    dxe, dxo, dye, dyo = (hip.alloc(phi.nbytes) for _ in range(4))

    def S(eps):
        ctx.set_gauge_device(hip.upload(fr.perturbed(U, omega, eps)), anti_pbc=True)
        ctx.solve_schur_squared_device(dxe, None, dphi, TOL)
        return float(np.sum(phi * hip.download(dxe, phi.shape))) - 2.0 * ctx.clover_logdet(1)[0]
    fine, coarse = fr.richardson(S, H), fr.richardson(S, 2 * H)
    ctx.set_gauge_device(hip.upload(U), anti_pbc=True)
    s0 = S(0.0)
    # Y: D^dagger Y = (phi_e, 0); X: D X = (y_e, 0), both with their odd parts
    ctx.solve_schur_device(dye, dyo, dphi, TOL, dagger=True)
    ctx.solve_schur_device(dxe, dxo, dye, TOL)
    X = np.empty((V, 12, 2)); Y = np.empty((V, 12, 2))
    X[~odd], X[odd] = hip.download(dxe, phi.shape), hip.download(dxo, phi.shape)
    Y[~odd], Y[odd] = hip.download(dye, phi.shape), hip.download(dyo, phi.shape)
    out = hip.alloc(V * 72 * 8)
    ctx.force_bilinear_device(out, hip.upload(Y), hip.upload(X), -2.0)
    ctx.force_logdet(out, 1, -2.0, accumulate=True)
    mine = fr.pairing(omega, hip.download(out, (V, 4, 9, 2)))
    spread, solve = abs(fine - coarse), TOL * abs(s0) / H
    print(f"S {s0:.12e} derivative {fine:+.12e} force {mine:+.12e} spread {spread:.2e} solve {solve:.2e} difference {abs(mine - fine):.2e}")
    assert abs(fine) > 1e-3 and abs(mine - fine) <= 10 * max(spread, solve)
    ctx.close()


# 8 ------------------------------------------------------------------------------------------------------------------------
def refused(call, *words):
    with pytest.raises(api.DDAMGError) as e:
        call()
    assert all(w in str(e.value) for w in words), str(e.value)


def test_refusals(monkeypatch, hip):
    lat = "8^4"
    U, X, Y = fields(lat)
    V = len(X)
    out = hip.alloc(nbytes(lat)); dx = hip.upload(X); dy = hip.upload(Y)
    # a process grid (every direction exchanged with itself)
    ctx = context(lat, "pivot", monkeypatch, grid=(-1, 1, 1, 1))
    y64 = ctx.vector(0, 64); x64 = ctx.vector(0, 64)
    refused(lambda: ctx.force_bilinear_vec(out, y64, x64), "process grid", "not built yet")
    refused(lambda: ctx.force_bilinear_device(out, dy, dx), "process grid")
    refused(lambda: ctx.force_logdet(out, 1), "process grid")
    y64.free(); x64.free(); ctx.close()
    ctx = context(lat, "pivot", monkeypatch)
    y64 = ctx.vector(0, 64).upload(Y); x64 = ctx.vector(0, 64).upload(X); y32 = ctx.vector(0, 32); x32 = ctx.vector(0, 32)
    good = by_vec(ctx, hip, lat, Y, X)
    # vectors, pointers, parity
    refused(lambda: ctx.force_bilinear_vec(out, y32, x32), "fp32")
    refused(lambda: ctx.force_bilinear_vec(out, y64, x32), "fp32")
    host = np.zeros(V * 72)
    refused(lambda: ctx.force_bilinear_vec(int(host.ctypes.data), y64, x64), "not a pointer into device memory")
    refused(lambda: ctx.force_bilinear_device(out, int(host.ctypes.data), dx), "not a pointer into device memory")
    refused(lambda: ctx.force_logdet(int(host.ctypes.data), 0), "not a pointer into device memory")
    refused(lambda: ctx.force_bilinear_device(0, dy, dx), "null")
    refused(lambda: ctx.force_bilinear_device(out, dy, out + 8 * 24), "overlap")                  # x_dev inside force_dev
    big = hip.alloc(nbytes(lat) + 8 * 24 * V)
    refused(lambda: ctx.force_bilinear_device(big + 8 * 24 * V, dy, big + 8 * 24), "overlap")     # force_dev reaching into the end of x_dev
    refused(lambda: ctx.force_bilinear_device(big, big + nbytes(lat) - 8, dx), "overlap")         # ... and y_dev's first real in its last
    refused(lambda: ctx.force_bilinear_device(out + 64, dy, dx), "smaller than the array")
    refused(lambda: ctx.force_logdet(out, 2), "parity")
    refused(lambda: ctx.force_logdet(out, -1), "parity")
    # operators with no single link field behind them
    ctx.set_operator(*ctx.get_operator())
    refused(lambda: ctx.force_bilinear_vec(out, y64, x64), "did not come from one link field")
    refused(lambda: ctx.force_logdet(out, 1), "did not come from one link field")
    ctx.set_gauge2(U, synth_field(LATTICES[lat][0], 6), anti_pbc=True)
    refused(lambda: ctx.force_bilinear_device(out, dy, dx), "did not come from one link field")
    ctx.set_gauge2_device(hip.upload(U), hip.upload(synth_field(LATTICES[lat][0], 6)), anti_pbc=True)
    refused(lambda: ctx.force_bilinear_device(out, dy, dx), "did not come from one link field")
    # ... and the context serves again once it has one
    ctx.set_gauge(U, anti_pbc=True)
    assert np.array_equal(by_vec(ctx, hip, lat, Y, X), good)
    for v in (y64, x64, y32, x32):
        v.free()
    ctx.close()


def test_a_singular_block_is_refused(monkeypatch, hip):
    """csw = 0 and m0 = -4: every clover block is zero"""
    lat = "4^4"
    L, B = LATTICES[lat]
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    ctx = dd.Context(params(L, [B] * 4, -4.0, 0.0))
    ctx.set_gauge(fields(lat)[0], anti_pbc=True)
    out = hip.alloc(nbytes(lat))
    refused(lambda: ctx.force_logdet(out, 1), "singular", "parity 1")
    ctx.close()
