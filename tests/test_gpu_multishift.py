"""Multi-shift CG on Dhat^dagger Dhat + sigma_s (-m gpu): ddamg_hip_solve_schur_multishift_vec / _device against the numpy statement
of the same recurrence (multishift_reference.py) on the operator the context holds, against dense solves at 4^4, and
ddamg_hip_schur_odd_part_device against the even-odd reference.

Lattices of the parity test: 4^4 (index table, the dense matrix at hand; 128 even sites x 12 rows = 6 full workgroups of the update
kernel), 4x4x6x6 (288 even sites x 12 = 13.5 workgroups: the last one is half filled), 8^4 with 4^4 blocks (arithmetic neighbours,
pivot links, 96 workgroups).

Bars.  Iteration counts: the reference's +- 1 (the two recurrences differ by rounding, which can move the crossing of tol by a
step).  relres <= 2 tol: the loop stops on the recursed residual, the reported one is recomputed (the project's convention,
test_solve_dagger).  |relres - numpy's residual of the downloaded x_s| <= ROUND of test_gpu_eo_system.py, the rounding of the
operator products.  Error against the dense solution: ||x - A^-1 b|| <= cond(A) ||b - A x|| / ||A|| ... <= cond(A) relres, and relres
<= 2 tol, so 2 cond tol.  Odd part: 1e-13, the project's fp64 bar."""
import os
import numpy as np
import pytest
from conftest import relerr, splitmix_uniform
from ddalphaamg_amd import api
import ddalphaamg_amd as dd
from oracle import orc, mg_oracle as mo
import eo_reference as eo
import force_reference as fr
import multishift_reference as ms
from test_gpu_device_interface import Hip, params, two_level_4, synth_field
from test_gpu_dagger import LATTICES, SWITCHES, M0, CSW, context, inputs, hierarchy, rhs, norm
from test_gpu_eo_system import even_only, half_bytes, TOL, ROUND

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SHIFTS = [0.0, 1e-3, 1e-2, 0.1, 1.0, 10.0, 100.0]
EXTRA = {"4x4x6x6": ([4, 4, 6, 6], 2)}          # the tail case of the update kernel; not among the lattices of test_gpu_dagger


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.free_all()


def lattice(lat):
    return LATTICES[lat] if lat in LATTICES else EXTRA[lat]


def one_level(lat, monkeypatch, grid=(1, 1, 1, 1)):
    """a one-level context at (M0, CSW) on the synthetic field of seed 5: test_gpu_dagger's where it knows the lattice"""
    if lat in LATTICES:
        return context(lat, "pivot" if LATTICES[lat][1] == 4 else "table", monkeypatch, grid=grid)
    L, B = EXTRA[lat]
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    ctx = dd.Context(params(L, [B] * 4, M0, CSW))
    ctx.set_gauge(synth_field(L, 5), anti_pbc=True)
    return ctx


_ops, _refs = {}, {}


def operator(key, ctx, L):
    """(v -> Dhat^dagger Dhat v on the even unknowns from the oracle's matrix of ctx.get_operator(), the even indices), made once per key"""
    if key not in _ops:
        _ops[key] = ms.sparse_normal_operator(mo.fine_matrix(L, *ctx.get_operator()), L)
    return _ops[key]


def reference(key, ctx, L, b, shifts=SHIFTS, tols=TOL, max_iterations=2000):
    """multishift_reference.multishift_cg on the context's operator and the even part of b, made once per set of arguments"""
    full = (key, tuple(shifts), tuple(np.atleast_1d(tols)), max_iterations)
    if full not in _refs:
        op, even = operator(key, ctx, L)
        _refs[full] = ms.multishift_cg(op, mo.cplx(even_only(L, b)).ravel()[even], shifts, tols, max_iterations)
    return _refs[full]


def true_residual(key, ctx, L, b, x, sigma):
    """||b_e - (Dhat^dagger Dhat + sigma) x_e|| / ||b_e|| in numpy, of a downloaded full-lattice x"""
    op, even = operator(key, ctx, L)
    bc, xc = mo.cplx(even_only(L, b)).ravel()[even], mo.cplx(x).ravel()[even]
    return norm(bc - op(xc) - sigma * xc) / norm(bc)


def run_vec(ctx, b, shifts, tols=None, max_iterations=0):
    """(the full-lattice vectors that come back, (iterations, relres, ritz)) of ddamg_hip_solve_schur_multishift_vec; b is not written"""
    vb = ctx.vector(0, 64).upload(b)
    xs = [ctx.vector(0, 64).upload(np.full(b.shape, 7.0)) for _ in shifts]
    out = ctx.solve_schur_multishift_vec(shifts, xs, vb, tols, max_iterations)
    x = [v.download() for v in xs]
    assert np.array_equal(vb.download(), b, equal_nan=True)
    for v in xs + [vb]:
        v.free()
    return x, out


def run_device(ctx, hip, L, b, shifts, tols=None, max_iterations=0, odd_parts=True):
    """the same through the half-field form: ([x_e], [x_o or None], (iterations, relres, ritz)); odd_parts: True, None, or a mask"""
    odd = eo.parity(L) == 1
    n = len(odd) // 2
    db = hip.upload(np.ascontiguousarray(even_only(L, b)[~odd]))
    xe = [hip.upload(np.full((n, 12, 2), 7.0)) for _ in shifts]
    mask = [True] * len(shifts) if odd_parts is True else odd_parts
    xo = None if mask is None else [hip.upload(np.full((n, 12, 2), 7.0)) if m else None for m in mask]
    out = ctx.solve_schur_multishift_device(shifts, xe, xo, db, tols, max_iterations)
    assert np.array_equal(hip.download(db, (n, 12, 2)), even_only(L, b)[~odd])
    return ([hip.download(p, (n, 12, 2)) for p in xe], None if xo is None else [hip.download(p, (n, 12, 2)) if p else None for p in xo], out)


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lat", ["4^4", "4x4x6x6", "8^4"])
def test_parity_with_the_reference(lat, monkeypatch, hip):
    L = lattice(lat)[0]
    ctx = one_level(lat, monkeypatch)
    D, cl = ctx.get_operator()
    odd = eo.parity(L) == 1
    b = even_only(L, rhs(L), np.nan)                  # NaN on the odd sites of b: not read
    x, (its, rr, ritz) = run_vec(ctx, b, SHIFTS, [TOL] * len(SHIFTS))
    hist = ctx.residual_history()
    xr, itr, al, be, histr, T = reference(lat, ctx, L, b)
    print(lat, "iterations", its, "reference", list(itr), "relres", ["%.2e" % r for r in rr], "ritz", ritz)
    assert len(hist) == max(its) and abs(len(hist) - len(histr)) <= 1           # ||r_k|| / ||b|| of the base system
    m = min(len(hist), len(histr))
    assert np.allclose(hist[:m], histr[:m], rtol=1e-6, atol=ROUND)
    for s, sigma in enumerate(SHIFTS):
        assert abs(its[s] - itr[s]) <= 1, (s, its[s], itr[s])
        assert rr[s] <= 2 * TOL, (s, rr[s])
        true = true_residual(lat, ctx, L, b, x[s], sigma)
        psi = eo.schur(L, D, cl, even_only(L, x[s]))[2]
        err_odd = relerr(np.where(odd[:, None, None], x[s], 0.0), psi)
        print(" shift", sigma, "relres", rr[s], "numpy", true, "odd part", err_odd)
        assert abs(true - rr[s]) <= ROUND and err_odd < 1e-13
    if lat == "4^4":
        Q, even = ms.dense_normal_operator(mo.fine_matrix(L, D, cl), L)
        ev = np.linalg.eigvalsh(Q)
        bc = mo.cplx(even_only(L, b)).ravel()[even]
        for s, sigma in enumerate(SHIFTS):
            want = np.linalg.solve(Q + sigma * np.eye(len(bc)), bc)
            err = norm(mo.cplx(x[s]).ravel()[even] - want) / norm(want)
            cond = (ev[-1] + sigma) / (ev[0] + sigma)
            print(" shift", sigma, "error against the dense solution", err, "bar", 2 * cond * TOL)
            assert err <= 2 * cond * TOL
        rayleigh = (np.vdot(bc, Q @ bc) / np.vdot(bc, bc)).real
        slack = 1e-10 * ev[-1]
        print(" spectrum", ev[0], ev[-1], "ritz", ritz, "rayleigh", rayleigh)
        assert ev[0] - slack <= ritz[0] <= rayleigh <= ritz[1] <= ev[-1] + slack
    # the half-field form: the same bits, with the odd parts, with some of them, with none
    xe, xo, out = run_device(ctx, hip, L, b, SHIFTS, None)
    assert out == (its, rr, ritz) and np.array_equal(ctx.residual_history(), hist)
    for s in range(len(SHIFTS)):
        assert np.array_equal(xe[s], x[s][~odd]) and np.array_equal(xo[s], x[s][odd])
    mask = [s % 2 == 0 for s in range(len(SHIFTS))]
    xe, xo, out = run_device(ctx, hip, L, b, SHIFTS, [0.0] * len(SHIFTS), odd_parts=mask)     # an entry <= 0: params.tol = TOL
    assert ctx.params.tol == TOL and out == (its, rr, ritz)
    for s in range(len(SHIFTS)):
        assert np.array_equal(xe[s], x[s][~odd]) and (xo[s] is None or np.array_equal(xo[s], x[s][odd]))
    xe, xo, out = run_device(ctx, hip, L, b, SHIFTS, odd_parts=None)
    assert out == (its, rr, ritz) and all(np.array_equal(xe[s], x[s][~odd]) for s in range(len(SHIFTS)))
    ctx.close()


# 2 ------------------------------------------------------------------------------------------------------------------------
def test_a_converged_shift_is_frozen(monkeypatch):
    """the largest shift converges first and is left alone from then on: a run that stops there returns its bits"""
    lat = "4^4"
    L = lattice(lat)[0]
    ctx = one_level(lat, monkeypatch)
    b = even_only(L, rhs(L))
    x, (its, rr, _) = run_vec(ctx, b, SHIFTS)
    s = len(SHIFTS) - 1
    assert all(its[t] > its[s] for t in range(s)), its
    y, (jts, _, _) = run_vec(ctx, b, SHIFTS, max_iterations=its[s])
    assert jts == [its[s]] * len(SHIFTS) and np.array_equal(y[s], x[s])
    assert not np.array_equal(y[0], x[0])
    ctx.close()


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_a_shift_does_not_depend_on_its_place_or_its_company(monkeypatch):
    lat = "4x4x6x6"
    L = lattice(lat)[0]
    ctx = one_level(lat, monkeypatch)
    b = even_only(L, rhs(L))
    s0, sa, sb, sc = 0.01, 0.5, 2.0, 30.0
    x, r = run_vec(ctx, b, [s0, sa, sb, sc])
    y, q = run_vec(ctx, b, [sc, s0, sb])
    assert np.array_equal(y[1], x[0]) and np.array_equal(y[2], x[2]) and np.array_equal(y[0], x[3])
    assert (q[0][1], q[0][2], q[0][0]) == (r[0][0], r[0][2], r[0][3]) and (q[1][1], q[1][2], q[1][0]) == (r[1][0], r[1][2], r[1][3])
    assert q[2] == r[2]
    z, t = run_vec(ctx, b, [s0, sb, sb, s0, sc])          # duplicates, of the base system too
    assert np.array_equal(z[1], z[2]) and np.array_equal(z[0], z[3]) and np.array_equal(z[0], x[0]) and np.array_equal(z[1], x[2])
    assert t[0][1] == t[0][2] and t[0][0] == t[0][3] and t[1][1] == t[1][2] and t[1][0] == t[1][3]
    x2, r2 = run_vec(ctx, b, [s0, sa, sb, sc])            # twice: the same bits
    assert r2 == r and all(np.array_equal(u, v) for u, v in zip(x2, x))
    ctx.close()


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_one_shift_zero_is_the_squared_solve(hip):
    """sigma = 0 alone against ddamg_hip_solve_schur_squared_device: both solve Dhat^dagger Dhat x = b, to their residuals"""
    ctx, L = hierarchy("4^4")
    odd = eo.parity(L) == 1
    n = len(odd) // 2
    b = even_only(L, rhs(L))
    xe, xo, (its, rr, _) = run_device(ctx, hip, L, b, [0.0])
    db = hip.upload(np.ascontiguousarray(b[~odd])); de = hip.alloc(half_bytes(L)); do = hip.alloc(half_bytes(L))
    _, _, rr_b = ctx.solve_schur_squared_device(de, do, db, TOL)
    want_e, want_o = hip.download(de, (n, 12, 2)), hip.download(do, (n, 12, 2))
    Q, _ = ms.dense_normal_operator(mo.fine_matrix(L, *ctx.get_operator()), L)
    cond = np.linalg.cond(Q)
    err = relerr(xe[0], want_e)
    print("iterations", its, "relres", rr, "squared solve", rr_b, "cond", cond, "difference", err, "odd parts", relerr(xo[0], want_o))
    assert rr[0] <= 2 * TOL and err <= cond * (TOL + rr_b)
    ctx.close()


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_tolerances_per_shift(monkeypatch):
    lat = "4^4"
    L = lattice(lat)[0]
    ctx = one_level(lat, monkeypatch)
    b = even_only(L, rhs(L))
    tols = [1e-10, 1e-6, 1e-10, 1e-4, 1e-10, 1e-8, 1e-10]
    _, (strict, _, _) = run_vec(ctx, b, SHIFTS)
    x, (its, rr, _) = run_vec(ctx, b, SHIFTS, tols)
    itr = reference(lat, ctx, L, b, SHIFTS, tols)[1]
    print("iterations", its, "reference", list(itr), "all at 1e-10", strict, "relres", rr)
    for s in range(len(SHIFTS)):
        assert abs(its[s] - itr[s]) <= 1 and rr[s] <= 2 * tols[s]
        assert its[s] < strict[s] if tols[s] > 1e-10 else its[s] == strict[s]
    ctx.close()


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_a_starved_run_reports_what_it_reached(monkeypatch):
    lat = "4^4"
    L = lattice(lat)[0]
    ctx = one_level(lat, monkeypatch)
    b = even_only(L, rhs(L))
    x, (its, rr, ritz) = run_vec(ctx, b, SHIFTS, max_iterations=3)
    xr, itr, *_ = reference(lat, ctx, L, b, SHIFTS, TOL, 3)
    op, even = operator(lat, ctx, L)
    bc = mo.cplx(b).ravel()[even]
    assert its == [3] * len(SHIFTS) and list(itr) == its and len(ctx.residual_history()) == 3
    for s, sigma in enumerate(SHIFTS):
        want = norm(bc - op(xr[s]) - sigma * xr[s]) / norm(bc)
        print(" shift", sigma, "relres", rr[s], "reference after three steps", want)
        assert rr[s] > 100 * TOL and abs(rr[s] - want) <= ROUND
    ctx.close()


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_a_zero_right_hand_side(monkeypatch, hip):
    lat = "4^4"
    L = lattice(lat)[0]
    ctx = one_level(lat, monkeypatch)
    x, out = run_vec(ctx, np.zeros_like(rhs(L)), SHIFTS)
    assert out == ([0] * len(SHIFTS), [0.0] * len(SHIFTS), (0.0, 0.0)) and not np.any(x) and len(ctx.residual_history()) == 0
    xe, xo, out = run_device(ctx, hip, L, np.zeros_like(rhs(L)), SHIFTS[:2])
    assert out == ([0, 0], [0.0, 0.0], (0.0, 0.0)) and not np.any(xe) and not np.any(xo)
    ctx.close()


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_schur_odd_part_device(monkeypatch, hip):
    """both forms against the even-odd reference on 4x6x8x10; with the bits of the odd part ddamg_hip_solve_schur_device returns"""
    lat = "4x6x8x10"
    L = lattice(lat)[0]
    ctx = one_level(lat, monkeypatch)
    D, cl = ctx.get_operator()
    odd = eo.parity(L) == 1
    n = len(odd) // 2
    x = even_only(L, inputs(lat)[1])
    de = hip.upload(np.ascontiguousarray(x[~odd])); do = hip.upload(np.full((n, 12, 2), 7.0))
    for dagger in (False, True):
        ctx.schur_odd_part_device(do, de, dagger=dagger)
        psi = eo.schur(L, D, cl, x, dagger)[2]
        err = relerr(hip.download(do, (n, 12, 2)), psi[odd])
        print(lat, "dagger" if dagger else "plain", "relerr", err)
        assert err < 1e-13 and np.array_equal(hip.download(de, (n, 12, 2)), x[~odd])
    ctx.close()
    ctx, L = hierarchy("4^4")
    odd = eo.parity(L) == 1
    n = len(odd) // 2
    db = hip.upload(np.ascontiguousarray(rhs(L)[~odd]))
    de, do, d2 = hip.alloc(half_bytes(L)), hip.alloc(half_bytes(L)), hip.alloc(half_bytes(L))
    for dagger in (False, True):
        ctx.solve_schur_device(de, do, db, TOL, dagger=dagger)
        ctx.schur_odd_part_device(d2, de, dagger=dagger)
        assert np.array_equal(hip.download(d2, (n, 12, 2)), hip.download(do, (n, 12, 2)))
    ctx.close()


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_the_rational_force(monkeypatch, hip):
    """S = sum_s rho_s phi^dagger (Dhat^dagger Dhat + sigma_s)^-1 phi through the multi-shift solve on perturbed links, against
    sum_s rho_s force_bilinear(Y_s, X_s, -2) with X_s = x_s and its odd part, Y_s = Dhat x_s and the dagger odd part"""
    FTOL = 1e-12
    H = 2.0 ** -8
    lat = "4^4"
    L = lattice(lat)[0]
    V = int(np.prod(L)); n = V // 2
    ctx = one_level(lat, monkeypatch)
    U = inputs(lat)[0]
    odd = eo.parity(L) == 1
    phi = np.ascontiguousarray(rhs(L)[~odd])
    shifts, rho = [0.05, 0.7, 9.0], [0.3, 1.1, 2.5]
    omega = fr.random_algebra(np.random.default_rng(33), (V, 4))
    dphi = hip.upload(phi)
    dxe = [hip.alloc(phi.nbytes) for _ in shifts]; dxo = [hip.alloc(phi.nbytes) for _ in shifts]
    dye, dyo = hip.alloc(phi.nbytes), hip.alloc(phi.nbytes)

    def S(eps):
        ctx.set_gauge_device(hip.upload(fr.perturbed(U, omega, eps)), anti_pbc=True)
        ctx.solve_schur_multishift_device(shifts, dxe, None, dphi, [FTOL] * 3)
        return float(sum(r * np.sum(phi * hip.download(p, phi.shape)) for r, p in zip(rho, dxe)))
    fine, coarse = fr.richardson(S, H), fr.richardson(S, 2 * H)
    s0 = S(0.0)
    its, rr, _ = ctx.solve_schur_multishift_device(shifts, dxe, dxo, dphi, [FTOL] * 3)
    out = hip.alloc(V * 72 * 8)
    for s in range(len(shifts)):
        ctx.schur_apply_device(dye, dxe[s])
        ctx.schur_odd_part_device(dyo, dye, dagger=True)
        X = np.empty((V, 12, 2)); Y = np.empty((V, 12, 2))
        X[~odd], X[odd] = hip.download(dxe[s], phi.shape), hip.download(dxo[s], phi.shape)
        Y[~odd], Y[odd] = hip.download(dye, phi.shape), hip.download(dyo, phi.shape)
        ctx.force_bilinear_device(out, hip.upload(Y), hip.upload(X), -2.0 * rho[s], accumulate=s > 0)
    mine = fr.pairing(omega, hip.download(out, (V, 4, 9, 2)))
    spread, solve = abs(fine - coarse), FTOL * abs(s0) / H
    print(f"S {s0:.12e} derivative {fine:+.12e} force {mine:+.12e} spread {spread:.2e} solve {solve:.2e} difference {abs(mine - fine):.2e}", its, rr)
    assert abs(fine) > 1e-3 and abs(mine - fine) <= 10 * max(spread, solve)
    ctx.close()


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_through_rccl_self_exchange(monkeypatch):
    """every direction exchanged with itself against the undivided run: counts +- 1, relres <= 2 tol, the solutions within 1e-7"""
    lat = "8^4"
    L = lattice(lat)[0]
    b = even_only(L, rhs(L))
    shifts = [0.0, 0.1, 10.0]
    res = []
    for grid in ((1, 1, 1, 1), (-1, -1, -1, -1)):
        ctx = one_level(lat, monkeypatch, grid=grid)
        res.append(run_vec(ctx, b, shifts))
        ctx.close()
    (x0, (it0, rr0, rz0)), (x1, (it1, rr1, rz1)) = res
    print("undivided", it0, rr0, rz0, "self-exchange", it1, rr1, rz1)
    for s in range(len(shifts)):
        assert abs(it1[s] - it0[s]) <= 1 and rr0[s] <= 2 * TOL and rr1[s] <= 2 * TOL and relerr(x1[s], x0[s]) < 1e-7


# 11 -----------------------------------------------------------------------------------------------------------------------
def test_two_processes():
    """8x4x4x4 split in T over the host transport: three shifts, every rank reaches 2 tol with the same counts"""
    from launcher import torchrun
    r = torchrun(2, os.path.join(HERE, "dist_multishift_worker.py"), "--grid", "2,1,1,1", timeout=300)
    print(r.stdout[-3000:])
    assert "DIST_MULTISHIFT_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# 12 -----------------------------------------------------------------------------------------------------------------------
def refused(call, *words):
    with pytest.raises(api.DDAMGError) as e:
        call()
    assert all(w in str(e.value) for w in words), str(e.value)


def test_refusals(monkeypatch, hip):
    lat = "4^4"
    L = lattice(lat)[0]
    V = int(np.prod(L)); n = V * 12
    ctx = dd.Context(two_level_4())
    f64, g64, h64, f32, c32 = ctx.vector(0, 64), ctx.vector(0, 64), ctx.vector(0, 64), ctx.vector(0, 32), ctx.vector(1, 32)
    d1 = hip.alloc(8 * n + 64); d2 = hip.alloc(8 * n); d3 = hip.alloc(8 * n); short = hip.alloc(8 * n) + 4 * n
    host = np.zeros(n); hostp = int(host.ctypes.data)
    vec, dev, oddp = ctx.solve_schur_multishift_vec, ctx.solve_schur_multishift_device, ctx.schur_odd_part_device
    # no operator yet
    refused(lambda: vec([0.0], [g64], f64), "no operator")
    refused(lambda: dev([0.0], [d1], None, d2), "no operator")
    refused(lambda: oddp(d1, d2), "no operator")
    ctx.set_gauge(synth_field(L, 2), anti_pbc=True)
    # the shifts
    refused(lambda: vec([], [], f64), "nshift")
    refused(lambda: vec([0.0] * 33, [g64] * 33, f64), "nshift")
    refused(lambda: dev([], [], None, d2), "nshift")
    for bad in (-1e-3, np.inf, np.nan):
        refused(lambda: vec([0.0, bad], [g64, h64], f64), "finite and not negative")
        refused(lambda: dev([bad], [d1], None, d2), "finite and not negative")
    # the vectors
    refused(lambda: vec([0.0], [f32], f64), "fine-level fp64")
    refused(lambda: vec([0.0], [g64], f32), "fine-level fp64")
    refused(lambda: vec([0.0], [c32], f64), "fine-level fp64")
    refused(lambda: vec([0.0], [f64], f64), "two vectors")
    refused(lambda: vec([0.0, 1.0], [g64, f64], f64), "two vectors")
    refused(lambda: vec([0.0, 1.0], [g64, g64], f64), "distinct")
    # the arrays
    refused(lambda: dev([0.0], [hostp], None, d2), "not a pointer into device memory")
    refused(lambda: dev([0.0], [d1], None, hostp), "not a pointer into device memory")
    refused(lambda: dev([0.0], [d1], [hostp], d2), "not a pointer into device memory")
    refused(lambda: dev([0.0], [0], None, d2), "null")
    refused(lambda: dev([0.0], [d1], None, 0), "null")
    refused(lambda: dev([0.0], [short], None, d2), "smaller than the array")
    refused(lambda: dev([0.0], [d1], [short], d2), "smaller than the array")
    refused(lambda: dev([0.0], [d1], None, short), "smaller than the array")
    refused(lambda: dev([0.0], [d2], None, d2), "overlap")
    refused(lambda: dev([0.0], [d1 + 64], None, d1), "overlap")
    refused(lambda: dev([0.0, 1.0], [d1, d1 + 64], None, d2), "overlap")
    refused(lambda: dev([0.0, 1.0], [d1, d3], [None, d1], d2), "overlap")
    refused(lambda: dev([0.0], [d1], [d2], d2), "overlap")
    for args, word in (((hostp, d2), "not a pointer into device memory"), ((d2, hostp), "not a pointer into device memory"), ((0, d2), "null"),
                       ((d2, 0), "null"), ((short, d2), "smaller than the array"), ((d2, short), "smaller than the array"), ((d1, d1), "overlap"),
                       ((d1 + 64, d1), "overlap")):
        refused(lambda: oddp(*args), word)
    # the context still works, without a setup
    f64.upload(even_only(L, rhs(L)))
    its, rr, _ = vec([0.0, 1.0], [g64, h64], f64)
    assert min(its) > 0 and max(rr) <= 2 * ctx.params.tol
    for v in (f64, g64, h64, f32, c32):
        v.free()
    ctx.close()
    # an odd local extent: refused before anything touches the operator, so none is needed
    Lo = [4, 4, 2, 3]
    ctx = dd.Context(params(Lo, Lo, 0.3, 1.0))
    a, b = ctx.vector(0, 64), ctx.vector(0, 64)
    e1 = hip.alloc(8 * 24 * 96); e2 = hip.alloc(8 * 24 * 96)
    refused(lambda: ctx.solve_schur_multishift_vec([0.0], [a], b), "even local lattice extents")
    refused(lambda: ctx.solve_schur_multishift_device([0.0], [e1], None, e2), "even local lattice extents")
    refused(lambda: ctx.schur_odd_part_device(e1, e2), "even local lattice extents")
    a.free(); b.free()
    ctx.close()


# 13 -----------------------------------------------------------------------------------------------------------------------
def test_memory_returns(monkeypatch, hip):
    """the first call sizes what the context keeps (the reduction workspace, the list of even sites, the even-odd work vectors); a
    second one leaves memory_in_use as it was, and everything goes with the context"""
    start = api.memory_in_use()
    lat = "4^4"
    L = lattice(lat)[0]
    ctx = one_level(lat, monkeypatch)
    b = even_only(L, rhs(L))

    def everything():
        run_vec(ctx, b, SHIFTS)
        xe, _, _ = run_device(ctx, hip, L, b, SHIFTS[:3])
        hip.free_all()
        d1 = hip.upload(xe[0]); d2 = hip.alloc(half_bytes(L))
        ctx.schur_odd_part_device(d2, d1); ctx.schur_odd_part_device(d2, d1, dagger=True)
        hip.free_all()
    everything()
    mem = api.memory_in_use()
    everything()
    assert api.memory_in_use() == mem
    ctx.close()
    assert api.memory_in_use() == start
