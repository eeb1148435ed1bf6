"""The even-odd preconditioned system (-m gpu): Dhat = D_ee - D_eo D_oo^-1 D_oe on the even sites, its dagger, the half-field
layout kernels, log det D_ss of one parity, and the solves of Dhat, Dhat^dagger and Dhat^dagger Dhat with the odd part that belongs to
them.

The reference is built from existing pieces only (eo_reference.py): psi_o = -D_oo^-1 [D (phi_e, 0)]_o with the oracle's D and a numpy
inverse of the 6x6 blocks of get_operator(), Dhat phi_e = [D (phi_e, psi_o)]_e, whose odd part must vanish; at 4^4 also the Schur
complement of the oracle's matrix, which fixes the parity convention with no library code involved.

Bars.  fp64: 1e-13, the project's.  fp32: not fixed in advance but taken from the number format -- the distance from the fp64
reference of the same numpy restatement with operator, input, both intermediate vectors and the result rounded to fp32 (products in
fp64), measured on the four lattices below for both forms: 4.23e-08 (4^4), 4.25e-08 (4x6x8x10), 4.22e-08 (8^4), 4.25e-08 (4x4x12x12,
the largest, the dagger form).  The bar is ten times the largest: 4.25e-07."""
import os
import numpy as np
import pytest
from conftest import relerr, splitmix_uniform
from ddalphaamg_amd import api
import ddalphaamg_amd as dd
from oracle import orc, mg_oracle as mo
import eo_reference as eo
from test_gpu_device_interface import Hip, params, two_level_4, synth_field
from test_gpu_dagger import LATTICES, M0, CSW, context, inputs, hierarchy, rhs, norm

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G5 = eo.G5
EPS = np.finfo(np.float64).eps
BAR = {64: 1e-13, 32: 10 * 4.25e-08}
TOL = 1e-10
ROUND = 0.05 * TOL      # see test_solve_schur
# index table; tile tail (7.5 tiles); arithmetic neighbours and pivot links; three tiles in a direction
APPLY_LATTICES = ["4^4", "4x6x8x10", "8^4", "4x4x12x12"]


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.free_all()


def form_of(lat):
    return "pivot" if LATTICES[lat][1] == 4 else "table"


def rounded(a, prec):
    return a.astype(np.float32).astype(np.float64) if prec == 32 else a


def even_only(L, a, fill=0.0):
    """a on the even sites, `fill` on the odd ones"""
    return np.where(eo.parity(L)[:, None, None] == 1, fill, a)


def apply_vec(ctx, x, prec, dagger):
    """(ddamg_hip_schur_apply of x, the input vector after the call), downloaded"""
    a = ctx.vector(0, prec).upload(x); b = ctx.vector(0, prec)
    ctx.schur_apply(b, a, dagger=dagger)
    out, kept = b.download(), a.download()
    a.free(); b.free()
    return out, kept


_reference = {}


def reference(lat, ctx):
    """{dagger: Dhat(^dagger) of the lattice's input} in fp64, computed once; the odd part of the product must vanish"""
    if lat not in _reference:
        L = LATTICES[lat][0]
        D, cl = ctx.get_operator()
        _reference[lat] = {}
        for dagger in (False, True):
            out, rest, _ = eo.schur(L, D, cl, inputs(lat)[1], dagger)
            assert norm(rest) <= 1e-13 * norm(out), norm(rest) / norm(out)
            _reference[lat][dagger] = out
    return _reference[lat]


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lat", APPLY_LATTICES)
def test_schur_apply(lat, monkeypatch, hip):
    """both precisions and both forms against the reference; the odd sites of the input hold NaN and are not read, the odd sites
    of the output are zero, the input is not written; the dagger form is gamma5, schur_apply, gamma5 bit for bit; the half-field
    form is the vector form bit for bit; at 4^4 the Schur complement of the oracle's matrix and its conjugate transpose"""
    L = LATTICES[lat][0]
    ctx = context(lat, form_of(lat), monkeypatch)
    ref = reference(lat, ctx)
    odd = eo.parity(L) == 1
    x = even_only(L, inputs(lat)[1], np.nan)
    for prec in (64, 32):
        outs = {}
        for dagger in (False, True):
            out, kept = apply_vec(ctx, x, prec, dagger)
            assert np.array_equal(kept, rounded(x, prec), equal_nan=True)
            assert np.all(out[odd] == 0) and np.any(out[~odd] != 0)
            err = relerr(out, ref[dagger])
            print(lat, prec, "dagger" if dagger else "plain", "relerr", err, "bar", BAR[prec])
            assert err < BAR[prec], (prec, dagger, err)
            outs[dagger] = out
        # gamma5, schur_apply, gamma5 through the entry points
        a = ctx.vector(0, prec).upload(x); g = ctx.vector(0, prec); b = ctx.vector(0, prec)
        ctx.gamma5(g, a)
        ctx.schur_apply(b, g)
        ctx.gamma5(b, b)
        assert np.array_equal(b.download(), outs[True])
        for v in (a, g, b):
            v.free()
        if prec == 64:
            half = hip.upload(np.ascontiguousarray(inputs(lat)[1][~odd]))
            out_half = hip.alloc(half_bytes(L))
            for dagger in (False, True):
                ctx.schur_apply_device(out_half, half, dagger=dagger)
                assert np.array_equal(hip.download(out_half, (len(odd) // 2, 12, 2)), outs[dagger][~odd])
            assert np.array_equal(hip.download(half, (len(odd) // 2, 12, 2)), inputs(lat)[1][~odd])
            if lat == "4^4":
                S, even = eo.schur_matrix(mo.fine_matrix(L, *ctx.get_operator()), L)
                xe = mo.cplx(inputs(lat)[1]).ravel()[even]
                for dagger, M in ((False, S), (True, S.conj().T)):
                    full = np.zeros(len(odd) * 12, dtype=np.complex128)
                    full[even] = M @ xe
                    err = relerr(outs[dagger], mo.reim(full.reshape(-1, 12)))
                    print(lat, "against the matrix", "dagger" if dagger else "plain", err)
                    assert err < BAR[64]
    ctx.close()


def half_bytes(L):
    return int(np.prod(L)) // 2 * 24 * 8


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [32, 64])
def test_half_fields_round_trip(prec, monkeypatch, hip):
    """upload_parity / download_parity, both parities, with and without zero_other, sentinels on the parity that is not touched;
    against the lexicographic form of the same vector, so the half index is lex >> 1"""
    lat = "4x6x8x10"
    L = LATTICES[lat][0]
    V = int(np.prod(L))
    ctx = context(lat, "table", monkeypatch)
    field = splitmix_uniform(V * 24, 31).reshape(V, 12, 2)
    sentinel = splitmix_uniform(V * 24, 32).reshape(V, 12, 2) + 7.0
    v = ctx.vector(0, prec)
    for par in (0, 1):
        mine = eo.parity(L) == par
        half = np.ascontiguousarray(field[mine])
        d_half = hip.upload(half)
        for zero_other in (True, False):
            v.upload(sentinel)
            v.upload_parity_device(par, d_half, zero_other=zero_other)
            got = v.download()
            assert np.array_equal(got[mine], rounded(half, prec))
            assert np.array_equal(got[~mine], 0 * half if zero_other else rounded(sentinel[~mine], prec))
        back = hip.upload(np.full(half.shape, -3.0))
        v.download_parity_device(par, back)
        assert np.array_equal(hip.download(back, half.shape), rounded(half, prec))       # the round trip, bit for bit in fp64
        assert np.array_equal(hip.download(d_half, half.shape), half)                    # the source is not written
    v.free()
    ctx.close()


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(-1, 1, 1, 1), (1, 1, 1, -1), (-1, -1, -1, -1)], ids=["T", "X", "TZYX"])
def test_schur_apply_through_rccl_self_exchange(grid, monkeypatch):
    lat = "8^4"
    L = LATTICES[lat][0]
    x = even_only(L, inputs(lat)[1], np.nan)
    ctx = context(lat, "pivot", monkeypatch)
    whole = {(prec, dagger): apply_vec(ctx, x, prec, dagger)[0] for prec in (32, 64) for dagger in (False, True)}
    ctx.close()
    ctx = context(lat, "pivot", monkeypatch, grid=grid)
    for (prec, dagger), want in whole.items():
        out, _ = apply_vec(ctx, x, prec, dagger)
        err = relerr(out, want)
        print(grid, prec, dagger, "relerr", err)
        assert np.all(out[eo.parity(L) == 1] == 0) and err < BAR[prec]
    ctx.close()


# 4 ------------------------------------------------------------------------------------------------------------------------
def logdet_reference(L, cl, scale=(1.0, 1.0)):
    """[(sum of log|det block| over the sites of the parity, sign of the product, the bar 1e-13 sum |log|det block||)] for parity
    0, 1 from numpy.linalg.slogdet of the blocks times the scale of their parity"""
    B = eo.clover_blocks(cl)
    out = []
    for par in (0, 1):
        sg, ld = np.linalg.slogdet(scale[par] * B[eo.parity(L) == par])
        out.append((float(np.sum(ld)), int(round(float(np.prod(sg.real)))), 1e-13 * float(np.sum(np.abs(ld)))))
    return out


def check_logdet(ctx, L, scale=(1.0, 1.0), what=""):
    want = logdet_reference(L, ctx.get_operator()[1], scale)
    for par in (0, 1):
        got = ctx.clover_logdet(par)
        print(what, "parity", par, "log|det|", got[0], "numpy", want[par][0], "difference", abs(got[0] - want[par][0]), "bar", want[par][2])
        assert got == ctx.clover_logdet(par)                           # twice: the same bits
        assert got[1] == want[par][1] and abs(got[0] - want[par][0]) <= want[par][2], (par, got, want[par])


@pytest.mark.parametrize("lat", ["4x6x8x10", "8^4"])
def test_clover_logdet(lat, monkeypatch):
    """both parities against slogdet, twice with the same bits; it follows shift_mass and scale_clover without an upload
    (get_operator keeps showing the unscaled field, so the scaled reference is the unscaled blocks times the scale)"""
    L = LATTICES[lat][0]
    ctx = context(lat, form_of(lat), monkeypatch)
    check_logdet(ctx, L, what=lat)
    before = ctx.clover_logdet(1)[0]
    ctx.shift_mass(M0 + 0.05)
    check_logdet(ctx, L, what=lat + " shifted")
    assert ctx.clover_logdet(1)[0] != before
    ctx.scale_clover(1.1, 0.9)
    check_logdet(ctx, L, scale=(1.1, 0.9), what=lat + " scaled")
    ctx.close()


def hand_made_operator(ctx, L, edit):
    """set_operator with the links of the context and its clover field after edit(cl, parity)"""
    D, cl = ctx.get_operator()
    cl = cl.copy()
    edit(cl, eo.parity(L))
    ctx.set_operator(D, cl)
    return D, cl


def diagonal_block(cl, site, block, diag):
    cl[site, 6 * block:6 * block + 6, 0] = diag
    cl[site, 6 * block:6 * block + 6, 1] = 0
    cl[site, 12 + 15 * block:12 + 15 * (block + 1)] = 0


def test_clover_logdet_sign(monkeypatch):
    """exactly three odd sites with one negative eigenvalue in one block: sign -1 on the odd sites, +1 on the even ones"""
    lat = "4^4"
    L = LATTICES[lat][0]
    ctx = context(lat, "table", monkeypatch)

    def edit(cl, par):
        for k, site in enumerate(np.flatnonzero(par == 1)[[3, 40, 101]]):
            diagonal_block(cl, site, k % 2, [2.0, 3.0, -1.5, 2.5, 4.0, 3.5])
    hand_made_operator(ctx, L, edit)
    check_logdet(ctx, L, what="three negative eigenvalues")
    assert ctx.clover_logdet(1)[1] == -1 and ctx.clover_logdet(0)[1] == 1
    ctx.close()


def test_clover_logdet_refuses_a_singular_block(monkeypatch):
    """one exactly singular block on an even site: an error that names the parity, not a NaN; the other parity and the operator
    still work"""
    lat = "4^4"
    L = LATTICES[lat][0]
    ctx = context(lat, "table", monkeypatch)
    D, cl = hand_made_operator(ctx, L, lambda cl, par: diagonal_block(cl, np.flatnonzero(par == 0)[17], 1, [2.0, 3.0, 0.0, 2.5, 4.0, 3.5]))
    with pytest.raises(api.DDAMGError) as e:
        ctx.clover_logdet(0)
    assert "singular" in str(e.value) and "parity 0" in str(e.value)
    want = logdet_reference(L, cl)[1]
    got = ctx.clover_logdet(1)
    assert got[1] == 1 and abs(got[0] - want[0]) <= want[2]
    x = inputs(lat)[1]
    a = ctx.vector(0, 64).upload(x); b = ctx.vector(0, 64)
    ctx.dirac_apply(b, a)
    assert relerr(b.download(), orc.dirac_apply(L, D, cl, x, 64)) < 1e-13
    a.free(); b.free()
    ctx.close()


# 5 ------------------------------------------------------------------------------------------------------------------------
def even_rhs(L, fill=np.nan):
    """a right-hand side on the even sites; its odd sites hold `fill` (NaN: they are not read)"""
    return even_only(L, rhs(L), fill)


def solve_vec(ctx, b, dagger=False, guess=None, tol=TOL):
    """(the full-lattice vector that comes back, (iterations, coarse iterations, relres)) of ddamg_hip_solve_schur_vec"""
    vb = ctx.vector(0, 64).upload(b); vx = ctx.vector(0, 64)
    if guess is not None:
        vx.upload(guess)
    r = ctx.solve_schur_vec(vx, vb, tol, dagger=dagger, use_guess=guess is not None)
    x = vx.download()
    assert np.array_equal(vb.download(), b, equal_nan=True)
    vb.free(); vx.free()
    return x, r


def dense_pieces(ctx, L):
    """the dense blocks of the oracle's matrix by parity (4^4 only)"""
    A = mo.fine_matrix(L, *ctx.get_operator()).tocsr()
    even = np.flatnonzero(np.repeat(eo.parity(L), 12) == 0); odd = np.flatnonzero(np.repeat(eo.parity(L), 12) == 1)
    Aee, Aeo, Aoe, Aoo = (A[r][:, c].toarray() for r, c in ((even, even), (even, odd), (odd, even), (odd, odd)))
    return A, even, odd, Aee, Aeo, Aoe, np.linalg.inv(Aoo)


@pytest.mark.parametrize("which", ["4^4", "8^4"])
def test_solve_schur(which, hip):
    """both systems: relres <= tol and the Schur residual of the returned x_e in numpy; the odd part is the formula applied to the
    returned x_e, and the full vector X solves A X = (b_e, 0) to relres; the half-field form with and without x_o gives the same
    bits; memory returns; at 4^4 the residual to the rounding of the products and x_e within cond(Dhat) tol of the dense solution"""
    ctx, L = hierarchy(which)
    D, cl = ctx.get_operator()
    odd = eo.parity(L) == 1
    b = even_rhs(L)
    be = even_only(L, b)
    if which == "4^4":
        A, even, oddi, Aee, Aeo, Aoe, Aoo_inv = dense_pieces(ctx, L)
        S = Aee - Aeo @ Aoo_inv @ Aoe
    solve_vec(ctx, b, dagger=True)                                 # (the first call sizes whatever the context keeps)
    mem = api.memory_in_use()
    for dagger in (False, True):
        x, (it, cit, rr) = solve_vec(ctx, b, dagger)
        hist = ctx.residual_history()
        xe = even_only(L, x)
        Sx, _, psi = eo.schur(L, D, cl, xe, dagger)
        true = norm(be - Sx) / norm(be)
        err_odd = relerr(np.where(odd[:, None, None], x, 0.0), psi)
        full = G5 * orc.dirac_apply(L, D, cl, G5 * x, 64) if dagger else orc.dirac_apply(L, D, cl, x, 64)
        res_full = norm(be - full) / norm(be)
        print(which, "dagger" if dagger else "plain", "iterations", it, cit, "relres", rr, "numpy", true, "full system", res_full, "odd part", err_odd)
        assert it > 0 and len(hist) > 0 and rr <= TOL
        assert err_odd < 1e-13
        # the residuals agree to the rounding of the products, 2 * 64 eps || |Dhat| |x| || / ||b|| (computed below at 4^4, where the
        # matrix is at hand): 3e-14 times a ratio that stays below 180 on these lattices, a twentieth of tol
        assert abs(true - rr) <= ROUND and abs(res_full - rr) <= ROUND
        if which == "4^4":
            M = S.conj().T if dagger else S
            # rounding of the three chained products and of the diagonal one, 64 entries per row taken, device and numpy
            xa = np.abs(mo.cplx(x).ravel()[even])
            chain = np.abs(Aeo) @ (np.abs(Aoo_inv) @ (np.abs(Aoe) @ xa))
            bound = 2 * 64 * EPS * (norm(np.abs(Aee) @ xa) + 3 * norm(chain)) / norm(be)
            xc = mo.cplx(x).ravel()[even]; bc = mo.cplx(be).ravel()[even]
            exact = norm(bc - M @ xc) / norm(bc)
            print("bound", bound, "matrix residual", exact)
            assert abs(exact - rr) <= bound
            want = np.linalg.solve(M, bc)
            cond = np.linalg.cond(M)
            print("cond", cond, "error", norm(xc - want) / norm(want))
            assert norm(xc - want) / norm(want) <= cond * TOL
        # the half-field form, with the odd part and without
        db = hip.upload(np.ascontiguousarray(be[~odd])); dxe = hip.alloc(half_bytes(L)); dxo = hip.alloc(half_bytes(L))
        assert ctx.solve_schur_device(dxe, dxo, db, TOL, dagger=dagger) == (it, cit, rr)
        n = len(odd) // 2
        assert np.array_equal(hip.download(dxe, (n, 12, 2)), x[~odd]) and np.array_equal(hip.download(dxo, (n, 12, 2)), x[odd])
        dxe2 = hip.upload(np.zeros((n, 12, 2)))
        assert ctx.solve_schur_device(dxe2, None, db, TOL, dagger=dagger) == (it, cit, rr)
        assert np.array_equal(hip.download(dxe2, (n, 12, 2)), x[~odd])
        assert np.array_equal(ctx.residual_history(), hist)
    assert api.memory_in_use() == mem
    ctx.close()


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_solve_schur_from_a_guess():
    """a zero guess gives the bits and counts of use_guess = 0; a converged guess costs nothing and comes back as it is; the
    solution at a neighbouring mass is a guess that saves iterations; b = 0 gives x = 0 with zero counts"""
    ctx, L = hierarchy("4^4")
    b = even_rhs(L)
    odd = eo.parity(L)[:, None, None] == 1
    for dagger in (False, True):
        x, r = solve_vec(ctx, b, dagger)
        x0, r0 = solve_vec(ctx, b, dagger, guess=even_only(L, np.zeros_like(b), np.nan))      # the odd sites of a guess are not read
        assert r0 == r and np.array_equal(x0, x)
        x1, (it1, cit1, rr1) = solve_vec(ctx, b, dagger, guess=x)
        assert (it1, cit1) == (0, 0) and rr1 == r[2] and len(ctx.residual_history()) == 0
        assert np.array_equal(np.where(odd, 0.0, x1), np.where(odd, 0.0, x)) and np.array_equal(x1, x)
    x, (it, cit, rr) = solve_vec(ctx, b)
    ctx.shift_mass(0.3 + 1e-3)
    near, _ = solve_vec(ctx, b)
    ctx.shift_mass(0.3)
    x2, (it2, cit2, rr2) = solve_vec(ctx, b, guess=near)
    print("plain", it, "from the solution at the neighbouring mass", it2, "relres", rr2)
    assert 0 < it2 < it and rr2 <= TOL and relerr(x2, x) < 1e-8
    z, rz = solve_vec(ctx, np.zeros_like(b), guess=near)
    assert rz == (0, 0, 0.0) and not np.any(z)
    ctx.close()


# 7 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["4^4", "8^4"])
def test_solve_schur_squared(which, hip):
    """the two solves back to back: the counts come in pairs and x is that of the two calls; relres is that of Dhat^dagger Dhat in
    numpy; the half-field form gives the same bits"""
    ctx, L = hierarchy(which)
    D, cl = ctx.get_operator()
    odd = eo.parity(L) == 1
    b = even_rhs(L)
    be = even_only(L, b)
    y, (ity, city, _) = solve_vec(ctx, b, dagger=True)
    x0, (itx, citx, _) = solve_vec(ctx, even_only(L, y))
    hist0 = ctx.residual_history()
    vb = ctx.vector(0, 64).upload(b); vx = ctx.vector(0, 64)
    mem = api.memory_in_use()
    its, cits, rr = ctx.solve_schur_squared_vec(vx, vb, TOL)
    assert api.memory_in_use() == mem                              # y and the residual's workspace are gone
    x = vx.download()
    vb.free(); vx.free()
    assert np.array_equal(x, x0) and its == (ity, itx) and cits == (city, citx) and np.array_equal(ctx.residual_history(), hist0)
    xe = even_only(L, x)
    SHSx = eo.schur(L, D, cl, eo.schur(L, D, cl, xe)[0], True)[0]
    true = norm(be - SHSx) / norm(be)
    print(which, "iterations", its, cits, "relres", rr, "numpy", true)
    if which == "4^4":
        A, even, oddi, Aee, Aeo, Aoe, Aoo_inv = dense_pieces(ctx, L)
        S = Aee - Aeo @ Aoo_inv @ Aoe
        xc = mo.cplx(x).ravel()[even]; bc = mo.cplx(be).ravel()[even]
        # rounding of S x, carried through S^H, and that of the second product, as test_solve_squared bounds it; |S| entry-wise from the
        # pieces, 64 entries per row of every factor, three factors in the chain
        Sa = np.abs(Aee) + 3 * np.abs(Aeo) @ np.abs(Aoo_inv) @ np.abs(Aoe)
        bound = 2 * 64 * EPS * (norm(Sa.T @ (Sa @ np.abs(xc))) + norm(Sa.T @ np.abs(S @ xc))) / norm(bc)
        exact = norm(bc - S.conj().T @ (S @ xc)) / norm(bc)
        print("bound", bound, "matrix residual", exact)
        assert abs(exact - rr) <= bound
    assert abs(true - rr) <= ROUND
    n = len(odd) // 2
    db = hip.upload(np.ascontiguousarray(be[~odd])); dxe = hip.alloc(half_bytes(L)); dxo = hip.alloc(half_bytes(L))
    assert ctx.solve_schur_squared_device(dxe, dxo, db, TOL) == (its, cits, rr)
    assert np.array_equal(hip.download(dxe, (n, 12, 2)), x[~odd]) and np.array_equal(hip.download(dxo, (n, 12, 2)), x[odd])
    ctx.close()


# 8 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["mixed_precision_2", "method_minus_1"])
def test_solve_schur_with_the_other_solvers(variant):
    if variant == "mixed_precision_2":
        ctx, L = hierarchy("4^4", mixed_precision=2)
    else:
        L = [4] * 4
        p = params(L, [2] * 4, 0.3, 1.0)
        p.method, p.mixed_precision, p.restart, p.max_restart, p.tol = -1, 1, 50, 20, TOL
        ctx = dd.Context(p)
        ctx.set_gauge(synth_field(L, 2), anti_pbc=True)
    D, cl = ctx.get_operator()
    b = even_rhs(L)
    for dagger in (False, True):
        x, (it, cit, rr) = solve_vec(ctx, b, dagger)
        true = norm(even_only(L, b) - eo.schur(L, D, cl, even_only(L, x), dagger)[0]) / norm(even_only(L, b))
        print(variant, "dagger" if dagger else "plain", "iterations", it, "relres", rr, "numpy", true)
        assert it > 0 and rr <= TOL and abs(true - rr) <= ROUND
    ctx.close()


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_solve_schur_through_rccl_self_exchange(gold8):
    """the same iteration count +- 1 as undivided, relres <= tol; log det through the all-reduce"""
    from test_gpu_self_exchange import params as grid_params
    L = [8] * 4
    b = even_rhs(L)
    res = []
    for grid in ([1, 1, 1, 1], [-1, -1, -1, -1]):
        ctx = dd.Context(grid_params(gold8, grid, 2, 1))
        if grid[0] == -1:
            ctx.comm_init_rccl(api.rccl_unique_id())
        ctx.set_gauge(gold8["gauge"], anti_pbc=True)
        ctx.setup(2)
        x, r = solve_vec(ctx, b)
        res.append((x, r, ctx.clover_logdet(0), ctx.clover_logdet(1)))
        ctx.close()
    (x0, (it0, _, rr0), e0, o0), (x1, (it1, _, rr1), e1, o1) = res
    print("undivided", it0, rr0, "self-exchange", it1, rr1)
    assert rr0 <= TOL and rr1 <= TOL and abs(it1 - it0) <= 1 and relerr(x1, x0) < 1e-7
    assert e1 == e0 and o1 == o0              # one process: the all-reduce adds nothing


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_two_processes():
    """8x4x4x4 split in T over the host transport: log det on both ranks is the undivided value, one Schur solve reaches tol"""
    from launcher import torchrun
    r = torchrun(2, os.path.join(HERE, "dist_eo_worker.py"), "--grid", "2,1,1,1", timeout=300)
    print(r.stdout[-3000:])
    assert "DIST_EO_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# 11 -----------------------------------------------------------------------------------------------------------------------
def test_refusals(gold4, hip):
    q = two_level_4()
    q.m0, q.csw = float(gold4["meta_f64"][0]), float(gold4["meta_f64"][1])
    ctx = dd.Context(q)
    ctx.set_gauge(gold4["gauge"], anti_pbc=True)

    class Null:
        _h = None
    f32, g32, f64, g64, c32 = ctx.vector(0, 32), ctx.vector(0, 32), ctx.vector(0, 64), ctx.vector(0, 64), ctx.vector(1, 32)
    solves = (ctx.solve_schur_vec, ctx.solve_schur_squared_vec)
    n = 128 * 24
    host = np.zeros(n)
    d1 = hip.alloc(8 * n + 64); d2 = hip.alloc(8 * n); d3 = hip.alloc(8 * n); short = hip.alloc(8 * n) + 4 * n       # half an array behind `short`
    # before a setup: the solves only
    bad = [(f, (f64, g64)) for f in solves] + [(ctx.solve_schur_device, (d1, d2, d3)), (ctx.solve_schur_squared_device, (d1, None, d3))]
    for f, args in bad:
        with pytest.raises(api.DDAMGError) as e:
            f(*args)
        assert "setup" in str(e.value), (f.__name__, str(e.value))
    ctx.schur_apply(g64, f64); ctx.schur_apply(g32, f32); ctx.schur_apply_device(d1, d2); ctx.clover_logdet(0)     # these need none
    ctx.setup(2)
    calls = (ctx.schur_apply,) + solves
    bad = [(f, (Null, f64)) for f in calls] + [(f, (f64, Null)) for f in calls]
    bad += [(f, (c32, c32)) for f in calls]                                       # a coarse level
    bad += [(f, (f32, f64)) for f in calls]                                       # mixed precisions
    bad += [(f, (f32, g32)) for f in solves]                                      # the solves take fp64
    bad += [(f, (f64, f64)) for f in calls] + [(ctx.schur_apply, (f32, f32))]     # out == in
    hostp = int(host.ctypes.data)
    bad += [(ctx.schur_apply_device, a) for a in ((hostp, d2), (d2, hostp), (0, d2), (d2, 0), (d1, d1), (d1 + 64, d1), (short, d2), (d2, short))]
    for f in (ctx.solve_schur_device, ctx.solve_schur_squared_device):
        bad += [(f, a) for a in ((hostp, None, d2), (d2, None, hostp), (d2, hostp, d3), (0, None, d2), (d2, None, 0), (d1, None, d1), (d1 + 64, None, d1),
                                 (d2, d1, d1 + 64), (d2, d2, d3), (short, None, d2), (d2, short, d3), (d2, None, short))]
    bad += [(f64.upload_parity_device, (par, d2)) for par in (-1, 2)] + [(f64.download_parity_device, (par, d2)) for par in (-1, 2)]
    bad += [(f64.upload_parity_device, (0, hostp)), (f64.upload_parity_device, (0, short)), (f64.download_parity_device, (1, 0)),
            (c32.upload_parity_device, (0, d2))]
    bad += [(ctx.clover_logdet, (par,)) for par in (-1, 2)]
    for f, args in bad:
        with pytest.raises(api.DDAMGError) as e:
            f(*args)
        assert str(e.value), (f.__name__, args)
    # the context still solves
    b = even_rhs([4] * 4)
    f64.upload(b)
    it, cit, rr = ctx.solve_schur_vec(g64, f64, TOL)
    assert it > 0 and rr <= TOL
    for v in (f32, g32, f64, g64, c32):
        v.free()
    ctx.close()


def test_an_odd_local_extent_is_refused(hip):
    """refused before anything touches the operator, so none is needed; the context goes on working"""
    Lo = [4, 4, 2, 3]                          # an odd X extent: the pair 2k, 2k+1 straddles two rows
    ctx = dd.Context(params(Lo, Lo, 0.3, 1.0))
    V = int(np.prod(Lo))
    a, b = ctx.vector(0, 64), ctx.vector(0, 64)
    d = hip.alloc(8 * 24 * V)
    d2 = hip.alloc(8 * 24 * V)
    for f, args in ((ctx.schur_apply, (a, b)), (ctx.schur_apply_device, (d, d2)), (ctx.clover_logdet, (0,)), (a.upload_parity_device, (0, d)),
                    (a.download_parity_device, (0, d)), (ctx.solve_schur_vec, (a, b)), (ctx.solve_schur_device, (d, None, d2)),
                    (ctx.solve_schur_squared_vec, (a, b)), (ctx.solve_schur_squared_device, (d, None, d2))):
        with pytest.raises(api.DDAMGError) as e:
            f(*args)
        assert "even local lattice extents" in str(e.value), (f.__name__, str(e.value))
    x = splitmix_uniform(V * 24, 5).reshape(V, 12, 2)
    assert np.array_equal(a.upload(x).download(), x)
    a.free(); b.free()
    ctx.close()


# 12 -----------------------------------------------------------------------------------------------------------------------
def test_memory_returns(hip):
    """every new call once to size what the context keeps, then once more: memory_in_use is what it was; the context's workspace
    goes with the context"""
    start = api.memory_in_use()
    ctx, L = hierarchy("4^4")
    V = 256
    odd = eo.parity(L) == 1
    b = even_rhs(L, 0.0)
    half = hip.upload(np.ascontiguousarray(b[~odd])); h2 = hip.alloc(half_bytes(L)); h3 = hip.alloc(half_bytes(L))

    def everything():
        for prec in (32, 64):
            u = ctx.vector(0, prec); w = ctx.vector(0, prec)
            u.upload_parity_device(0, half)
            ctx.schur_apply(w, u); ctx.schur_apply(w, u, dagger=True)
            w.download_parity_device(0, h2)
            u.free(); w.free()
        ctx.schur_apply_device(h2, half)
        ctx.clover_logdet(0); ctx.clover_logdet(1)
        vb = ctx.vector(0, 64).upload(b); vx = ctx.vector(0, 64)
        ctx.solve_schur_vec(vx, vb, TOL); ctx.solve_schur_vec(vx, vb, TOL, dagger=True, use_guess=True)
        ctx.solve_schur_squared_vec(vx, vb, TOL)
        vb.free(); vx.free()
        ctx.solve_schur_device(h2, h3, half, TOL)
        ctx.solve_schur_squared_device(h2, None, half, TOL)
    everything()
    mem = api.memory_in_use()
    everything()
    assert api.memory_in_use() == mem
    ctx.close()
    assert api.memory_in_use() == start
