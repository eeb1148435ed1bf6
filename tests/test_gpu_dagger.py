"""D^dagger in one pass, gamma5, and the D^dagger / D^dagger D solves (-m gpu): ddamg_hip_dirac_apply_dagger against the three-pass form
gamma5, D, gamma5 bit for bit in every link and clover form, on one process and through the RCCL self-exchange, and against the
adjoint of the oracle's matrix; ddamg_hip_gamma5 against numpy; the solves against the gamma5-wrapped solves of D and against the
oracle's residuals.

What catches a seeded fault (run once against three libraries built with the fault, loaded through DDAMG_HIP_LIBRARY):
  no sign on the face reads from global memory: test_dagger_is_the_three_pass_form_bit_for_bit on every lattice of more than one tile,
                                                test_dagger_is_the_adjoint on the same lattices;
  no sign in halo_pack_kernel:                  test_dagger_through_rccl_self_exchange (all six cases);
  the sign on spin 2, 3 at the store:           every case of the three tests above (the result is the negative)."""
import numpy as np
import pytest
from conftest import load_golden, relerr, splitmix_uniform
from ddalphaamg_amd import api
import ddalphaamg_amd as dd
from oracle import orc, mg_oracle as mo
from test_gpu_device_interface import Hip, params, two_level_4, params_8_b4, check_dirac, synth_field

pytestmark = pytest.mark.gpu
G5 = np.array([-1.0] * 6 + [1.0] * 6)[None, :, None]
M0, CSW = -0.1, 1.0
# (T, Z, Y, X), block: one tile; 16 tiles in the XCD-aware order; three tiles in each direction in turn, so that the +mu and -mu
# neighbour tiles differ; index-table neighbours and a tile tail (1920 sites = 7.5 tiles)
LATTICES = {"4^4": ([4] * 4, 2), "8^4": ([8] * 4, 4), "12x12x4x4": ([12, 12, 4, 4], 4), "4x4x12x12": ([4, 4, 12, 12], 4), "4x6x8x10": ([4, 6, 8, 10], 2)}
# switches -> reals per link that ran; "table": 2^4 blocks, the index table (full links)
FORMS = {"pivot": ({}, 10), "two-row": ({"DDAMG_LINK_PIVOT": "0"}, 12), "full": ({"DDAMG_LINK_COMPRESSION": "0"}, 18),
         "pivot-clover72": ({"DDAMG_CLOVER_COMPRESSION": "0"}, 10), "table": ({}, 18), "table-clover72": ({"DDAMG_CLOVER_COMPRESSION": "0"}, 18)}
CASES = [(lat, form) for lat, (L, B) in LATTICES.items() for form in (("pivot", "two-row", "full", "pivot-clover72") if B == 4 else ("table", "table-clover72"))]
SWITCHES = ("DDAMG_LINK_PIVOT", "DDAMG_LINK_COMPRESSION", "DDAMG_CLOVER_COMPRESSION")
_inputs = {}


def inputs(lat):
    """gauge field and source of a lattice, made once"""
    if lat not in _inputs:
        L = LATTICES[lat][0]
        V = int(np.prod(L))
        _inputs[lat] = (synth_field(L, 5), splitmix_uniform(V * 24, 9).reshape(V, 12, 2))
    return _inputs[lat]


def context(lat, form, monkeypatch, grid=(1, 1, 1, 1)):
    """a one-level context on the lattice with the switches of the form set before it is created"""
    L, B = LATTICES[lat]
    env, reals = FORMS[form]
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    ctx = dd.Context(params(L, [B] * 4, M0, CSW, grid=grid))
    if min(grid) < 0:
        ctx.comm_init_rccl(api.rccl_unique_id())
    ctx.set_gauge(inputs(lat)[0], anti_pbc=True)
    assert ctx.link_reals() == reals
    return ctx


def fused_and_three_pass(ctx, x, prec):
    """(D^dagger x in one pass, gamma5 D gamma5 x through the entry points), downloaded"""
    a = ctx.vector(0, prec).upload(x); b = ctx.vector(0, prec); c = ctx.vector(0, prec)
    ctx.dirac_apply_dagger(b, a)
    fused = b.download()
    ctx.gamma5(c, a)          # out of place
    ctx.dirac_apply(b, c)
    ctx.gamma5(b, b)          # in place
    three = b.download()
    assert np.array_equal(a.download(), x.astype(np.float32 if prec == 32 else np.float64).astype(np.float64))   # the input is not written
    for v in (a, b, c):
        v.free()
    return fused, three


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lat,form", CASES, ids=[f"{a}-{b}" for a, b in CASES])
def test_dagger_is_the_three_pass_form_bit_for_bit(lat, form, monkeypatch):
    ctx = context(lat, form, monkeypatch)
    for prec in (32, 64):
        fused, three = fused_and_three_pass(ctx, inputs(lat)[1], prec)
        assert np.any(fused != 0) and np.array_equal(fused, three), (prec, relerr(fused, three))
    ctx.close()


@pytest.mark.parametrize("lat", ["8^4", "4x4x12x12"])
@pytest.mark.parametrize("grid", [(-1, 1, 1, 1), (1, 1, 1, -1), (-1, -1, -1, -1)], ids=["T", "X", "TZYX"])
def test_dagger_through_rccl_self_exchange(lat, grid, monkeypatch):
    """pack (with the sign), exchange, interior tiles, boundary tiles; at 4x4x12x12 the X direction has three tiles"""
    x = inputs(lat)[1]
    ctx = context(lat, "pivot", monkeypatch)
    whole = {prec: fused_and_three_pass(ctx, x, prec)[0] for prec in (32, 64)}
    ctx.close()
    ctx = context(lat, "pivot", monkeypatch, grid=grid)
    for prec, tol in ((32, 2e-6), (64, 1e-13)):
        fused, three = fused_and_three_pass(ctx, x, prec)
        assert np.array_equal(fused, three), (prec, relerr(fused, three))
        assert relerr(fused, whole[prec]) < tol          # and the operator of the undivided lattice
    ctx.close()


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lat", sorted(LATTICES))
def test_dagger_is_the_adjoint(lat, monkeypatch):
    """against the conjugate transpose of the oracle's matrix where that is small (no gamma5 code involved: this fixes the sign
    convention), against gamma5, oracle apply, gamma5 elsewhere; the bars of the operator itself"""
    L, B = LATTICES[lat]
    x = inputs(lat)[1]
    ctx = context(lat, "pivot" if B == 4 else "table", monkeypatch)
    D, cl = ctx.get_operator()
    if lat in ("4^4", "4x6x8x10"):
        ref = mo.reim((mo.fine_matrix(L, D, cl).conj().T @ mo.cplx(x).ravel()).reshape(-1, 12))
    else:
        ref = G5 * orc.dirac_apply(L, D, cl, G5 * x, 64)
    for prec, tol in ((64, 1e-13), (32, 2e-6)):
        fused, _ = fused_and_three_pass(ctx, x, prec)
        err = relerr(fused, ref)
        print(lat, prec, "relerr", err)
        assert err < tol, (prec, err)
    ctx.close()


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [32, 64])
def test_gamma5(prec, monkeypatch):
    lat = "4x6x8x10"
    ctx = context(lat, "table", monkeypatch)
    a = ctx.vector(0, prec).upload(inputs(lat)[1]); b = ctx.vector(0, prec)
    x = a.download()                                   # rounded to the precision
    ctx.gamma5(b, a)
    assert np.array_equal(b.download(), G5 * x) and np.array_equal(a.download(), x)
    ctx.gamma5(b, b)
    assert np.array_equal(b.download(), x)             # twice: the identity
    ctx.gamma5(a, a)
    assert np.array_equal(a.download(), G5 * x)        # in place
    a.free(); b.free(); ctx.close()


# 4, 5 ---------------------------------------------------------------------------------------------------------------------
def hierarchy(which, mixed_precision=1):
    """(context after its setup, lattice): two_level_4() on a synthetic field, or the 8^4 / 4^4-block hierarchy of the golden run"""
    if which == "4^4":
        q = two_level_4()
        q.post_smooth_iter[0] = 2; q.block_iter[0] = 4
        q.restart, q.max_restart, q.tol = 30, 20, 1e-10
        q.coarse_iter, q.coarse_restart, q.coarse_tol = 100, 5, 5e-2
        q.mixed_precision = mixed_precision
        ctx = dd.Context(q)
        ctx.set_gauge(synth_field([4] * 4, 2), anti_pbc=True)
        ctx.setup(2)
        return ctx, [4] * 4
    ctx = dd.Context(params_8_b4(load_golden("ref_8x8_b4.npz")))
    ctx.set_gauge(load_golden("ref_8x8_dirac.npz")["gauge"], anti_pbc=True)
    ctx.setup(3)
    return ctx, [8] * 4


def rhs(L):
    V = int(np.prod(L))
    return splitmix_uniform(V * 24, 21).reshape(V, 12, 2)


def norm(a):
    return float(np.linalg.norm(np.asarray(a).ravel()))


def vec_and_device_forms(ctx, hip, b, solve_vec, solve_device):
    """(x, the counts and relres) of the _vec and of the _device form of a solve"""
    vb = ctx.vector(0, 64).upload(b); vx = ctx.vector(0, 64)
    rv = solve_vec(vx, vb, 1e-10)
    xv = vx.download()
    vb.free(); vx.free()
    db = hip.upload(b); dx = hip.alloc(b.nbytes)
    rd = solve_device(dx, db, 1e-10)
    assert np.array_equal(hip.download(db, b.shape), b)
    return (xv, rv), (hip.download(dx, b.shape), rd)


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.free_all()


@pytest.mark.parametrize("which", ["4^4", "8^4"])
def test_solve_dagger(which, hip):
    ctx, L = hierarchy(which)
    b = rhs(L)
    x0, it0, cit0, rr0 = ctx.solve(G5 * b, 1e-10)
    hist0 = ctx.residual_history()
    x, it, cit, rr = ctx.solve_dagger(b, 1e-10)
    # (the iteration stops on its estimate of the residual, which differs from the recomputed one by rounding: twice tol is generous)
    assert rr < 2e-10 and (it, cit, rr) == (it0, cit0, rr0) and np.array_equal(ctx.residual_history(), hist0)
    assert np.array_equal(x, G5 * x0)
    for xf, counts in vec_and_device_forms(ctx, hip, b, ctx.solve_dagger_vec, ctx.solve_dagger_device):
        assert np.array_equal(xf, x) and counts == (it, cit, rr)
    if which == "4^4":
        # the reported number is the residual of D^dagger x = b, to the rounding of the product: 54 entries per row (64 taken), once
        # for the device's product and once for numpy's
        AH = mo.fine_matrix(L, *ctx.get_operator()).conj().T.tocsr()
        bc, xc = mo.cplx(b).ravel(), mo.cplx(x).ravel()
        bound = 2 * 64 * np.finfo(np.float64).eps * norm(abs(AH) @ abs(xc)) / norm(bc)
        true = norm(bc - AH @ xc) / norm(bc)
        print("relres", rr, "oracle", true, "bound", bound)
        assert abs(true - rr) <= bound
    ctx.close()


@pytest.mark.parametrize("which", ["4^4", "8^4"])
def test_solve_squared(which, hip):
    ctx, L = hierarchy(which)
    b = rhs(L)
    y, ity, city, _ = ctx.solve_dagger(b, 1e-10)
    x0, itx, citx, _ = ctx.solve(y, 1e-10)
    hist0 = ctx.residual_history()
    x, its, cits, rr = ctx.solve_squared(b, 1e-10)                 # (the first call sizes whatever the solves keep)
    assert np.array_equal(x, x0) and its == (ity, itx) and cits == (city, citx)
    assert np.array_equal(ctx.residual_history(), hist0)           # the history of the second solve
    mem = api.memory_in_use()
    x, its, cits, rr2 = ctx.solve_squared(b, 1e-10)
    assert api.memory_in_use() == mem                              # y and the residual's workspace are gone
    assert np.array_equal(x, x0) and rr2 == rr
    for xf, counts in vec_and_device_forms(ctx, hip, b, ctx.solve_squared_vec, ctx.solve_squared_device):
        assert np.array_equal(xf, x) and counts == (its, cits, rr)
    assert api.memory_in_use() == mem
    if which == "4^4":
        A = mo.fine_matrix(L, *ctx.get_operator()).tocsr(); AH = A.conj().T.tocsr()
        bc, xc = mo.cplx(b).ravel(), mo.cplx(x).ravel()
        # rounding of A x, carried through A^H, and that of the second product; device and numpy
        bound = 2 * 64 * np.finfo(np.float64).eps * (norm(abs(AH) @ (abs(A) @ abs(xc))) + norm(abs(AH) @ abs(A @ xc))) / norm(bc)
        true = norm(bc - AH @ (A @ xc)) / norm(bc)
        print("relres", rr, "oracle", true, "bound", bound)
        assert abs(true - rr) <= bound
    ctx.close()


# 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["mixed_precision_2", "method_minus_1"])
def test_solve_dagger_with_the_other_solvers(variant):
    if variant == "mixed_precision_2":
        ctx, L = hierarchy("4^4", mixed_precision=2)
    else:
        L = [4] * 4
        p = params(L, [2] * 4, 0.3, 1.0)
        p.method, p.mixed_precision, p.restart, p.max_restart, p.tol = -1, 1, 50, 20, 1e-10
        ctx = dd.Context(p)
        ctx.set_gauge(synth_field(L, 2), anti_pbc=True)
    b = rhs(L)
    x0, it0, cit0, rr0 = ctx.solve(G5 * b, 1e-10)
    hist0 = ctx.residual_history()
    x, it, cit, rr = ctx.solve_dagger(b, 1e-10)
    print(variant, "iterations", it, "relres", rr)
    assert rr < 2e-10 and (it, cit, rr) == (it0, cit0, rr0) and np.array_equal(ctx.residual_history(), hist0)
    assert np.array_equal(x, G5 * x0)
    ctx.close()


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_refusals(gold4, hip):
    q = two_level_4()
    q.m0, q.csw = float(gold4["meta_f64"][0]), float(gold4["meta_f64"][1])
    ctx = dd.Context(q)
    ctx.set_gauge(gold4["gauge"], anti_pbc=True)

    class Null:
        _h = None
    f32, f64, g64, c32 = ctx.vector(0, 32), ctx.vector(0, 64), ctx.vector(0, 64), ctx.vector(1, 32)
    vector_calls = (ctx.dirac_apply_dagger, ctx.gamma5)
    vector_solves = (ctx.solve_dagger_vec, ctx.solve_squared_vec)
    bad = [(f, (Null, f64)) for f in vector_calls + vector_solves] + [(f, (f64, Null)) for f in vector_calls + vector_solves]
    bad += [(f, (c32, c32)) for f in vector_calls + vector_solves]                # a coarse level
    bad += [(f, (f32, f64)) for f in vector_calls + vector_solves]                # mixed precisions
    bad += [(f, (f32, f32)) for f in vector_solves]                               # the solves take fp64
    bad += [(ctx.dirac_apply_dagger, (f64, f64)), (ctx.dirac_apply_dagger, (f32, f32))]   # in place
    n = 256 * 24
    host = np.zeros(n)
    d1 = hip.alloc(8 * n + 64); d2 = hip.alloc(8 * n); short = hip.alloc(8 * n) + 4 * n       # half an array behind `short`
    for f in (ctx.solve_dagger_device, ctx.solve_squared_device):
        bad += [(f, (int(host.ctypes.data), d2)), (f, (d2, int(host.ctypes.data))), (f, (0, d2)), (f, (d2, 0)),
                (f, (d1, d1)), (f, (d1 + 64, d1)), (f, (short, d2)), (f, (d2, short))]
    for f, args in bad:
        with pytest.raises(api.DDAMGError) as e:
            f(*args)
        assert str(e.value), (f.__name__, args)
    check_dirac(ctx, gold4)
    for v in (f32, f64, g64, c32):
        v.free()
    ctx.close()
