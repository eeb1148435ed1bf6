"""The store of past solutions and the guess extrapolated from it (-m gpu): ddamg_hip_chrono_*, ddamg_hip_solve_chrono_* and
ddamg_hip_solve_squared_chrono_*.  The extrapolation against numpy's least-squares optimum on the 4^4 golden operator along a mass
scan (the Gram matrix of the images has a condition of 6e5, 8e9 and 2e13 for two, three and four vectors there: normal equations would
fail, Gram-Schmidt applied twice does not); a degenerate history; exactness on a right-hand side inside the span, on a ragged lattice
too; the ring; memory; and what it is for -- the solves of a trajectory of nearby operators, D x = b and D^dagger D x = b, against the
plain solves, on one process and through the RCCL self-exchange."""
import numpy as np
import pytest
from conftest import relerr
from ddalphaamg_amd import api
import ddalphaamg_amd as dd
from oracle import orc, mg_oracle as mo
from test_gpu_device_interface import Hip, params, synth_field
import test_gpu_self_exchange as selfx

pytestmark = pytest.mark.gpu
D, DDAGGER = 0, 1
DELTA = 1e-2
L4 = [4] * 4


def norm(a):
    return float(np.linalg.norm(np.asarray(a).ravel()))


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.free_all()


_scan = {}


def mass_scan(gold4):
    """(b, the dense solutions at m0 + j DELTA for j = 0..3, the matrix at m0 + 4 DELTA) of the 4^4 golden operator, right-hand side
    all ones; made once"""
    if not _scan:
        m0, csw = float(gold4["meta_f64"][0]), float(gold4["meta_f64"][1])
        b = np.ones(12 * 256, dtype=complex)
        mats = [mo.fine_matrix(L4, *orc.gauge_to_operator(L4, gold4["gauge"], 1, m0 + j * DELTA, csw)[:2]) for j in range(5)]
        _scan["b"] = b
        _scan["x"] = [np.linalg.solve(A.toarray(), b) for A in mats[:4]]
        _scan["A"] = mats[4].tocsr()
    return _scan["b"], _scan["x"], _scan["A"]


def scan_context(gold4):
    """one level, plain GMRES: no setup; the operator at m0 + 4 DELTA"""
    m0, csw = float(gold4["meta_f64"][0]), float(gold4["meta_f64"][1])
    p = params(L4, [2] * 4, m0, csw)
    p.method, p.restart, p.max_restart = 0, 50, 20
    ctx = dd.Context(p)
    ctx.set_gauge(gold4["gauge"], anti_pbc=True)
    ctx.shift_mass(m0 + 4 * DELTA)
    return ctx


def field(z):
    """a complex vector as the [V][12][2] array of the boundary"""
    return mo.reim(np.asarray(z).reshape(-1, 12))


def optimum(A, vectors, b):
    """min_c ||b - A V c|| / ||b|| by numpy's least squares"""
    Q = np.stack([A @ v for v in vectors], axis=1)
    c = np.linalg.lstsq(Q, b, rcond=None)[0]
    return norm(b - Q @ c) / norm(b)


def guess_from(ctx, store, vectors, b, system=D):
    """reset, push the vectors in time order, guess; returns (x0 as a complex vector, kept, predicted_relres)"""
    store.reset()
    v = ctx.vector(0, 64)
    for z in vectors:
        store.push(v.upload(field(z)))
    vb = ctx.vector(0, 64).upload(field(b)); x0 = ctx.vector(0, 64)
    kept, predicted = store.guess(x0, vb, system)
    out = mo.cplx(x0.download()).ravel()
    assert np.array_equal(vb.download(), field(b))          # the right-hand side is not written
    for w in (v, vb, x0):
        w.free()
    return out, kept, predicted


# 1 ------------------------------------------------------------------------------------------------------------------------
def test_extrapolation_along_a_mass_scan_against_numpy(gold4):
    """CPU values of the optimum (classical Gram-Schmidt applied twice, fp64): 2.50e-3, 4.58e-5, 1.70e-6, 7.53e-8 for k = 1..4.  The
    excess expected from rounding is cond(Q) 2^-53 ~ 1e-11 of ||b||; the margin of 1.1 covers the order of the reductions only."""
    b, xs, A = mass_scan(gold4)
    ctx = scan_context(gold4)
    store = ctx.chrono_create(4)
    true = {}
    for k in (1, 2, 3, 4):
        x0, kept, predicted = guess_from(ctx, store, xs[4 - k:], b)
        true[k] = norm(b - A @ x0) / norm(b)
        opt = optimum(A, xs[4 - k:], b)
        print(f"k = {k}: kept {kept}, predicted {predicted:.4e}, true {true[k]:.4e}, lstsq optimum {opt:.4e}")
        assert kept == k and store.count() == k
        if k <= 3:
            assert abs(predicted - true[k]) <= 1e-6 * true[k]
            assert true[k] <= 1.1 * opt
        else:
            assert true[4] <= true[3]
    assert abs(true[1] / 2.50e-3 - 1) < 0.01 and abs(true[2] / 4.58e-5 - 1) < 0.01 and abs(true[3] / 1.70e-6 - 1) < 0.01
    store.free()
    ctx.close()


def test_a_duplicate_in_the_history_is_dropped(gold4):
    b, xs, A = mass_scan(gold4)
    ctx = scan_context(gold4)
    store = ctx.chrono_create(4)
    x0, kept, predicted = guess_from(ctx, store, [xs[3], xs[3], xs[2]], b)
    true, opt = norm(b - A @ x0) / norm(b), optimum(A, [xs[3], xs[2]], b)
    print(f"kept {kept}, predicted {predicted:.4e}, true {true:.4e}, optimum of the two distinct vectors {opt:.4e}")
    assert kept == 2 and store.count() == 3 and np.all(np.isfinite(x0)) and np.isfinite(predicted)
    assert true <= 1.1 * opt and abs(opt / 4.58e-5 - 1) < 0.01
    store.free()
    ctx.close()


# 2 ------------------------------------------------------------------------------------------------------------------------
def exactness(ctx, L, apply, system):
    """b = A (V a) for four random vectors: the guess is V a.  The CPU procedure gives a residual of 5e-16; the factor 2000 up to the
    bar is for the device's reduction order"""
    n = 12 * int(np.prod(L))
    rng = np.random.default_rng(17)
    vectors = [rng.standard_normal(n) + 1j * rng.standard_normal(n) for _ in range(4)]
    a = rng.standard_normal(4) + 1j * rng.standard_normal(4)
    xa = sum(ai * v for ai, v in zip(a, vectors))
    b = apply(xa)
    store = ctx.chrono_create(4)
    x0, kept, predicted = guess_from(ctx, store, vectors, b, system)
    true = norm(b - apply(x0)) / norm(b)
    print(f"{L}, system {system}: kept {kept}, predicted {predicted:.2e}, true {true:.2e}, x0 against V a {relerr(mo.reim(x0), mo.reim(xa)):.2e}")
    assert kept == 4 and true < 1e-12 and relerr(mo.reim(x0), mo.reim(xa)) < 1e-12
    store.free()


@pytest.mark.parametrize("system", [D, DDAGGER])
def test_a_right_hand_side_inside_the_span_is_met_exactly(gold4, system):
    A = mass_scan(gold4)[2]
    if system == DDAGGER:
        A = A.conj().T.tocsr()
    ctx = scan_context(gold4)
    exactness(ctx, L4, lambda z: A @ z, system)
    ctx.close()


def test_a_ragged_lattice():
    """192 sites: 2304 chunks of 16 bytes, nine workgroups, none of them full in the last stride"""
    L = [6, 4, 2, 4]
    ctx = dd.Context(params(L, [2] * 4, -0.1, 1.0))
    ctx.set_gauge(synth_field(L, 5), anti_pbc=True)
    Dop, cl = ctx.get_operator()
    exactness(ctx, L, lambda z: mo.cplx(orc.dirac_apply(L, Dop, cl, field(z), 64)).ravel(), D)
    ctx.close()


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_the_ring_and_the_memory(gold4):
    b, xs, A = mass_scan(gold4)
    ctx = scan_context(gold4)
    ring = ctx.chrono_create(2)
    x_ring, kept, _ = guess_from(ctx, ring, xs[1:4], b)             # three pushes into two slots
    assert ring.count() == 2 and kept == 2
    mem = api.memory_in_use()                                       # (the first guess sized what the context keeps for its reductions)
    fresh = ctx.chrono_create(2)
    assert api.memory_in_use()[0] == mem[0] + 2 * 8 * 24 * 256
    x_fresh, kept, _ = guess_from(ctx, fresh, xs[2:4], b)
    assert kept == 2 and np.array_equal(x_ring, x_fresh)
    held = api.memory_in_use()
    assert held[0] == mem[0] + (2 + 2 * 2 + 1) * 8 * 24 * 256       # the vectors, and the workspace of a guess
    assert np.array_equal(guess_from(ctx, fresh, xs[2:4], b)[0], x_fresh) and api.memory_in_use() == held
    ctx.chrono_destroy(fresh)
    assert api.memory_in_use() == mem
    ring.reset()
    assert ring.count() == 0
    x0, kept, predicted = guess_from(ctx, ring, [], b)              # an empty store: the zero guess
    assert kept == 0 and predicted == 1.0 and not np.any(x0)
    ring.free()
    assert ctx._lib.ddamg_hip_chrono_destroy(ctx._h, None) == 0      # no store: a no-op
    other = scan_context(gold4)
    mine = ctx.chrono_create(1)
    v = other.vector(0, 64)
    for call in (lambda: other.chrono_push_vec(mine, v), lambda: other.chrono_count(mine), lambda: other.chrono_reset(mine),
                 lambda: other.chrono_guess_vec(mine, v, v), lambda: other.solve_chrono_vec(mine, v, v),
                 lambda: other._lib.ddamg_hip_chrono_destroy(other._h, mine._h) and api._check(1), lambda: ctx.chrono_create(9),
                 lambda: ctx.chrono_create(0)):
        with pytest.raises(api.DDAMGError) as e:
            call()
        assert str(e.value)
    v.free(); other.close()
    mine.free()
    ctx.close()


# 4 ------------------------------------------------------------------------------------------------------------------------
_trajectory = {}


def trajectory(gold8, grid):
    """six solves of D x = 1 at m0 + j DELTA behind one setup at m0, from the store and plainly; rows of
    (count before the solve, iterations from the store, plain iterations, guess_relres, relres); made once per grid"""
    key = tuple(grid)
    if key not in _trajectory:
        p = selfx.params(gold8, grid, 2, 1)
        ctx = dd.Context(p)
        if min(grid) < 0:
            ctx.comm_init_rccl(api.rccl_unique_id())
        ctx.set_gauge(gold8["gauge"], anti_pbc=True)
        ctx.setup(2)
        b = np.zeros((4096, 12, 2)); b[..., 0] = 1.0
        vb = ctx.vector(0, 64).upload(b); vx = ctx.vector(0, 64)
        store = ctx.chrono_create(4)
        rows = []
        for j in range(6):
            ctx.shift_mass(p.m0 + j * DELTA)
            plain = ctx.solve_vec(vx, vb, 1e-10)[0]
            count = store.count()
            it, cit, rr, gr = ctx.solve_chrono_vec(store, vx, vb, 1e-10)
            rows.append((count, it, plain, gr, rr))
        print(f"grid {list(grid)}:  j  count  from the store  plain  guess_relres  relres")
        for j, (count, it, plain, gr, rr) in enumerate(rows):
            print(f"  {j}  {count}  {it:3d}  {plain:3d}  {gr:.3e}  {rr:.3e}")
        for w in (vb, vx):
            w.free()
        store.free()
        ctx.close()
        _trajectory[key] = rows
    return _trajectory[key]


def test_a_trajectory_of_solves(gold8):
    """Measured on an MI355X: see docs/design/05_host.md, 5d."""
    rows = trajectory(gold8, [1, 1, 1, 1])
    for j, (count, it, plain, gr, rr) in enumerate(rows):
        assert count == min(j, 4) and rr < 2e-10
        assert it <= plain and (j < 2 or it < plain), (j, it, plain)
    g = [r[3] for r in rows]
    assert g[0] == 1.0 and g[1] > g[2] > g[3] > g[4]


def test_a_trajectory_through_rccl_self_exchange(gold8):
    rows, whole = trajectory(gold8, [-1, -1, -1, -1]), trajectory(gold8, [1, 1, 1, 1])
    for j, (r, w) in enumerate(zip(rows, whole)):
        assert r[0] == min(j, 4) and r[4] < 2e-10
        assert abs(r[1] - w[1]) <= 1 and abs(r[2] - w[2]) <= 1, (j, r, w)


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_squared_solves_along_a_trajectory(gold8, hip):
    """D^dagger D x = 1 at four masses: both solves of the pair start from their own store.  Both results solve to 1e-10 a system
    whose condition is that of D^dagger D, a few hundred here: they agree to 1e-7
    Measured on an MI355X: see docs/design/05_host.md, 5d."""
    p = selfx.params(gold8, [1, 1, 1, 1], 2, 1)
    ctx = dd.Context(p)
    ctx.set_gauge(gold8["gauge"], anti_pbc=True)
    ctx.setup(2)
    b = np.zeros((4096, 12, 2)); b[..., 0] = 1.0
    vb = ctx.vector(0, 64).upload(b); vx = ctx.vector(0, 64)
    db = hip.upload(b); dx = hip.alloc(b.nbytes)
    hy, hx, hy_dev, hx_dev = (ctx.chrono_create(4) for _ in range(4))
    print("  j  from the stores (D^dagger, D)  plain (D^dagger, D)  relres  plain relres")
    for j in range(4):
        ctx.shift_mass(p.m0 + j * DELTA)
        its0, cits0, rr0 = ctx.solve_squared_vec(vx, vb, 1e-10)
        x_plain = vx.download()
        its, cits, rr = ctx.solve_squared_chrono_vec(hy, hx, vx, vb, 1e-10)
        x = vx.download()
        print(f"  {j}  {its}  {its0}  {rr:.3e}  {rr0:.3e}")
        assert (hy.count(), hx.count()) == (j + 1, j + 1)
        assert relerr(x, x_plain) < 1e-7
        assert its[0] <= its0[0] and its[1] <= its0[1] and (j < 2 or sum(its) < sum(its0)), (j, its, its0)
        # the _device form, from stores with the same history: the same bits
        assert ctx.solve_squared_chrono_device(hy_dev, hx_dev, dx, db, 1e-10) == (its, cits, rr)
        assert np.array_equal(hip.download(dx, b.shape), x) and np.array_equal(hip.download(db, b.shape), b)
    # no store for the D^dagger solve: that solve is the plain one, the other still starts from its store
    its1, _, rr1 = ctx.solve_squared_chrono_vec(None, hx, vx, vb, 1e-10)
    assert its1[0] == its0[0] and its1[1] <= its0[1] and relerr(vx.download(), x_plain) < 1e-7 and hx.count() == 4
    for s in (hy, hx, hy_dev, hx_dev):
        s.free()
    vb.free(); vx.free()
    ctx.close()
