"""Solves that start from the caller's vector (-m gpu): ddamg_hip_solve_guess, _vec and _device in residual-correction form.  A zero
guess is the plain solve bit for bit with every solver the library has; a converged guess costs nothing; a near guess saves iterations
and the residuals that come back are those of the system the caller posed, checked against the oracle's matrix; the same through the
RCCL self-exchange; and what is refused."""
import numpy as np
import pytest
from ddalphaamg_amd import api
import ddalphaamg_amd as dd
from oracle import mg_oracle as mo
from test_gpu_device_interface import Hip, params, two_level_4, check_dirac, synth_field
from test_gpu_dagger import hierarchy, rhs, norm
import test_gpu_self_exchange as selfx

pytestmark = pytest.mark.gpu
D, DDAGGER = 0, 1
EPS = np.finfo(np.float64).eps


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.free_all()


def one_level(method):
    """a 4^4 context without a hierarchy: CGN (-1), plain GMRES (0), or FGMRES with BiCGstab (5)"""
    L = [4] * 4
    p = params(L, [2] * 4, 0.3, 1.0)
    p.method, p.mixed_precision, p.restart, p.max_restart, p.tol = method, 1, 50, 20, 1e-10
    ctx = dd.Context(p)
    ctx.set_gauge(synth_field(L, 2), anti_pbc=True)
    if method == 5:
        ctx.setup(0)
    return ctx, L


def near_guess(x, seed=3):
    """x + 1e-6 ||x|| xi / ||xi||"""
    xi = np.random.default_rng(seed).standard_normal(x.shape)
    return x + 1e-6 * norm(x) * xi / norm(xi)


def zero_guess_is_the_plain_solve(ctx, b):
    for system, plain in ((D, ctx.solve), (DDAGGER, ctx.solve_dagger)):
        x0, it0, cit0, rr0 = plain(b, 1e-10)
        hist0 = ctx.residual_history()
        x, it, cit, rr, gr = ctx.solve_guess(np.zeros_like(b), b, 1e-10, system=system)
        print("system", system, "iterations", it, "relres", rr, "plain", rr0, "guess_relres", gr)
        assert it0 > 0 and np.array_equal(x, x0) and (it, cit) == (it0, cit0)
        assert gr == 1.0 and abs(rr - rr0) <= 1e-6 * rr0
        assert np.array_equal(ctx.residual_history(), hist0)


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["mixed_precision_1", "mixed_precision_0", "mixed_precision_2", "method_minus_1", "method_0", "method_5"])
def test_zero_guess_is_the_plain_solve_bit_for_bit(case):
    """D 0 = 0, b - 0 = b, and tol ||b|| / ||b|| = tol: no special case for a zero vector is involved"""
    kind, value = case.rsplit("_", 1)
    if kind == "mixed_precision":
        ctx, L = hierarchy("4^4", mixed_precision=int(value))
    else:
        ctx, L = one_level(-1 if case == "method_minus_1" else int(value))
    zero_guess_is_the_plain_solve(ctx, rhs(L))
    ctx.close()


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("system", [D, DDAGGER])
def test_a_converged_guess_costs_nothing(system):
    ctx, L = hierarchy("4^4")
    b = rhs(L)
    xs = (ctx.solve if system == D else ctx.solve_dagger)(b, 1e-10)[0]
    x, it, cit, rr, gr = ctx.solve_guess(xs, b, 1e-9, system=system)
    assert (it, cit) == (0, 0) and np.array_equal(x, xs) and gr == rr and 0 < rr < 1e-9
    assert len(ctx.residual_history()) == 0
    # a right-hand side of zero: the solution is zero whatever the guess
    x, it, cit, rr, gr = ctx.solve_guess(xs, np.zeros_like(b), 1e-9, system=system)
    assert (it, cit, rr, gr) == (0, 0, 0.0, 0.0) and not np.any(x)
    ctx.close()


# 3 ------------------------------------------------------------------------------------------------------------------------
def three_forms(ctx, hip, system, x0, b, tol):
    """the host form's (x, iterations, coarse iterations, relres, guess_relres), once the _vec and _device forms gave the same bits"""
    host = ctx.solve_guess(x0, b, tol, system=system)
    vx = ctx.vector(0, 64).upload(x0); vb = ctx.vector(0, 64).upload(b)
    rv = ctx.solve_guess_vec(vx, vb, tol, system=system)
    assert np.array_equal(vx.download(), host[0]) and rv == host[1:] and np.array_equal(vb.download(), b)
    vx.free(); vb.free()
    dx = hip.upload(x0); db = hip.upload(b)
    rd = ctx.solve_guess_device(dx, db, tol, system=system)
    assert np.array_equal(hip.download(dx, b.shape), host[0]) and rd == host[1:] and np.array_equal(hip.download(db, b.shape), b)
    return host


@pytest.mark.parametrize("system", [D, DDAGGER])
@pytest.mark.parametrize("which", ["4^4", "8^4"])
def test_a_near_guess(which, system, hip):
    """the guess starts about five of the ten decades down, so the correction solve must need fewer iterations.  Measured on an MI355X:
    4^4, 3 (D) and 4 (D^dagger) iterations where the plain solves take 8; 8^4, 6 where they take 15; guess_relres 1.3e-6 to 1.6e-6"""
    ctx, L = hierarchy(which)
    b = rhs(L)
    xs, it_plain, _, _ = (ctx.solve if system == D else ctx.solve_dagger)(b, 1e-10)
    x0 = near_guess(xs)
    x, it, cit, rr, gr = three_forms(ctx, hip, system, x0, b, 1e-10)
    print(which, "system", system, "plain", it_plain, "from the guess", it, "guess_relres", gr, "relres", rr)
    # (the iteration stops on its estimate of the residual, which differs from the recomputed one by rounding: twice tol, as for
    # the plain D^dagger solve)
    assert rr < 2e-10 and 0 < it < it_plain and rr < gr < 1e-3
    if which == "4^4":
        # both reported numbers are residuals of the system posed, relative to b, to the rounding of the product: 54 entries per
        # row (64 taken), once for the device's product and once for numpy's
        A = mo.fine_matrix(L, *ctx.get_operator()).tocsr()
        if system == DDAGGER:
            A = A.conj().T.tocsr()
        bc = mo.cplx(b).ravel()
        for name, v, reported in (("relres", x, rr), ("guess_relres", x0, gr)):
            vc = mo.cplx(v).ravel()
            bound = 2 * 64 * EPS * norm(abs(A) @ abs(vc)) / norm(bc)
            true = norm(bc - A @ vc) / norm(bc)
            print(name, reported, "oracle", true, "bound", bound)
            assert abs(true - reported) <= bound
    ctx.close()


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_through_rccl_self_exchange(gold8, hip):
    """the fp64 operator's halo exchange and the global sums of the one-pass residual, the process its own neighbour"""
    ctx = dd.Context(selfx.params(gold8, [-1] * 4, 2, 1))
    ctx.comm_init_rccl(api.rccl_unique_id())
    ctx.set_gauge(gold8["gauge"], anti_pbc=True)
    ctx.setup(2)
    b = rhs([8] * 4)
    zero_guess_is_the_plain_solve(ctx, b)
    xs, it_plain, _, _ = ctx.solve(b, 1e-10)
    x, it, cit, rr, gr = three_forms(ctx, hip, D, near_guess(xs), b, 1e-10)
    print("plain", it_plain, "from the guess", it, "guess_relres", gr, "relres", rr)
    assert rr < 2e-10 and 0 < it < it_plain and rr < gr < 1e-3
    ctx.close()


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_refusals(gold4, hip):
    q = two_level_4()
    q.post_smooth_iter[0] = 2; q.block_iter[0] = 4
    q.restart, q.max_restart, q.tol = 30, 20, 1e-10
    q.coarse_iter, q.coarse_restart, q.coarse_tol = 100, 5, 5e-2
    q.m0, q.csw = float(gold4["meta_f64"][0]), float(gold4["meta_f64"][1])
    ctx = dd.Context(q)
    ctx.set_gauge(gold4["gauge"], anti_pbc=True)

    class Null:
        _h = None
    n = 256 * 24
    b = rhs([4] * 4)
    f32, f64, g64, c32 = ctx.vector(0, 32), ctx.vector(0, 64).upload(np.zeros_like(b)), ctx.vector(0, 64).upload(b), ctx.vector(1, 32)
    host = np.zeros(n)
    d1 = hip.alloc(8 * n + 64); d2 = hip.alloc(8 * n); short = hip.alloc(8 * n) + 4 * n        # half an array behind `short`
    vec, dev = ctx.solve_guess_vec, ctx.solve_guess_device
    bad = [(vec, (f64, g64), {}), (dev, (d1, d2), {}), (ctx.solve_guess, (np.zeros_like(b), b), {})]      # before the setup
    for f, args, kw in bad:
        with pytest.raises(api.DDAMGError) as e:
            f(*args, **kw)
        assert "setup" in str(e.value), (f.__name__, args)
    ctx.setup(2)
    bad = [(vec, (Null, g64), {}), (vec, (f64, Null), {})]                                    # a null argument
    bad += [(vec, (c32, c32), {}), (vec, (f32, f32), {}), (vec, (f32, g64), {}), (vec, (f64, f32), {})]   # a coarse or fp32 vector
    bad += [(vec, (f64, f64), {})]                                                            # the guess is the right-hand side
    bad += [(vec, (f64, g64), {"system": 2}), (dev, (d1, d2), {"system": 2}), (dev, (d1, d2), {"system": -1}),
            (ctx.solve_guess, (np.zeros_like(b), b), {"system": 2})]
    bad += [(dev, (int(host.ctypes.data), d2), {}), (dev, (d2, int(host.ctypes.data)), {}), (dev, (0, d2), {}), (dev, (d2, 0), {}),
            (dev, (d1, d1), {}), (dev, (d1 + 64, d1), {}), (dev, (short, d2), {}), (dev, (d2, short), {})]
    for f, args, kw in bad:
        with pytest.raises(api.DDAMGError) as e:
            f(*args, **kw)
        assert str(e.value), (f.__name__, args, kw)
    check_dirac(ctx, gold4)
    it, cit, rr, gr = vec(f64, g64, 1e-10)                     # the context still solves
    assert it > 0 and gr == 1.0 and rr < 2e-10 and np.array_equal(g64.download(), b)
    for v in (f32, f64, g64, c32):
        v.free()
    ctx.close()
