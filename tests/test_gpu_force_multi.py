"""The fermion force of many pairs in one pass (-m gpu): ddamg_hip_force_bilinear_multi_vec / _device and
ddamg_hip_force_rational_device against the numpy restatement tests/force_reference.py, against the loop of single calls they
replace, and against finite differences of the rational action through the library's own multi-shift solve.

Lattices: those of test_gpu_force.py (4^4, 4x6x8x10, 8^4, 4x4x12x12) and 4x4x6x6 with 2^4 blocks, whose 576 sites leave the last
workgroup of 128 half filled; every other lattice has a multiple of 128 sites and cannot show a wrong tail.  Pairs: their own
splitmix_uniform seeds, weights of mixed sign and magnitude.  Pair counts in units of the group G = api.FORCE_GROUP: 1, G (one full
launch in the write form), G + 1 (a second launch in the add form with one pair), 2 G + 1, and 32, the most the call takes.

Bars.  Against the reference: 1e-13 of the reference's norm, the project's fp64 bar, as for the single call.  Against the loop of
single calls: 2e-13, since both lie within 1e-13 of one reference; equal bits are not promised (the compiler fuses kernel by kernel).
Finite differences: the rule of test_gpu_multishift.test_the_rational_force, ten times the larger of the Richardson spread and
FTOL |S| / H.
Measured on the MI355X: against the reference 2.7e-16 (one pair) to 3.9e-16 (32 pairs); against the loop of single calls 2.6e-16 and
3.6e-16, one pair of weight one against the single call 9.7e-17 (not zero: the kernels differ); the cancelled pair 1.9e-16 of its
force; the rational form against the recipe loop 2.3e-16; finite differences: S = 52.0, derivative -0.7392, spread 6.5e-7,
FTOL |S| / H = 1.3e-8, difference 4.4e-8.  Times: docs/design/04_kernels.md, "Fermion force"."""
import numpy as np
import pytest
from conftest import relerr, splitmix_uniform
from ddalphaamg_amd import api
import ddalphaamg_amd as dd
import eo_reference as eo
import force_reference as fr
from test_gpu_device_interface import Hip, params, synth_field
from test_gpu_dagger import LATTICES, SWITCHES, M0, rhs
import test_gpu_force as tf

pytestmark = pytest.mark.gpu
G = api.FORCE_GROUP
EXTRA = {"4x4x6x6": ([4, 4, 6, 6], 2)}
LATS = tf.LATS + ["4x4x6x6"]
WEIGHTS = [0.3, -1.1, 2.5, -0.04, 7.0, 1.0, -3.2, 0.6]
_pairs, _refs = {}, {}


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.free_all()


def lattice(lat):
    return LATTICES[lat] if lat in LATTICES else EXTRA[lat]


def links(lat):
    return tf.fields(lat)[0] if lat in LATTICES else synth_field(lattice(lat)[0], 5)


def context(lat, monkeypatch, csw=1.0, grid=(1, 1, 1, 1)):
    if lat in LATTICES:
        return tf.context(lat, "pivot" if LATTICES[lat][1] == 4 else "table", monkeypatch, csw, grid=grid)
    L, B = EXTRA[lat]
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    ctx = dd.Context(params(L, [B] * 4, M0, csw, grid=grid))
    if min(grid) < 0:
        ctx.comm_init_rccl(api.rccl_unique_id())
    ctx.set_gauge(links(lat), anti_pbc=True)
    return ctx


def weight(s):
    return WEIGHTS[s % len(WEIGHTS)] * (1.0 + s // len(WEIGHTS))


def pair(lat, s):
    """(Y_s, X_s) of a lattice, made once and never changed"""
    if (lat, s) not in _pairs:
        V = int(np.prod(lattice(lat)[0]))
        p = tuple(splitmix_uniform(V * 24, 100 + 2 * s + k).reshape(V, 12, 2) for k in (0, 1))
        for a in p:
            a.setflags(write=False)
        _pairs[(lat, s)] = p
    return _pairs[(lat, s)]


def reference(lat, csw, s):
    """the reference force of pair s, computed once"""
    if (lat, csw, s) not in _refs:
        Y, X = pair(lat, s)
        f = fr.force_bilinear(lattice(lat)[0], links(lat), 1, M0, csw, Y, X)
        f.setflags(write=False)
        _refs[(lat, csw, s)] = f
    return _refs[(lat, csw, s)]


def reference_sum(lat, csw, n):
    return sum(weight(s) * reference(lat, csw, s) for s in range(n))


def nbytes(lat):
    return int(np.prod(lattice(lat)[0])) * 72 * 8


def guarded(hip, lat, fill=None):
    """an output array with 64 sentinel reals on either side: (base, the array's address, check())"""
    n = nbytes(lat) // 8
    host = np.full(n + 128, -3.25e200)
    if fill is not None:
        host[64:-64] = fill.ravel()
    base = hip.upload(host)

    def check():
        back = hip.download(base, (n + 128,))
        assert np.all(back[:64] == -3.25e200) and np.all(back[-64:] == -3.25e200), "the sentinels around force_dev were written"
    return base + 64 * 8, check


def shape(lat):
    return (int(np.prod(lattice(lat)[0])), 4, 9, 2)


def multi_vec(ctx, hip, lat, n, coeff=1.0, accumulate=False, out=None, weights=None, pairs=None):
    pairs = [pair(lat, s) for s in range(n)] if pairs is None else pairs
    weights = [weight(s) for s in range(n)] if weights is None else weights
    ys = [ctx.vector(0, 64).upload(p[0]) for p in pairs]; xs = [ctx.vector(0, 64).upload(p[1]) for p in pairs]
    out = hip.alloc(nbytes(lat)) if out is None else out
    assert ctx.force_bilinear_multi_vec(out, ys, xs, weights, coeff, accumulate) == out
    for v, p in zip(ys + xs, [p[0] for p in pairs] + [p[1] for p in pairs]):
        assert np.array_equal(v.download(), p)
        v.free()
    return hip.download(out, shape(lat))


def multi_device(ctx, hip, lat, n, coeff=1.0, accumulate=False, out=None):
    pairs = [pair(lat, s) for s in range(n)]
    dy = [hip.upload(p[0]) for p in pairs]; dx = [hip.upload(p[1]) for p in pairs]
    out = hip.alloc(nbytes(lat)) if out is None else out
    assert ctx.force_bilinear_multi_device(out, dy, dx, [weight(s) for s in range(n)], coeff, accumulate) == out
    for d, p in zip(dy + dx, [p[0] for p in pairs] + [p[1] for p in pairs]):
        assert np.array_equal(hip.download(d, p.shape), p)
    return hip.download(out, shape(lat))


def loop_of_single_calls(ctx, hip, lat, n, coeff=1.0):
    out = hip.alloc(nbytes(lat))
    for s in range(n):
        Y, X = pair(lat, s)
        vy = ctx.vector(0, 64).upload(Y); vx = ctx.vector(0, 64).upload(X)
        ctx.force_bilinear_vec(out, vy, vx, coeff * weight(s), accumulate=s > 0)
        vy.free(); vx.free()
    return hip.download(out, shape(lat))


# 1 ------------------------------------------------------------------------------------------------------------------------
CASES = [(lat, 1.0, n) for lat in LATS for n in (1, G, G + 1)] + [(lat, csw, 2 * G + 1) for lat in ("8^4", "4x4x6x6") for csw in (0.0, 1.0)] \
    + [("4^4", 1.0, 32)]


@pytest.mark.parametrize("lat,csw,n", CASES, ids=[f"{a}-csw{b:g}-n{c}" for a, b, c in CASES])
def test_against_the_reference(lat, csw, n, monkeypatch, hip):
    ctx = context(lat, monkeypatch, csw)
    ref = reference_sum(lat, csw, n)
    out, check = guarded(hip, lat)
    got = multi_vec(ctx, hip, lat, n, out=out)
    check()
    err = relerr(got, ref)
    print(lat, "csw", csw, "pairs", n, "norm", np.linalg.norm(ref), "relerr", err)
    assert err < 1e-13
    out, check = guarded(hip, lat)
    assert np.array_equal(multi_device(ctx, hip, lat, n, out=out), got)      # the same bits from both entry points
    check()
    assert np.array_equal(multi_vec(ctx, hip, lat, n), got)                  # ... and from two calls
    ctx.close()


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lat", LATS)
def test_against_the_loop_of_single_calls(lat, monkeypatch, hip):
    ctx = context(lat, monkeypatch, 1.0)
    for n in (1, G + 1):
        loop = loop_of_single_calls(ctx, hip, lat, n, coeff=-2.0)
        got = multi_vec(ctx, hip, lat, n, coeff=-2.0)
        err = relerr(got, loop)
        print(lat, "pairs", n, "against the loop", err)
        assert err < 2e-13
    # one pair of weight one against the single call
    Y, X = pair(lat, 0)
    single = tf.by_vec(ctx, hip, lat, Y, X) if lat in LATTICES else None
    if single is None:
        vy = ctx.vector(0, 64).upload(Y); vx = ctx.vector(0, 64).upload(X); out = hip.alloc(nbytes(lat))
        ctx.force_bilinear_vec(out, vy, vx)
        single = hip.download(out, shape(lat))
        vy.free(); vx.free()
    one = multi_vec(ctx, hip, lat, 1, weights=[1.0])
    print(lat, "one pair of weight one against the single call", relerr(one, single))
    assert relerr(one, single) < 2e-13
    ctx.close()


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_coeff_accumulate_and_repeated_inputs(monkeypatch, hip):
    lat = "4x4x6x6"
    ctx = context(lat, monkeypatch, 1.0)
    n = G + 1
    f = multi_vec(ctx, hip, lat, n)
    norm = np.linalg.norm(f)
    assert relerr(multi_vec(ctx, hip, lat, n, coeff=-2.0), -2.0 * f) < 1e-13
    start = splitmix_uniform(f.size, 12).reshape(f.shape)
    out, check = guarded(hip, lat, start)
    got = multi_vec(ctx, hip, lat, n, coeff=0.7, accumulate=True, out=out)
    check()
    assert relerr(got, start + 0.7 * f) < 1e-13
    got = multi_device(ctx, hip, lat, 1, coeff=-1.5, accumulate=True, out=out)
    assert relerr(got, start + 0.7 * f - 1.5 * weight(0) * reference("4x4x6x6", 1.0, 0)) < 1e-13
    # coeff = 0 onto a field leaves its bits
    out, check = guarded(hip, lat, start)
    assert np.array_equal(multi_vec(ctx, hip, lat, n, coeff=0.0, accumulate=True, out=out), start)
    check()
    # a repeated pair with weights w and -w cancels to within the bar, measured against the force of the pair alone
    p0, p1 = pair(lat, 0), pair(lat, 1)
    alone = np.linalg.norm(multi_vec(ctx, hip, lat, 1, weights=[2.5]))
    cancelled = multi_vec(ctx, hip, lat, 3, weights=[2.5, 0.6, -2.5], pairs=[p0, p1, p0])
    rest = multi_vec(ctx, hip, lat, 1, weights=[0.6], pairs=[p1])
    print("cancellation", np.linalg.norm(cancelled - rest) / alone)
    assert np.linalg.norm(cancelled - rest) <= 1e-13 * alone
    # the same vector as x of two pairs: the very same Vector objects, twice in the lists
    ys = [ctx.vector(0, 64).upload(p0[0]), ctx.vector(0, 64).upload(p1[0])]; x = ctx.vector(0, 64).upload(p0[1])
    out = hip.alloc(nbytes(lat))
    ctx.force_bilinear_multi_vec(out, ys, [x, x], [0.3, -1.1])
    want = 0.3 * reference(lat, 1.0, 0) - 1.1 * fr.force_bilinear(lattice(lat)[0], links(lat), 1, M0, 1.0, p1[0], p0[1])
    assert relerr(hip.download(out, shape(lat)), want) < 1e-13
    for v in ys + [x]:
        v.free()
    assert norm > 1.0
    ctx.close()


# 4 ------------------------------------------------------------------------------------------------------------------------
SHIFTS, RHO = [0.05, 0.7, 9.0], [0.3, 1.1, 2.5]


def recipe_loop(ctx, hip, L, dxe, dxo, rho, coeff):
    """the per-shift recipe of INTEGRATION.md made of the calls that exist without the rational entry point"""
    V = int(np.prod(L)); half = V * 12 * 8
    dye, dyo = hip.alloc(half), hip.alloc(half)
    out = hip.alloc(V * 72 * 8)
    vx = ctx.vector(0, 64); vy = ctx.vector(0, 64)
    for s in range(len(rho)):
        ctx.schur_apply_device(dye, dxe[s])
        ctx.schur_odd_part_device(dyo, dye, dagger=True)
        ctx.vec_upload_parity_device(vx, 0, dxe[s]); ctx.vec_upload_parity_device(vx, 1, dxo[s], zero_other=False)
        ctx.vec_upload_parity_device(vy, 0, dye); ctx.vec_upload_parity_device(vy, 1, dyo, zero_other=False)
        ctx.force_bilinear_vec(out, vy, vx, coeff * rho[s], accumulate=s > 0)
    vx.free(); vy.free()
    return hip.download(out, (V, 4, 9, 2))


@pytest.mark.parametrize("lat", ["4^4", "4x4x6x6"])
def test_rational_force_against_the_recipe(lat, monkeypatch, hip):
    L = lattice(lat)[0]
    V = int(np.prod(L))
    ctx = context(lat, monkeypatch, 1.0)
    odd = eo.parity(L) == 1
    phi = np.ascontiguousarray(rhs(L)[~odd])
    dphi = hip.upload(phi)
    dxe = [hip.alloc(phi.nbytes) for _ in SHIFTS]; dxo = [hip.alloc(phi.nbytes) for _ in SHIFTS]
    ctx.solve_schur_multishift_device(SHIFTS, dxe, dxo, dphi, [1e-12] * 3)
    xe0 = [hip.download(p, phi.shape) for p in dxe]; xo0 = [hip.download(p, phi.shape) for p in dxo]
    loop = recipe_loop(ctx, hip, L, dxe, dxo, RHO, -2.0)
    out, check = guarded(hip, lat)
    ctx.force_rational_device(out, RHO, dxe, dxo, -2.0)
    given = hip.download(out, (V, 4, 9, 2))
    check()
    err = relerr(given, loop)
    print(lat, "rational force: norm", np.linalg.norm(loop), "against the recipe loop", err)
    assert err < 2e-13
    # the odd part computed inside is the odd part of the solve: the same bits with None, and with one entry None
    ctx.force_rational_device(out, RHO, dxe, None, -2.0)
    assert np.array_equal(hip.download(out, (V, 4, 9, 2)), given)
    ctx.force_rational_device(out, RHO, dxe, [dxo[0], None, dxo[2]], -2.0)
    assert np.array_equal(hip.download(out, (V, 4, 9, 2)), given)
    check()
    for p, a in zip(dxe + dxo, xe0 + xo0):
        assert np.array_equal(hip.download(p, phi.shape), a)          # the inputs are unchanged
    # accumulate
    start = splitmix_uniform(given.size, 13).reshape(given.shape)
    acc = hip.upload(start)
    ctx.force_rational_device(acc, RHO, dxe, dxo, 0.5, accumulate=True)
    assert relerr(hip.download(acc, given.shape), start - 0.25 * given) < 1e-13
    ctx.close()


def test_the_rational_force_against_finite_differences(monkeypatch, hip):
    """test_gpu_multishift.test_the_rational_force with force_rational_device in place of the loop: the same bar, formula and case"""
    FTOL = 1e-12
    H = 2.0 ** -8
    lat = "4^4"
    L = lattice(lat)[0]
    V = int(np.prod(L))
    ctx = context(lat, monkeypatch, tf.CSW)
    U = links(lat)
    odd = eo.parity(L) == 1
    phi = np.ascontiguousarray(rhs(L)[~odd])
    shifts, rho = [0.05, 0.7, 9.0], [0.3, 1.1, 2.5]
    omega = fr.random_algebra(np.random.default_rng(33), (V, 4))
    dphi = hip.upload(phi)
    dxe = [hip.alloc(phi.nbytes) for _ in shifts]; dxo = [hip.alloc(phi.nbytes) for _ in shifts]

    def S(eps):
        ctx.set_gauge_device(hip.upload(fr.perturbed(U, omega, eps)), anti_pbc=True)
        ctx.solve_schur_multishift_device(shifts, dxe, None, dphi, [FTOL] * 3)
        return float(sum(r * np.sum(phi * hip.download(p, phi.shape)) for r, p in zip(rho, dxe)))
    fine, coarse = fr.richardson(S, H), fr.richardson(S, 2 * H)
    s0 = S(0.0)
    its, rr, _ = ctx.solve_schur_multishift_device(shifts, dxe, dxo, dphi, [FTOL] * 3)
    out = hip.alloc(V * 72 * 8)
    ctx.force_rational_device(out, rho, dxe, dxo, -2.0)
    mine = fr.pairing(omega, hip.download(out, (V, 4, 9, 2)))
    spread, solve = abs(fine - coarse), FTOL * abs(s0) / H
    print(f"S {s0:.12e} derivative {fine:+.12e} force {mine:+.12e} spread {spread:.2e} solve {solve:.2e} difference {abs(mine - fine):.2e}", its, rr)
    assert abs(fine) > 1e-3 and abs(mine - fine) <= 10 * max(spread, solve)
    ctx.close()


# 6 ------------------------------------------------------------------------------------------------------------------------
def refused(call, *words):
    with pytest.raises(api.DDAMGError) as e:
        call()
    assert all(w in str(e.value) for w in words), str(e.value)


def test_refusals(monkeypatch, hip):
    lat = "4^4"
    L = lattice(lat)[0]
    V = int(np.prod(L))
    ctx = context(lat, monkeypatch, 1.0)
    Y, X = pair(lat, 0)
    out = hip.alloc(nbytes(lat)); dy = hip.upload(Y); dx = hip.upload(X)
    vy = ctx.vector(0, 64).upload(Y); vx = ctx.vector(0, 64).upload(X); v32 = ctx.vector(0, 32)
    half = hip.upload(np.ascontiguousarray(X[:V // 2]))
    inf, nan = float("inf"), float("nan")
    # the count
    refused(lambda: ctx.force_bilinear_multi_vec(out, [], [], []), "npairs = 0", "DDAMG_HIP_MAX_FORCE_PAIRS")
    refused(lambda: ctx.force_bilinear_multi_vec(out, [vy] * 33, [vx] * 33, [1.0] * 33), "npairs = 33", "DDAMG_HIP_MAX_FORCE_PAIRS")
    refused(lambda: ctx.force_bilinear_multi_device(out, [], [], []), "npairs = 0")
    refused(lambda: ctx.force_bilinear_multi_device(out, [dy] * 33, [dx] * 33, [1.0] * 33), "npairs = 33")
    refused(lambda: ctx.force_rational_device(out, [], []), "nshift = 0")
    refused(lambda: ctx.force_rational_device(out, [1.0] * 33, [half] * 33), "nshift = 33")
    # null arrays and entries
    lib = ctx._lib
    assert lib.ddamg_hip_force_bilinear_multi_vec(ctx._h, api._dev(out, V * 72, "t"), 1, None, None, None, 1.0, 0) != 0
    assert b"null argument" in lib.ddamg_hip_last_error()
    assert lib.ddamg_hip_force_rational_device(ctx._h, api._dev(out, V * 72, "t"), 1, None, None, None, 1.0, 0) != 0
    assert b"null argument" in lib.ddamg_hip_last_error()
    refused(lambda: ctx.force_bilinear_multi_vec(out, [vy, None], [vx, vx], [1.0, 1.0]), "null argument", "vector 1")
    refused(lambda: ctx.force_bilinear_multi_device(out, [dy, dy], [dx, None], [1.0, 1.0]), "null argument", "array 1")
    refused(lambda: ctx.force_rational_device(out, [1.0, 1.0], [half, None]), "null argument", "x_e_dev[1]")
    refused(lambda: ctx.force_bilinear_multi_vec(0, [vy], [vx], [1.0]), "null")
    # weights
    refused(lambda: ctx.force_bilinear_multi_vec(out, [vy, vy], [vx, vx], [1.0, nan]), "weight 1 is not finite")
    refused(lambda: ctx.force_bilinear_multi_device(out, [dy], [dx], [inf]), "weight 0 is not finite")
    refused(lambda: ctx.force_rational_device(out, [0.5, -inf], [half, half]), "weight 1 is not finite")
    # vectors and pointers
    refused(lambda: ctx.force_bilinear_multi_vec(out, [vy, v32], [vx, vx], [1.0, 1.0]), "fp32")
    host = np.zeros(V * 72)
    refused(lambda: ctx.force_bilinear_multi_device(out, [dy], [int(host.ctypes.data)], [1.0]), "not a pointer into device memory")
    refused(lambda: ctx.force_rational_device(int(host.ctypes.data), [1.0], [half]), "not a pointer into device memory")
    # overlap with force_dev: the second pair's array, so that every entry is looked at
    refused(lambda: ctx.force_bilinear_multi_device(out, [dy, dy], [dx, out + 8 * 24], [1.0, 1.0]), "overlap")
    refused(lambda: ctx.force_bilinear_multi_device(out, [dy, out], [dx, dx], [1.0, 1.0]), "overlap")
    refused(lambda: ctx.force_rational_device(out, [1.0, 1.0], [half, out + 64]), "overlap")
    refused(lambda: ctx.force_rational_device(out, [1.0, 1.0], [half, half], [None, out + 8 * 24]), "overlap")          # x_o_dev inside force_dev
    # operators with no single link field behind them
    ctx.set_operator(*ctx.get_operator())
    refused(lambda: ctx.force_bilinear_multi_vec(out, [vy], [vx], [1.0]), "did not come from one link field")
    refused(lambda: ctx.force_rational_device(out, [1.0], [half]), "did not come from one link field")
    for v in (vy, vx, v32):
        v.free()
    ctx.close()
    # (a process grid: tests/test_gpu_force_multi_grid.py, where the plain forms refuse and name their twins)
    # odd local extents (rational form)
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    Lo = [4, 4, 2, 3]       # refused before anything touches the operator, so none is needed
    ctx = dd.Context(params(Lo, Lo, M0, 1.0))
    out = hip.alloc(96 * 72 * 8); half = hip.upload(np.zeros(48 * 24))
    refused(lambda: ctx.force_rational_device(out, [1.0], [half]), "even local lattice extents")
    ctx.close()
