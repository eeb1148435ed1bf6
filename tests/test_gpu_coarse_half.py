"""GPU tests (-m gpu) of the coarsest level's couplings in 16-bit storage (ddamg_hip_set_coarse_storage, coarse_half.h):
the two kernels against a bound derived from the number formats, the coarsest solve and the whole solve in both storages, the
copy following the operator, the setup staying on the 32-bit couplings, memory accounting and the refusals.

The bound.  An element is stored as fp16(a / s), s the largest |re| or |im| of its matrix: a normal fp16 result is within 2^-11
relative, a subnormal one within 2^-25 s absolute.  Products are accumulated in fp32 over at most 9 * 64 terms in either storage
(9 * 64 * 2^-24 < 2^-14), which the factor 2 on both terms covers.  Component by component, with the sums over the self coupling
and the eight couplings of the site (matrix m, scale s_m):
    B_i = 2^-10 sum_j (|Re a_ij| + |Im a_ij|)(|Re x_j| + |Im x_j|) + 2^-23 sum_m s_m sum_{j in m} (|Re x_j| + |Im x_j|)"""
import numpy as np
import pytest
from conftest import load_golden, splitmix_uniform
from coarse_reference import CoarseMatrices
from ddalphaamg_amd import api
import ddalphaamg_amd as dd

pytestmark = pytest.mark.gpu

COARSE_TOL = 5e-2


def two_level_params(L, Lc, num_vect, m0, csw, mixed_precision=1, odd_even=1, setup_iter=4):
    p = api.default_params()
    p.num_levels = 2
    for mu in range(4):
        p.local_lattice[0][mu] = L; p.block_lattice[0][mu] = 2; p.local_lattice[1][mu] = Lc
    p.num_vect[0] = num_vect
    p.post_smooth_iter[0] = 2; p.block_iter[0] = 4; p.setup_iter[0] = setup_iter
    p.restart, p.max_restart, p.tol = 50, 20, 1e-10
    p.coarse_iter, p.coarse_restart, p.coarse_tol = 100, 5, COARSE_TOL
    p.mixed_precision, p.method, p.odd_even = mixed_precision, 2, odd_even
    p.m0, p.csw = m0, csw
    return p


def inputs(ctx):
    V, n = ctx.volume(1), ctx.ndof(1)
    unit = np.zeros((V, n, 2)); unit[V - 1, n - 1, 0] = 1.0
    return {"random": splitmix_uniform(V * n * 2, 4242).reshape(V, n, 2), "unit": unit}


def ctx_a(gold4, **kw):
    """(a) 4^4 golden configuration, 2^4 aggregates, the reference's 20 interpolation vectors: coarse lattice 2^4, n = 40, the
    forward and the backward neighbour of a site are the same site"""
    ctx = dd.Context(two_level_params(4, 2, 20, float(gold4["meta_f64"][0]), float(gold4["meta_f64"][1]), **kw))
    ctx.set_operator(gold4["D"], gold4["clover"])
    ctx.set_test_vectors(gold4["interp_vectors"], orthonormalised=True)
    return ctx


def with_first_apply(ctx):
    """the context and its coarse apply of inputs(ctx) as a fresh context gives it: before any call of set_coarse_storage"""
    vi = ctx.vector(1, 32); vo = ctx.vector(1, 32)
    first = {k: (vi.upload(x), ctx.coarse_apply(vo, vi), vo.download())[2] for k, x in inputs(ctx).items()}
    vi.free(); vo.free()
    return ctx, first


@pytest.fixture(scope="module")
def hier_a(gold4):
    ctx = ctx_a(gold4)
    yield with_first_apply(ctx)
    ctx.close()


@pytest.fixture(scope="module")
def hier_b(gold4):
    """(b) the same lattice with 10 test vectors from a one-iteration setup: n = 20, rows and columns 20..23 of every tile row are padding"""
    ctx = dd.Context(two_level_params(4, 2, 10, float(gold4["meta_f64"][0]), float(gold4["meta_f64"][1])))
    ctx.set_operator(gold4["D"], gold4["clover"])
    ctx.setup(1)
    yield with_first_apply(ctx)
    ctx.close()


@pytest.fixture(scope="module")
def hier_c(gold8):
    """(c) the 8^4 configuration, 2^4 aggregates, 20 test vectors from a one-iteration setup: coarse lattice 4^4, eight distinct neighbours"""
    ctx = dd.Context(two_level_params(8, 4, 20, float(gold8["meta_f64"][0]), float(gold8["meta_f64"][1])))
    ctx.set_gauge(gold8["gauge"], anti_pbc=True)
    ctx.setup(1)
    yield with_first_apply(ctx)
    ctx.close()


@pytest.fixture(params=["a", "b", "c"])
def hier(request):
    return request.getfixturevalue("hier_" + request.param)


def applies(ctx, xs, bits):
    """coarse_apply of every input with the storage set to `bits` (and left there)"""
    ctx.set_coarse_storage(bits)
    vi = ctx.vector(1, 32); vo = ctx.vector(1, 32)
    out = {k: (vi.upload(x), ctx.coarse_apply(vo, vi), vo.download())[2] for k, x in xs.items()}
    vi.free(); vo.free()
    return out


def assert_within_bound(y16, y32, B, what):
    d = np.abs(y16 - y32).max(axis=-1)
    worst = float((d / np.where(B > 0, B, 1.0)).max())
    print(f"{what}: max |y16 - y32| = {d.max():.3e}, largest |y16 - y32| / B = {worst:.3f}")
    assert np.all(d <= B), what


# ---- 1. the kernels against the bound ------------------------------------------------------------------------------------
def test_apply_in_16_bit_storage_is_within_the_format_bound(hier):
    ctx, y32 = hier                  # y32: from before any switch
    xs = inputs(ctx)
    y16 = applies(ctx, xs, 16)
    y32_again = applies(ctx, xs, 32)
    cm = CoarseMatrices(ctx)
    for k, x in xs.items():
        ref = cm.apply(x)
        assert np.abs(y32[k] - ref).max() <= 1e-5 * np.abs(ref).max()          # the numpy operator is the one on the device
        assert_within_bound(y16[k], y32[k], cm.bound(x), k)
        assert not np.array_equal(y16[k], y32[k])                              # the 16-bit path was taken
        assert np.array_equal(y32_again[k], y32[k])                            # 32 bits again: the parent's kernel, bit for bit


def test_half_hopping_term_and_self_mul_by_parity(hier_c):
    """ddamg_hip_coarse_hop / ddamg_hip_coarse_self_mul, the products the Schur complement is made of, in both storages against the
    downloaded operator in fp64: site range, sign and accumulation of the hopping term, M0 and its inverse.  16-bit storage
    within the bound of the hopping terms; 32-bit storage within 1e-5 of the largest component (fp32 sums of 8 * 40 terms)"""
    ctx, _ = hier_c
    cm = CoarseMatrices(ctx)
    V, n = cm.V, cm.n
    x = inputs(ctx)["random"]; o = np.float32(splitmix_uniform(V * n * 2, 99).reshape(V, n, 2)).astype(np.float64)
    xc = x[..., 0] + 1j * x[..., 1]
    odd = np.stack(np.unravel_index(np.arange(V), [4, 4, 4, 4]), axis=1).sum(axis=1) % 2 == 1
    hop = sum(np.einsum("xij,xj->xi", M, xc[src]) for M, src in zip(cm.mats[1:], cm.src[1:]))
    hop = np.stack([hop.real, hop.imag], axis=-1)
    vi = ctx.vector(1, 32).upload(x); vo = ctx.vector(1, 32); t = ctx.vector(1, 32)
    got = {}
    for bits in (32, 16):
        ctx.set_coarse_storage(bits)
        tol = cm.bound(x, first=1)[..., None] + 2.0 ** -22 * np.abs(o - hop) if bits == 16 else np.full((V, n, 1), 1e-5 * np.abs(hop).max())
        vo.upload(o); ctx.coarse_hop(vo, vi, 1, -1.0, True); y = vo.download()          # odd sites: out -= hop
        assert np.array_equal(y[~odd], o[~odd]) and np.all(np.abs(y - (o - hop))[odd] <= tol[odd])
        vo.upload(o); ctx.coarse_hop(vo, vi, 0, 1.0, False); y0 = vo.download()         # even sites: out = hop
        assert np.array_equal(y0[odd], o[odd]) and np.all(np.abs(y0 - hop)[~odd] <= tol[~odd])
        ctx.coarse_self_mul(t, vi, 0, False); m0x = t.download()
        ref = np.einsum("xij,xj->xi", cm.mats[0], xc)
        btol = (cm.bound(x) - cm.bound(x, first=1))[..., None] if bits == 16 else 1e-5 * np.abs(ref).max()
        assert np.all((np.abs(m0x - np.stack([ref.real, ref.imag], axis=-1)) <= btol)[~odd])
        vo.upload(o); ctx.coarse_self_mul(vo, t, 0, True); z = vo.download()            # M0^-1 applied to what the device made of M0 x
        assert np.array_equal(z[odd], o[odd])
        inv = np.linalg.inv(cm.mats[0]); tc = m0x[..., 0] + 1j * m0x[..., 1]; at = np.abs(m0x).sum(axis=-1)
        zref = np.einsum("xij,xj->xi", inv, tc)
        fp32 = 1e-5 * np.abs(zref).max()                                                # the device's inverse is fp32, as are its sums
        s_inv = np.maximum(np.abs(inv.real).max(axis=(1, 2)), np.abs(inv.imag).max(axis=(1, 2)))
        itol = fp32 + (2.0 ** -10 * np.einsum("xij,xj->xi", np.abs(inv.real) + np.abs(inv.imag), at) + 2.0 ** -23 * (s_inv * at.sum(axis=1))[:, None] if bits == 16 else 0.0)
        assert np.all((np.abs(z - np.stack([zref.real, zref.imag], axis=-1)) <= np.broadcast_to(itol, (V, n))[..., None])[~odd])
        got[bits] = (y, y0, m0x, z)
    ctx.set_coarse_storage(32)
    for v in (vi, vo, t):
        v.free()
    assert all(not np.array_equal(a, b) for a, b in zip(got[16], got[32]))


# ---- 2. the coarsest solve --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["a", "c"])
def test_coarsest_solve_in_16_bit_storage(which, request):
    ctx, _ = request.getfixturevalue("hier_" + which)
    V, n = ctx.volume(1), ctx.ndof(1)
    bh = splitmix_uniform(V * n * 2, 777).reshape(V, n, 2)
    b = ctx.vector(1, 32).upload(bh); x = ctx.vector(1, 32)
    ctx.set_coarse_storage(32)
    it32 = ctx.coarse_solve(x, b)
    ctx.set_coarse_storage(16)
    it16 = ctx.coarse_solve(x, b)
    x16 = x.download()
    ctx.set_coarse_storage(32)
    b.free(); x.free()
    # the residual against the downloaded operator in fp64; the slack 2^-8 is for the 2^-10-level difference between the
    # operator that was solved and the one that is checked
    res = np.linalg.norm(bh - CoarseMatrices(ctx).apply(x16)) / np.linalg.norm(bh)
    print(f"({which}) coarsest solve: {it32} iterations in 32-bit storage, {it16} in 16-bit; residual {res:.4e} of the right-hand side")
    assert res <= COARSE_TOL * (1 + 2.0 ** -8)
    assert abs(it16 - it32) <= 1


# ---- 3. the copy follows the operator ------------------------------------------------------------------------------------
def test_the_16_bit_copy_follows_mass_shift_and_operator_import(gold4):
    ctx = ctx_a(gold4)
    m0 = float(gold4["meta_f64"][0])
    xs = inputs(ctx)
    V, n = ctx.volume(1), ctx.ndof(1)
    cm0 = CoarseMatrices(ctx)
    first = applies(ctx, xs, 16)
    ctx.shift_mass(m0 + 0.1)
    cm1 = CoarseMatrices(ctx)
    y16 = applies(ctx, xs, 16); y32 = applies(ctx, xs, 32)
    for k, x in xs.items():
        assert_within_bound(y16[k], y32[k], cm1.bound(x), "shifted, " + k)
    # an unshifted copy would have left y16 where it was: on the unit vector the shifted diagonal entry moves its component by
    # 0.1, far more than the bound -- by the downloaded operators first, then on the device
    B0, B1 = cm0.bound(xs["unit"])[V - 1, n - 1], cm1.bound(xs["unit"])[V - 1, n - 1]
    moved = abs(cm1.apply(xs["unit"])[V - 1, n - 1, 0] - cm0.apply(xs["unit"])[V - 1, n - 1, 0])
    assert moved > 2 * (B0 + B1)
    assert abs(y16["unit"][V - 1, n - 1, 0] - first["unit"][V - 1, n - 1, 0]) > B1
    ctx.shift_mass(m0)
    back = applies(ctx, xs, 16)
    for k in xs:
        assert np.array_equal(back[k], first[k])
    # another operator through set_coarse_operator: the reference's own Galerkin product
    ctx.set_coarse_operator(gold4["coarse_D"], gold4["coarse_clover"])
    cm2 = CoarseMatrices(ctx)
    y16 = applies(ctx, xs, 16); y32 = applies(ctx, xs, 32)
    for k, x in xs.items():
        assert_within_bound(y16[k], y32[k], cm2.bound(x), "imported, " + k)
        assert not np.array_equal(y16[k], first[k])
    ctx.close()


# ---- 4. the whole solve ----------------------------------------------------------------------------------------------
def three_level_ctx(gold8):
    g3 = load_golden("ref_8x8_3lvl.npz")
    p = api.default_params()
    p.num_levels = 3
    for mu in range(4):
        p.local_lattice[0][mu] = 8; p.block_lattice[0][mu] = 2
        p.local_lattice[1][mu] = 4; p.block_lattice[1][mu] = 2
        p.local_lattice[2][mu] = 2
    p.num_vect[0] = 28; p.num_vect[1] = 28
    p.post_smooth_iter[0] = p.post_smooth_iter[1] = 2; p.block_iter[0] = p.block_iter[1] = 4
    p.setup_iter[0] = 4; p.setup_iter[1] = 3
    p.restart, p.max_restart, p.tol = 50, 20, 1e-10
    p.coarse_iter, p.coarse_restart, p.coarse_tol = 100, 5, COARSE_TOL
    p.kcycle, p.kcycle_restart, p.kcycle_max_restart, p.kcycle_tol = 1, 5, 2, 1e-1
    p.mixed_precision, p.method, p.odd_even = 1, 2, 1
    p.m0, p.csw = float(g3["meta_f64"][0]), float(g3["meta_f64"][1])
    ctx = dd.Context(p)
    ctx.set_gauge(gold8["gauge"], anti_pbc=True)
    return ctx


@pytest.mark.parametrize("hierarchy", ["ref_4x4", "ref_8x8_3lvl"])
def test_solve_in_32_16_32_bit_storage(hierarchy, gold4, gold8):
    if hierarchy == "ref_4x4":
        ctx = dd.Context(two_level_params(4, 2, 20, float(gold4["meta_f64"][0]), float(gold4["meta_f64"][1])))
        ctx.set_operator(gold4["D"], gold4["clover"])
    else:
        ctx = three_level_ctx(gold8)
    ctx.setup(4)
    b = np.zeros((ctx.volume(0), 12, 2)); b[..., 0] = 1.0
    runs = []
    for bits in (32, 16, 32):
        ctx.set_coarse_storage(bits)
        x, it, cit, rr = ctx.solve(b, 1e-10)
        runs.append((x.copy(), it, cit, rr, ctx.residual_history()))
    ctx.close()
    (x1, it1, cit1, rr1, h1), (x2, it2, cit2, rr2, h2), (x3, it3, cit3, rr3, h3) = runs
    print(f"{hierarchy}: outer iterations {it1} (32-bit) / {it2} (16-bit), coarse iterations {cit1} / {cit2}, relres {rr1:.3e} / {rr2:.3e}")
    assert rr2 <= 1e-10
    assert it2 <= it1 + 1
    assert abs(cit2 - cit1) <= 0.1 * cit1 + 1
    assert not np.array_equal(x2, x1)
    assert np.array_equal(x3, x1) and (it3, cit3, rr3) == (it1, cit1, rr1) and np.array_equal(h3, h1)


# ---- 5. the setup never sees the setting -----------------------------------------------------------------------------
@pytest.mark.parametrize("bootstrap", ["lockstep", "one-at-a-time"])
def test_setup_runs_on_the_32_bit_couplings_whatever_the_setting(gold4, monkeypatch, bootstrap):
    """A setup under DDAMG_COARSE_HALF=1 against one without the switch, on the same rand() stream: the same coarse iteration
    count, the same interpolation bit for bit.  The default bootstrap solves its coarsest systems in lockstep (coarse_lockstep.h),
    which never reads the 16-bit copy; with DDAMG_BOOTSTRAP_UNBATCHED every V-cycle of the bootstrap goes through coarse_solve(),
    the path the storage switches, so that case holds only through the setup's own guard.
    The golden file of the 4^4 configuration records no iteration count of the setup itself; what it records of a run after the
    reference's setup on the same stream is checked in the next test."""
    if bootstrap == "one-at-a-time":
        monkeypatch.setenv("DDAMG_BOOTSTRAP_UNBATCHED", "1")
    res = []
    for half in (None, "1"):
        if half:
            monkeypatch.setenv("DDAMG_COARSE_HALF", half)       # a context's switches are the environment at its creation
        ctx = dd.Context(two_level_params(4, 2, 20, float(gold4["meta_f64"][0]), float(gold4["meta_f64"][1])))
        ctx.set_operator(gold4["D"], gold4["clover"])
        ci = ctx.setup(4)
        vi = ctx.vector(1, 32).upload(inputs(ctx)["random"]); vo = ctx.vector(1, 32)
        ctx.coarse_apply(vo, vi)
        res.append((ci, ctx.get_interpolation(), vo.download(), ctx))
    monkeypatch.delenv("DDAMG_COARSE_HALF")
    (ci0, P0, y0, c0), (ci1, P1, y1, c1) = res
    print(f"{bootstrap}: {ci0} coarse iterations of the setup without the switch, {ci1} with it")
    assert ci1 == ci0 and ci0 > 0
    assert np.array_equal(P1, P0)
    assert not np.array_equal(y1, y0)            # the same hierarchy, but the second context does start in 16-bit storage
    # a further setup_update in 16-bit storage leaves the setting as it was: still 16 afterwards, and the same vectors as in c0
    c0.setup_update(1); c1.setup_update(1)
    assert np.array_equal(c1.get_interpolation(), c0.get_interpolation())
    vi = c1.vector(1, 32).upload(inputs(c1)["random"]); vo = c1.vector(1, 32); c1.coarse_apply(vo, vi); y16 = vo.download()
    c1.set_coarse_storage(32); c1.coarse_apply(vo, vi)
    assert not np.array_equal(y16, vo.download())
    c0.close(); c1.close()


def test_solve_after_a_setup_under_the_switch_matches_the_golden_run(gold4, monkeypatch):
    """what tests/golden/ref_4x4.npz records of the run after the reference's setup -- 11 outer and 72 coarse iterations for
    rhs = ones -- after our setup under DDAMG_COARSE_HALF=1, with the tolerances of test_full_setup_and_solve_iteration_parity"""
    monkeypatch.setenv("DDAMG_COARSE_HALF", "1")
    ctx = dd.Context(two_level_params(4, 2, 20, float(gold4["meta_f64"][0]), float(gold4["meta_f64"][1])))
    ctx.set_operator(gold4["D"], gold4["clover"])
    ctx.setup(4)
    ctx.set_coarse_storage(32)
    b = np.zeros((ctx.volume(0), 12, 2)); b[..., 0] = 1.0
    x, it, cit, rr = ctx.solve(b, 1e-10)
    ctx.close()
    assert it == int(gold4["ones_solve_iters"][0]) and abs(cit - int(gold4["ones_solve_iters"][1])) <= 8 and rr < 1e-10


# ---- 6. memory and refusals ---------------------------------------------------------------------------------------------
def test_memory_of_the_copy_and_refusals(gold4):
    before = api.memory_in_use()[0]
    ctx = ctx_a(gold4)
    xs = inputs(ctx)
    vi = ctx.vector(1, 32).upload(xs["random"]); vo = ctx.vector(1, 32)
    ctx.coarse_apply(vo, vi); y32 = vo.download()
    m32 = api.memory_in_use()[0]
    ctx.set_coarse_storage(16)
    assert api.memory_in_use()[0] == m32                     # nothing before the first use
    ctx.coarse_apply(vo, vi)
    V, n = ctx.volume(1), ctx.ndof(1); nt = (n + 7) // 8
    fp32_bytes = V * 6 * nt * nt * 64 * 8                     # M[0..4] and Minv, 8 bytes per complex number
    rise = api.memory_in_use()[0] - m32
    print(f"16-bit copy: {rise} bytes, fp32 couplings {fp32_bytes}")
    assert 0.5 * fp32_bytes <= rise <= 0.5 * fp32_bytes + 0.01 * fp32_bytes
    ctx.set_coarse_storage(32)
    assert api.memory_in_use()[0] == m32
    with pytest.raises(dd.DDAMGError, match="16 or 32"):
        ctx.set_coarse_storage(8)
    ctx.coarse_apply(vo, vi)
    assert np.array_equal(vo.download(), y32) and api.memory_in_use()[0] == m32
    vi.free(); vo.free()
    ctx.close()
    assert api.memory_in_use()[0] == before
    for kw, prec, word in ((dict(mixed_precision=0), 64, "mixed_precision"), (dict(odd_even=0), 32, "odd_even")):
        c = ctx_a(gold4, **kw)
        vi = c.vector(1, prec).upload(xs["random"]); vo = c.vector(1, prec)
        c.coarse_apply(vo, vi); y = vo.download()
        m = api.memory_in_use()[0]
        with pytest.raises(dd.DDAMGError, match=word):
            c.set_coarse_storage(16)
        c.coarse_apply(vo, vi)
        assert np.array_equal(vo.download(), y) and api.memory_in_use()[0] == m
        vi.free(); vo.free()
        c.close()
    assert api.memory_in_use()[0] == before
