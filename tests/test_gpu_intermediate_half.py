"""GPU tests (-m gpu) of the intermediate levels' couplings in 16-bit storage (ddamg_hip_set_intermediate_storage,
coarse_half_level.hip): the three kernels on an operator that the format holds exactly (where the two storages differ by the
order of their sums only), on the real operator against the format bound of tests/test_gpu_coarse_half.py, fused against
unfused block solver, K-cycle and solve in both storages, the setup staying on the fp32 couplings, the copy following the
operator, memory accounting and the refusals.

Hierarchies (level 1 is the intermediate level):
  S  ref_8x8_3lvl_small.npz as test_gpu_three_levels.py::ref3 builds it: 4^4, n = 16 (one tile group), Schwarz blocks of 16 sites
  P  ref_16x8_3lvl_prod.npz the same way: 4 x 2^3, n = 48 (nine groups), blocks of 2 sites, forward = backward neighbour in three directions
  Q  the 8^4 golden gauge field -> 4^4 -> 2^4 with 24 / 28 test vectors and setup(1): n = 48, blocks of 16 sites
  T  as Q with 10 test vectors on the fine level: n = 20 (padding rows; nine tiles = two groups and the tail tile)

Four levels (tests/golden/ref_16x16_4lvl.json) are not run here.

Tolerances.  TOL_KERNEL and TOL_SWEEP are those of test_gpu_three_levels.py for the same kernels; the smoother is compared in the
norm that file uses (relerr) and in the largest component.  The bound B of the real-operator tests is CoarseMatrices.bound,
derived in the docstring of test_gpu_coarse_half.py."""
import numpy as np
import pytest
from conftest import load_golden, splitmix_uniform, relerr, random_su3
from test_gpu_coarse_half import CoarseMatrices, assert_within_bound, two_level_params
from test_gpu_three_levels import TOL_KERNEL, TOL_SWEEP, maxerr
from ddalphaamg_amd import api
import ddalphaamg_amd as dd

pytestmark = pytest.mark.gpu

GOLDEN = {"S": "ref_8x8_3lvl_small.npz", "P": "ref_16x8_3lvl_prod.npz"}


# ---- contexts --------------------------------------------------------------------------------------------------------------
def golden_params(name, **over):
    """the parameters of test_gpu_three_levels.py::make_ctx"""
    g = load_golden(name)
    L0 = [int(x) for x in g["meta_int"][:4]]; B0 = [int(x) for x in g["meta_int"][4:8]]
    m3 = [int(x) for x in g["meta3_int"]]
    p = api.default_params()
    p.num_levels = 3
    for mu in range(4):
        p.local_lattice[0][mu] = L0[mu]; p.block_lattice[0][mu] = B0[mu]
        p.local_lattice[1][mu] = m3[mu]; p.block_lattice[1][mu] = m3[4 + mu]
        p.local_lattice[2][mu] = m3[8 + mu]
    p.num_vect[0], p.num_vect[1] = m3[12], m3[13]
    p.post_smooth_iter[0] = 2; p.post_smooth_iter[1] = m3[14]; p.block_iter[0] = 4; p.block_iter[1] = m3[15]
    p.setup_iter[0] = 2; p.setup_iter[1] = 2
    p.restart, p.max_restart, p.tol = 50, 20, 1e-10
    p.coarse_iter, p.coarse_restart, p.coarse_tol = 100, 5, 5e-2
    p.kcycle, p.kcycle_restart, p.kcycle_max_restart, p.kcycle_tol = 1, 5, 2, 1e-1
    p.mixed_precision, p.method, p.odd_even = 1, 2, 1
    p.m0, p.csw = float(g["meta_f64"][0]), float(g["meta_f64"][1])
    for k, v in over.items():
        setattr(p, k, v)
    return g, p


def golden_gauge(name, p):
    V = int(np.prod([int(v) for v in p.local_lattice[0]]))
    if name.startswith("ref_8x8"):
        return load_golden("ref_8x8_dirac.npz")["gauge"]
    return random_su3(V * 4, 1618).reshape(V, 4, 9, 2)   # oracle/make_golden.py: synthetic=1618


def golden_ctx(which, whole=True, **over):
    """S or P: the reference's level-1 operator (and, whole = True, its interpolation vectors of both levels: the whole hierarchy)"""
    name = GOLDEN[which]
    g, p = golden_params(name, **over)
    ctx = dd.Context(p)
    ctx.set_gauge(golden_gauge(name, p), anti_pbc=True)
    if whole and "interp_vectors" in g.files:
        ctx.set_interpolation(g["interp_vectors"], level=0)
    ctx.set_coarse_operator(g["coarse_D"], g["coarse_clover"], level=1)
    if whole:
        ctx.set_interpolation(g["l1_interp_vectors"], level=1)
    return ctx


def setup_params(nv0):
    """Q (nv0 = 24) and T (nv0 = 10)"""
    g3 = load_golden("ref_8x8_3lvl.npz")
    p = api.default_params()
    p.num_levels = 3
    for mu in range(4):
        p.local_lattice[0][mu] = 8; p.block_lattice[0][mu] = 2
        p.local_lattice[1][mu] = 4; p.block_lattice[1][mu] = 2
        p.local_lattice[2][mu] = 2
    p.num_vect[0] = nv0; p.num_vect[1] = 28
    p.post_smooth_iter[0] = p.post_smooth_iter[1] = 2; p.block_iter[0] = p.block_iter[1] = 4
    p.setup_iter[0] = 1; p.setup_iter[1] = 1
    p.restart, p.max_restart, p.tol = 50, 20, 1e-10
    p.coarse_iter, p.coarse_restart, p.coarse_tol = 100, 5, 5e-2
    p.kcycle, p.kcycle_restart, p.kcycle_max_restart, p.kcycle_tol = 1, 5, 2, 1e-1
    p.mixed_precision, p.method, p.odd_even = 1, 2, 1
    p.m0, p.csw = float(g3["meta_f64"][0]), float(g3["meta_f64"][1])
    return p


def setup_ctx(nv0, gold8):
    ctx = dd.Context(setup_params(nv0))
    ctx.set_gauge(gold8["gauge"], anti_pbc=True)
    ctx.setup(1)
    return ctx


def bare_ctx(nv0, gold8, D1, cl1):
    """the shape of Q / T without a setup, carrying the level-1 operator (D1, cl1): what the level-1 apply and smoother need"""
    ctx = dd.Context(setup_params(nv0))
    ctx.set_gauge(gold8["gauge"], anti_pbc=True)
    ctx.set_coarse_operator(D1, cl1, level=1)
    return ctx


def inputs(ctx):
    V, n = ctx.volume(1), ctx.ndof(1)
    unit = np.zeros((V, n, 2)); unit[V - 1, n - 1, 0] = 1.0
    return {"random": splitmix_uniform(V * n * 2, 4242).reshape(V, n, 2), "unit": unit}


def applies(ctx, xs, bits=None):
    """the level-1 coarse_apply of every input, with the storage set to `bits` first (and left there); None: as the context is"""
    if bits is not None:
        ctx.set_intermediate_storage(bits)
    vi = ctx.vector(1, 32); vo = ctx.vector(1, 32)
    out = {k: (vi.upload(x), ctx.coarse_apply(vo, vi), vo.download())[2] for k, x in xs.items()}
    vi.free(); vo.free()
    return out


def smooths(ctx, bits):
    """the level-1 smoother outputs of this module's cases in the given storage: cycles 1 and 2 from zero, and from a random start"""
    V, n = ctx.volume(1), ctx.ndof(1)
    ctx.set_intermediate_storage(bits)
    eta = ctx.vector(1, 32).upload(splitmix_uniform(V * n * 2, 31).reshape(V, n, 2)); phi = ctx.vector(1, 32)
    phi0 = splitmix_uniform(V * n * 2, 32).reshape(V, n, 2)
    out = {}
    for cyc in (1, 2):
        ctx.smoother(phi, eta, cyc, initial_guess_zero=True)
        out[f"zero start, {cyc} cycles"] = phi.download()
        phi.upload(phi0)
        ctx.smoother(phi, eta, cyc, initial_guess_zero=False)
        out[f"random start, {cyc} cycles"] = phi.download()
    eta.free(); phi.free()
    return out


@pytest.fixture(scope="module")
def hier_S():
    ctx = golden_ctx("S")
    yield ctx, applies(ctx, inputs(ctx))
    ctx.close()


@pytest.fixture(scope="module")
def hier_P():
    ctx = golden_ctx("P")
    yield ctx, applies(ctx, inputs(ctx))
    ctx.close()


@pytest.fixture(scope="module")
def hier_Q(gold8):
    ctx = setup_ctx(24, gold8)
    yield ctx, applies(ctx, inputs(ctx))
    ctx.close()


@pytest.fixture(scope="module")
def hier_T(gold8):
    ctx = setup_ctx(10, gold8)
    yield ctx, applies(ctx, inputs(ctx))
    ctx.close()


# ---- 1. an operator that the 16-bit format holds exactly -----------------------------------------------------------------
def quantise(a):
    """a: [matrices][reals of one device matrix].  P2 the power of two at or above the matrix's largest |entry|; every entry
    rounded to a multiple of P2 * 2^-10, the largest one set to +-P2"""
    a = np.array(a, dtype=np.float64)
    rows = np.arange(a.shape[0])
    big = np.abs(a).argmax(axis=1)
    P2 = 2.0 ** np.ceil(np.log2(np.abs(a).max(axis=1)))
    q = np.round(a / (P2[:, None] * 2.0 ** -10)) * (P2[:, None] * 2.0 ** -10)
    q[rows, big] = np.sign(a[rows, big]) * P2
    return q


def lossless_operator(D, cl):
    """(D, cl) in the import format, every device matrix quantised: a link is the n x n matrix of its four blocks; the self
    coupling is given by its packed form (the upper triangles of A and D, and B), whose entries are, up to signs, the entries of
    the device matrix [A B; -B^H D] -- the entry that becomes P2 is chosen there, and its mirror image follows it.
    Asserts the premise of the test: with s the matrix maximum, fp16(a / s) * s == a for every entry"""
    V = D.shape[0]
    Dq = quantise(D.reshape(V * 4, -1)).reshape(D.shape)
    clq = quantise(cl.reshape(V, -1)).reshape(cl.shape)
    for a in (Dq.reshape(V * 4, -1), clq.reshape(V, -1)):
        s = np.abs(a).max(axis=1)[:, None]
        assert np.all(s > 0) and np.array_equal(np.float16(a / s).astype(np.float64) * s, a)
        assert np.array_equal(np.float32(a).astype(np.float64), a)          # and fp32 holds it as well
    return Dq, clq


@pytest.mark.parametrize("once", [False, True], ids=["site-kernel", "every-link-once"])
@pytest.mark.parametrize("which", ["S", "P", "T"])
def test_lossless_storage_gives_the_fp32_result(which, once, gold8, monkeypatch, request):
    """apply (both forms: DDAMG_COARSE_APPLY_ONCE_MIN_SITES at its default, where these lattices take the listed site kernel, and
    1) and smoother of level 1 in both storages on an operator whose 16-bit copy is exact"""
    if once:
        monkeypatch.setenv("DDAMG_COARSE_APPLY_ONCE_MIN_SITES", "1")     # a context's switches are the environment at its creation
    else:
        monkeypatch.delenv("DDAMG_COARSE_APPLY_ONCE_MIN_SITES", raising=False)
    if which == "T":
        D1, cl1 = request.getfixturevalue("hier_T")[0].get_coarse_operator(level=1)
        Dq, clq = lossless_operator(D1, cl1)
        ctx = bare_ctx(10, gold8, Dq, clq)
    else:
        g = load_golden(GOLDEN[which])
        Dq, clq = lossless_operator(g["coarse_D"], g["coarse_clover"])
        ctx = golden_ctx(which, whole=False)
        ctx.set_coarse_operator(Dq, clq, level=1)
    xs = inputs(ctx)
    y32 = applies(ctx, xs, 32); y16 = applies(ctx, xs, 16)
    s32 = smooths(ctx, 32); s16 = smooths(ctx, 16)
    ctx.close()
    for k in xs:
        e = maxerr(y16[k], y32[k])
        print(f"{which}, {'once' if once else 'site'}, apply, {k}: {e:.3e} of the largest component")
        assert e <= TOL_KERNEL, k
    for k in s32:
        e, em = relerr(s16[k], s32[k]), maxerr(s16[k], s32[k])
        print(f"{which}, smoother, {k}: relative difference {e:.3e}, {em:.3e} of the largest component")
        assert np.all(np.isfinite(s16[k])) and np.abs(s32[k]).max() > 0
        assert e <= TOL_SWEEP and em <= TOL_SWEEP, k


# ---- 2. the real operator within the format bound ------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["S", "P", "Q", "T"])
def test_apply_in_16_bit_storage_is_within_the_format_bound(which, request):
    ctx, y32 = request.getfixturevalue("hier_" + which)          # y32: from before any switch
    xs = inputs(ctx)
    y16 = applies(ctx, xs, 16)
    y32_again = applies(ctx, xs, 32)
    cm = CoarseMatrices(ctx)
    for k, x in xs.items():
        ref = cm.apply(x)
        assert np.abs(y32[k] - ref).max() <= 1e-5 * np.abs(ref).max()          # the numpy operator is the one on the device
        assert_within_bound(y16[k], y32[k], cm.bound(x), f"{which}, {k}")
        assert not np.array_equal(y16[k], y32[k])                              # the 16-bit path was taken
        assert np.array_equal(y32_again[k], y32[k])                            # 32 bits again: the fp32 kernel, bit for bit


# ---- 3. fused and unfused block solver ---------------------------------------------------------------------------------
def test_fused_and_unfused_block_solver_agree_in_16_bit_storage(hier_Q, gold8, monkeypatch):
    """the smoother of level 1 through the fused block solver and, under DDAMG_COARSE_SAP_UNFUSED, step by step on the listed site
    kernel: two contexts that carry the same level-1 operator"""
    D1, cl1 = hier_Q[0].get_coarse_operator(level=1)
    res = []
    for unfused in (False, True):
        if unfused:
            monkeypatch.setenv("DDAMG_COARSE_SAP_UNFUSED", "1")
        else:
            monkeypatch.delenv("DDAMG_COARSE_SAP_UNFUSED", raising=False)
        ctx = bare_ctx(24, gold8, D1, cl1)
        res.append(smooths(ctx, 16))
        ctx.close()
    for k in res[0]:
        e, em = relerr(res[1][k], res[0][k]), maxerr(res[1][k], res[0][k])
        print(f"Q, {k}: unfused against fused {e:.3e}, {em:.3e} of the largest component")
        assert e <= TOL_SWEEP and em <= TOL_SWEEP, k
        assert not np.array_equal(res[1][k], res[0][k])           # two code paths did run


# ---- 4. K-cycle and solve ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["S", "Q"])
def test_kcycle_and_solve_in_32_16_32_bit_storage(which, request):
    ctx, _ = request.getfixturevalue("hier_" + which)
    V1, n1 = ctx.volume(1), ctx.ndof(1)
    b1 = ctx.vector(1, 32).upload(splitmix_uniform(V1 * n1 * 2, 555).reshape(V1, n1, 2)); x1 = ctx.vector(1, 32)
    b = np.zeros((ctx.volume(0), 12, 2)); b[..., 0] = 1.0
    runs = []
    for bits in (32, 16, 32):
        ctx.set_intermediate_storage(bits)
        kit = ctx.kcycle(x1, b1); xk = x1.download()
        x, it, cit, rr = ctx.solve(b, 1e-10)
        runs.append((x.copy(), it, cit, rr, ctx.residual_history(), kit, xk))
    b1.free(); x1.free()
    (xa, it1, cit1, rr1, h1, k1, xk1), (xb, it2, cit2, rr2, h2, k2, xk2), (xc, it3, cit3, rr3, h3, k3, xk3) = runs
    print(f"{which}: K-cycle iterations {k1} (32-bit) / {k2} (16-bit); outer iterations {it1} / {it2}, coarse iterations {cit1} / {cit2}, "
          f"relres {rr1:.3e} / {rr2:.3e}")
    assert k2 in (k1, k1 + 1)
    assert not np.array_equal(xk2, xk1)
    assert rr2 <= 1e-10
    assert it2 <= it1 + 1
    assert abs(cit2 - cit1) <= 0.1 * cit1 + 1
    assert not np.array_equal(xb, xa)
    assert np.array_equal(xc, xa) and (it3, cit3, rr3) == (it1, cit1, rr1) and np.array_equal(h3, h1)
    assert k3 == k1 and np.array_equal(xk3, xk1)


# ---- 5. the setup never sees the setting -----------------------------------------------------------------------------
def level1_interpolation(ctx):
    """the interpolation operator of level 1, column by column: aggregates do not overlap, so the level-2 vector that is 1 in
    component k of every site interpolates to column k of every aggregate, exactly"""
    V2, n2 = ctx.volume(2), ctx.ndof(2)
    c = ctx.vector(2, 32); f = ctx.vector(1, 32)
    cols = []
    for k in range(n2):
        e = np.zeros((V2, n2, 2)); e[:, k, 0] = 1.0
        c.upload(e); ctx.interpolate(f, c)
        cols.append(f.download())
    c.free(); f.free()
    return np.stack(cols)


def test_setup_runs_on_the_fp32_couplings_whatever_the_setting(monkeypatch):
    """setup(2) on the lattice of S under DDAMG_INTERMEDIATE_HALF=1 against one without the switch, on the same rand() stream:
    both interpolation operators and the operators of levels 1 and 2 bit for bit (with DDAMG_BOOTSTRAP_UNBATCHED as well, where
    the bootstrap's K-cycles go through the products the switch moves); the first level-1 apply of the second context differs"""
    name = GOLDEN["S"]
    for unbatched in (False, True):
        if unbatched:
            monkeypatch.setenv("DDAMG_BOOTSTRAP_UNBATCHED", "1")
        res = []
        for half in (None, "1"):
            if half:
                monkeypatch.setenv("DDAMG_INTERMEDIATE_HALF", half)
            g, p = golden_params(name)
            ctx = dd.Context(p)
            ctx.set_gauge(golden_gauge(name, p), anti_pbc=True)
            ci = ctx.setup(2)
            res.append((ci, ctx.get_interpolation(), level1_interpolation(ctx), ctx.get_coarse_operator(level=1), ctx.get_coarse_operator(level=2),
                        applies(ctx, inputs(ctx))))
            ctx.close()
        monkeypatch.delenv("DDAMG_INTERMEDIATE_HALF")
        (ci0, P0, Q0, op10, op20, y0), (ci1, P1, Q1, op11, op21, y1) = res
        print(f"{'one-at-a-time' if unbatched else 'batched'} bootstrap: {ci0} coarse iterations of the setup without the switch, {ci1} with it")
        assert ci1 == ci0 and ci0 > 0
        assert np.array_equal(P1, P0) and np.array_equal(Q1, Q0)
        assert all(np.array_equal(a, b) for a, b in zip(op11 + op21, op10 + op20))
        assert all(not np.array_equal(y1[k], y0[k]) for k in y0)     # the same hierarchy, but the second context does start in 16-bit storage


# ---- 6. the copy follows the operator ------------------------------------------------------------------------------------
def test_the_16_bit_copy_follows_mass_shift_and_operator_import(gold8):
    ctx = setup_ctx(24, gold8)                     # Q, its own context: the operator is replaced at the end
    m0 = float(ctx.params.m0)
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
    # 0.1, far more than the bound
    B0, B1 = cm0.bound(xs["unit"])[V - 1, n - 1], cm1.bound(xs["unit"])[V - 1, n - 1]
    moved = abs(cm1.apply(xs["unit"])[V - 1, n - 1, 0] - cm0.apply(xs["unit"])[V - 1, n - 1, 0])
    assert moved > 2 * (B0 + B1)
    assert abs(y16["unit"][V - 1, n - 1, 0] - first["unit"][V - 1, n - 1, 0]) > B1
    ctx.shift_mass(m0)
    back = applies(ctx, xs, 16)
    for k in xs:
        assert np.array_equal(back[k], first[k])
    # another operator through set_coarse_operator(level=1): links and self couplings rescaled, far from the first
    D1, cl1 = ctx.get_coarse_operator(level=1)
    ctx.set_coarse_operator(1.3 * D1, 0.9 * cl1, level=1)
    cm2 = CoarseMatrices(ctx)
    y16 = applies(ctx, xs, 16); y32 = applies(ctx, xs, 32)
    for k, x in xs.items():
        assert_within_bound(y16[k], y32[k], cm2.bound(x), "imported, " + k)
        assert not np.array_equal(y16[k], y32[k])
        assert np.abs(y16[k] - first[k]).max() > 2 * (cm0.bound(x) + cm2.bound(x)).max()     # a copy of the first operator would have stayed near `first`
    ctx.close()


# ---- 7. memory and refusals ---------------------------------------------------------------------------------------------
def test_memory_of_the_copy_and_refusals(gold4):
    before = api.memory_in_use()[0]
    ctx = golden_ctx("S")
    xs = inputs(ctx)
    vi = ctx.vector(1, 32).upload(xs["random"]); vo = ctx.vector(1, 32); ph = ctx.vector(1, 32)
    ctx.coarse_apply(vo, vi); y32 = vo.download()
    ctx.smoother(ph, vi, 1)
    m32 = api.memory_in_use()[0]
    ctx.set_intermediate_storage(16)
    assert api.memory_in_use()[0] == m32                     # nothing before the first use
    ctx.coarse_apply(vo, vi)
    ctx.smoother(ph, vi, 1)                                  # the smoother reads the same copy
    V, n = ctx.volume(1), ctx.ndof(1); nt = (n + 7) // 8
    fp32_bytes = V * 5 * nt * nt * 64 * 8                     # M[0..4] of level 1, 8 bytes per complex number
    rise = api.memory_in_use()[0] - m32
    print(f"16-bit copy: {rise} bytes, fp32 couplings {fp32_bytes}")
    assert 0.5 * fp32_bytes <= rise <= 0.51 * fp32_bytes
    ctx.set_intermediate_storage(32)
    assert api.memory_in_use()[0] == m32
    with pytest.raises(dd.DDAMGError, match="16 or 32"):
        ctx.set_intermediate_storage(8)
    ctx.coarse_apply(vo, vi)
    assert np.array_equal(vo.download(), y32) and api.memory_in_use()[0] == m32
    ctx.set_intermediate_storage(16)
    ctx.coarse_apply(vo, vi)
    assert api.memory_in_use()[0] == m32 + rise
    for v in (vi, vo, ph):
        v.free()
    ctx.close()                                              # in 16-bit storage: close() frees the copy as well
    assert api.memory_in_use()[0] == before
    # refusals: a message, and the storage as it was
    c = dd.Context(two_level_params(4, 2, 20, float(gold4["meta_f64"][0]), float(gold4["meta_f64"][1])))
    c.set_operator(gold4["D"], gold4["clover"])
    with pytest.raises(dd.DDAMGError, match="three levels"):
        c.set_intermediate_storage(16)
    c.set_intermediate_storage(32)
    c.close()
    for over, prec, word in ((dict(mixed_precision=0), 64, "mixed_precision"), (dict(method=4), 32, "method 1 to 3")):
        c = golden_ctx("S", whole=False, **over)
        vi = c.vector(1, prec).upload(xs["random"]); vo = c.vector(1, prec)
        c.coarse_apply(vo, vi); y = vo.download()
        m = api.memory_in_use()[0]
        with pytest.raises(dd.DDAMGError, match=word):
            c.set_intermediate_storage(16)
        c.coarse_apply(vo, vi)
        assert np.array_equal(vo.download(), y) and api.memory_in_use()[0] == m
        vi.free(); vo.free()
        c.close()
    assert api.memory_in_use()[0] == before
