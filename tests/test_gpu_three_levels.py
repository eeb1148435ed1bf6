"""GPU parity tests (-m gpu) of the INTERMEDIATE level and the SECOND coarse operator of a three-level hierarchy against dumps of
the real reference (oracle/ref_dump_stages.h dump_three_level):

  ref_8x8_3lvl_small.npz   the reference's 8^4 configuration, 8^4 -> 4^4 -> 2^4, 8 / 10 test vectors (16 / 20 dof per coarse
                           site): both interpolation operators, both coarse operators
  ref_16x8_3lvl_prod.npz   the production dof counts (48 / 56 per site) on 16 x 8^3 -> 4 x 2^3 -> 2^4 (Schwarz blocks of 2 x 1^3
                           sites on the intermediate level): the level-1 operator, its interpolation vectors, the level-2 operator

Element by element: the level-2 Galerkin operator (coarse_batch.hip on the matrix cores, and the column-by-column form); against
the dumped outputs: operator, restriction / interpolation, Schwarz smoother, V-cycle of the intermediate level -- one vector at a
time and for many right-hand sides at once (coarse_multi.hip, coarse_lockstep.hip: the kernels of the batched setup)."""
import numpy as np
import pytest
from conftest import relerr, splitmix_uniform, load_golden, random_su3
from ddalphaamg_amd import api
import ddalphaamg_amd as dd

pytestmark = pytest.mark.gpu

TOL_KERNEL = 5e-6
TOL_SWEEP = 1e-4


def make_ctx(name):
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
    ctx = dd.Context(p)
    V = int(np.prod(L0))
    if name.startswith("ref_8x8"):
        ctx.set_gauge(load_golden("ref_8x8_dirac.npz")["gauge"], anti_pbc=True)
    else:
        ctx.set_gauge(random_su3(V * 4, 1618).reshape(V, 4, 9, 2), anti_pbc=True)   # oracle/make_golden.py: synthetic=1618
    return g, ctx


def maxerr(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.fixture(scope="module", params=["ref_8x8_3lvl_small.npz", "ref_16x8_3lvl_prod.npz"], ids=["8x8-16-20dof", "16x8-48-56dof"])
def ref3(request):
    """context carrying the REFERENCE's level-1 operator and level-1 interpolation vectors; the level-2 operator is built from
    them by the library's Galerkin construction"""
    g, ctx = make_ctx(request.param)
    if "interp_vectors" in g.files:
        ctx.set_interpolation(g["interp_vectors"], level=0)
    ctx.set_coarse_operator(g["coarse_D"], g["coarse_clover"], level=1)
    ctx.set_interpolation(g["l1_interp_vectors"], level=1)
    yield g, ctx
    ctx.close()


def test_second_coarse_operator_element_by_element(ref3):
    """coarse_operator_PRECISION_setup on a coarse level (src/coarse_operator_generic.c:53-205): every entry of the level-2 self
    couplings and forward links; the matrix-core construction (coarse_batch_apply_kernel, coarse_batch_restrict_store_mfma_kernel)"""
    g, ctx = ref3
    D2, cl2 = ctx.get_coarse_operator(level=2)
    assert maxerr(D2, g["l2_coarse_D"]) < 1e-5 and maxerr(cl2, g["l2_coarse_clover"]) < 1e-5
    assert relerr(D2, g["l2_coarse_D"]) < 5e-6 and relerr(cl2, g["l2_coarse_clover"]) < 5e-6


def test_second_coarse_operator_column_by_column_form(monkeypatch):
    """the level-2 Galerkin operator in its column-by-column form (DDAMG_GALERKIN_UNBATCHED: masked gather + restriction + one
    store per column and part) and in the default matrix-core form, both from the reference's level-1 operator and
    interpolation vectors, both against the reference's level-2 operator.  A context's switches are the environment at its
    creation, so the variable is set before the context exists"""
    res = []
    for unbatched in (False, True):
        if unbatched:
            monkeypatch.setenv("DDAMG_GALERKIN_UNBATCHED", "1")
        g, ctx = make_ctx("ref_16x8_3lvl_prod.npz")
        ctx.set_coarse_operator(g["coarse_D"], g["coarse_clover"], level=1)
        ctx.set_interpolation(g["l1_interp_vectors"], level=1)
        D2, cl2 = ctx.get_coarse_operator(level=2)
        assert maxerr(D2, g["l2_coarse_D"]) < 1e-5 and maxerr(cl2, g["l2_coarse_clover"]) < 1e-5, unbatched
        res.append((D2, cl2))
        ctx.close()
    assert not np.array_equal(res[0][0], res[1][0])     # two code paths did run


@pytest.mark.parametrize("name", ["ref_8x8_3lvl_small.npz", "ref_16x8_3lvl_prod.npz"])
def test_gram_schmidt_on_the_aggregates_of_the_intermediate_level_in_registers(name, monkeypatch):
    """gram_schmidt_on_aggregates (src/linalg_generic.c:400-480) on the intermediate level in its three forms: the vector that is
    being orthogonalised in registers of one workgroup (DDAMG_COARSE_GS_FORM=workgroup) against the form that updates it through
    global memory (DDAMG_COARSE_GS_GLOBAL) -- the same element -> thread assignment and the same reductions, so the level-2
    operator of a whole setup agrees bit for bit -- and the default, one wavefront per aggregate and chirality"""
    res = []
    for form in ("wave", "workgroup", "global"):
        monkeypatch.delenv("DDAMG_COARSE_GS_GLOBAL", raising=False); monkeypatch.delenv("DDAMG_COARSE_GS_FORM", raising=False)
        if form == "global":
            monkeypatch.setenv("DDAMG_COARSE_GS_GLOBAL", "1")
        elif form == "workgroup":
            monkeypatch.setenv("DDAMG_COARSE_GS_FORM", "workgroup")
        g, ctx = make_ctx(name)
        ctx.setup(2)
        res.append(ctx.get_coarse_operator(level=2))
        ctx.close()
    assert np.array_equal(res[1][0], res[2][0]) and np.array_equal(res[1][1], res[2][1])
    # the default: one wavefront per aggregate and chirality, its sums by lane exchanges -- another order of the same sums
    assert maxerr(res[0][0], res[1][0]) < 2e-5 and maxerr(res[0][1], res[1][1]) < 2e-5


def test_whole_hierarchy_from_the_reference_interpolation_vectors():
    """both Galerkin constructions in a row from the reference's interpolation vectors of both levels (the level-1 operator is
    the library's own here, not the imported one)"""
    g, ctx = make_ctx("ref_8x8_3lvl_small.npz")
    ctx.set_interpolation(g["interp_vectors"], level=0)
    D1, cl1 = ctx.get_coarse_operator(level=1)
    assert maxerr(D1, g["coarse_D"]) < 1e-5 and maxerr(cl1, g["coarse_clover"]) < 1e-5
    ctx.set_interpolation(g["l1_interp_vectors"], level=1)
    D2, cl2 = ctx.get_coarse_operator(level=2)
    assert maxerr(D2, g["l2_coarse_D"]) < 2e-5 and maxerr(cl2, g["l2_coarse_clover"]) < 2e-5
    ctx.close()


def test_coarse_operators_apply(ref3):
    g, ctx = ref3
    for lvl in (1, 2):
        ctx.set_coarse_operator(g["coarse_D" if lvl == 1 else "l2_coarse_D"], g["coarse_clover" if lvl == 1 else "l2_coarse_clover"], level=lvl)
        x = ctx.vector(lvl, 32).upload(g[f"l{lvl}_apply_in"]); y = ctx.vector(lvl, 32)
        ctx.coarse_apply(y, x)
        assert relerr(y.download(), g[f"l{lvl}_apply_out"]) < TOL_KERNEL
        x.free(); y.free()


def columns(ctx, lvl, first, ncols, seed):
    """ncols host vectors of level lvl: `first`, then seeded random ones (one of them zero)"""
    n = ctx.ndof(lvl); V = ctx.volume(lvl)
    hs = [np.asarray(first, dtype=np.float64)]
    for c in range(1, ncols):
        hs.append(np.zeros((V, n, 2)) if c == 2 else splitmix_uniform(V * n * 2, seed + c).reshape(V, n, 2))
    return hs


@pytest.mark.parametrize("lvl", [1, 2])
def test_coarse_operator_of_many_right_hand_sides_on_the_matrix_cores(ref3, lvl):
    """cm_apply_kernel (intermediate level) and ls_self_kernel / ls_hop_kernel (coarsest level) on the reference's own operator:
    column 0 against the reference's apply_coarse_operator_float output, every column against the one-vector kernel"""
    g, ctx = ref3
    ctx.set_coarse_operator(g["coarse_D" if lvl == 1 else "l2_coarse_D"], g["coarse_clover" if lvl == 1 else "l2_coarse_clover"], level=lvl)
    ncols = 7 if lvl == 1 else 24
    hs = columns(ctx, lvl, g[f"l{lvl}_apply_in"], ncols, 500)
    ins = [ctx.vector(lvl, 32).upload(h) for h in hs]; outs = [ctx.vector(lvl, 32) for _ in hs]
    ctx.coarse_apply_many(outs, ins)
    assert relerr(outs[0].download(), g[f"l{lvl}_apply_out"]) < TOL_KERNEL
    one = ctx.vector(lvl, 32)
    for c in range(ncols):
        ctx.coarse_apply(one, ins[c])
        ref = one.download(); got = outs[c].download()
        if c == 2:
            assert np.all(got == 0.0)
        else:
            assert relerr(got, ref) < TOL_KERNEL, c
    for v in ins + outs + [one]:
        v.free()


def test_transfer_between_the_coarse_levels(ref3):
    g, ctx = ref3
    f = ctx.vector(1, 32).upload(g["l1_restrict_in"]); c = ctx.vector(2, 32)
    ctx.restrict(c, f)
    assert relerr(c.download(), g["l1_restrict_out"]) < TOL_KERNEL
    c.upload(g["l1_interpolate_in"])
    ctx.interpolate(f, c)
    assert relerr(f.download(), g["l1_interpolate_out"]) < TOL_KERNEL
    f.free(); c.free()


@pytest.mark.parametrize("unfused", [False, True], ids=["fused-block-solver", "step-by-step"])
def test_schwarz_smoother_of_the_intermediate_level(unfused, monkeypatch):
    """red_black_schwarz on coarse_block_operator with local_minres (src/schwarz_generic.c:1260-1431, src/coarse_operator_generic.c:
    208-235) against the reference's dumps: blocks of 16 sites and, on the second fixture, of TWO sites (fewer sites than the fused
    block solver has wavefronts)"""
    if unfused:
        monkeypatch.setenv("DDAMG_COARSE_SAP_UNFUSED", "1")
    for name in ("ref_8x8_3lvl_small.npz", "ref_16x8_3lvl_prod.npz"):
        g, ctx = make_ctx(name)
        ctx.set_coarse_operator(g["coarse_D"], g["coarse_clover"], level=1)
        eta = ctx.vector(1, 32).upload(g["l1_smoother_eta"]); phi = ctx.vector(1, 32)
        for cyc in (1, 2, 3):
            ctx.smoother(phi, eta, cyc, initial_guess_zero=True)
            assert relerr(phi.download(), g[f"l1_smoother_nores_out_c{cyc}"]) < TOL_SWEEP, (name, cyc)
        phi.upload(g["l1_smoother_phi0"])
        ctx.smoother(phi, eta, 2, initial_guess_zero=False)
        assert relerr(phi.download(), g["l1_smoother_res_out_c2"]) < TOL_SWEEP, name
        ctx.close()


@pytest.mark.parametrize("ncols", [5, 17, 32])
def test_schwarz_smoother_of_many_right_hand_sides(ref3, ncols):
    """cm_block_minres_kernel: column 0 against the reference's dumps, every column against the one-vector smoother; with 17 and 32
    columns the second half of the columns (the workgroups of col0 = 16) carries data"""
    g, ctx = ref3
    ctx.set_coarse_operator(g["coarse_D"], g["coarse_clover"], level=1)
    hs = columns(ctx, 1, g["l1_smoother_eta"], ncols, 600)
    etas = [ctx.vector(1, 32).upload(h) for h in hs]; phis = [ctx.vector(1, 32) for _ in hs]
    one = ctx.vector(1, 32)
    for cyc in (1, 2, 3):
        ctx.smoother_many(phis, etas, cyc, initial_guess_zero=True)
        assert relerr(phis[0].download(), g[f"l1_smoother_nores_out_c{cyc}"]) < TOL_SWEEP, cyc
        for c in range(1, ncols):
            ctx.smoother(one, etas[c], cyc, initial_guess_zero=True)
            ref = one.download(); got = phis[c].download()
            assert (np.all(got == 0.0) if c == 2 else relerr(got, ref) < TOL_SWEEP), (cyc, c)
    p0 = columns(ctx, 1, g["l1_smoother_phi0"], ncols, 700)
    for c in range(ncols):
        phis[c].upload(p0[c])
    ctx.smoother_many(phis, etas, 2, initial_guess_zero=False)
    assert relerr(phis[0].download(), g["l1_smoother_res_out_c2"]) < TOL_SWEEP
    for c in range(1, ncols):
        one.upload(p0[c])
        ctx.smoother(one, etas[c], 2, initial_guess_zero=False)
        got = phis[c].download()
        assert (np.all(got == 0.0) if c == 2 else relerr(got, one.download()) < TOL_SWEEP), c
    for v in etas + phis + [one]:
        v.free()


@pytest.mark.parametrize("ncols", [6, 17, 32])
def test_vcycle_of_the_intermediate_level(ref3, ncols):
    """vcycle_float on level 1 (restriction, coarsest odd-even solve, interpolation, smoother) against the reference's dump, one
    vector at a time and for many right-hand sides in lockstep; with 17 and 32 columns cm_restrict_kernel, cm_interpolate_kernel
    and the lockstep solve carry data in the second half of the columns"""
    g, ctx = ref3
    ctx.set_coarse_operator(g["coarse_D"], g["coarse_clover"], level=1)
    ctx.set_coarse_operator(g["l2_coarse_D"], g["l2_coarse_clover"], level=2)
    hs = columns(ctx, 1, g["l1_vcycle_eta"], ncols, 800)
    etas = [ctx.vector(1, 32).upload(h) for h in hs]; phis = [ctx.vector(1, 32) for _ in hs]
    one = ctx.vector(1, 32)
    ctx.vcycle(one, etas[0])
    assert relerr(one.download(), g["l1_vcycle_out"]) < 2e-4
    ctx.vcycle_many(phis, etas)
    assert relerr(phis[0].download(), g["l1_vcycle_out"]) < 2e-4
    for c in range(1, ncols):
        ctx.vcycle(one, etas[c])
        ref = one.download(); got = phis[c].download()
        # (the coarsest solves stop at 5e-2: where a column's stopping test falls on the rounding of the operator kernel the two
        # take a different number of steps, and agree to the accuracy of that solve only)
        assert (np.all(got == 0.0) if c == 2 else relerr(got, ref) < 5e-2), c
    for v in etas + phis + [one]:
        v.free()


@pytest.mark.parametrize("ncols", [6, 17, 32])
def test_kcycles_of_many_right_hand_sides_in_lockstep(ref3, ncols):
    """CoarseMulti::kcycle: FGMRES(5) x 2 with the level's V-cycle as preconditioner, every column its own recurrence, against the
    one-at-a-time K-cycle (Gmres<T>::solve): iteration counts (one more or less where a stopping test falls on the rounding) and the
    defining property -- the residual of every column below the K-cycle tolerance or the iteration budget spent"""
    g, ctx = ref3
    ctx.set_coarse_operator(g["coarse_D"], g["coarse_clover"], level=1)
    ctx.set_coarse_operator(g["l2_coarse_D"], g["l2_coarse_clover"], level=2)
    hs = columns(ctx, 1, g["l1_vcycle_eta"], ncols, 900)
    bs = [ctx.vector(1, 32).upload(h) for h in hs]; xs = [ctx.vector(1, 32) for _ in hs]
    one = ctx.vector(1, 32); Dx = ctx.vector(1, 32)
    its = ctx.kcycle_many(xs, bs)
    for c in range(ncols):
        if c == 2:
            assert its[c] == 0 and np.all(xs[c].download() == 0.0)
            continue
        it1 = ctx.kcycle(one, bs[c])
        assert abs(its[c] - it1) <= 1, (c, its, it1)
        ctx.coarse_apply(Dx, xs[c])
        res = np.linalg.norm(Dx.download() - hs[c]) / np.linalg.norm(hs[c])
        ctx.coarse_apply(Dx, one)
        res1 = np.linalg.norm(Dx.download() - hs[c]) / np.linalg.norm(hs[c])
        assert res < max(0.11, 1.5 * res1), (c, res, res1)
        if its[c] == it1:
            assert relerr(xs[c].download(), one.download()) < 5e-2, c
    for v in bs + xs + [one, Dx]:
        v.free()
