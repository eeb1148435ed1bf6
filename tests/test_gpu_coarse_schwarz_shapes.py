"""The Schwarz smoother of an intermediate level (CoarseSap<T>::smooth, coarse_mg.hip) at every block shape and dof count (-m gpu)
against the fp64 reference `mg_oracle.Schwarz` with plain-block MinRes on the operator's matrix (tests/coarse_schwarz_reference.py;
pinned on the CPU in tests/test_coarse_schwarz_reference.py).

Shapes (coarse_schwarz_reference.SHAPES): level-1 blocks of 2, 4, 8, 16, 24, 32, 64 and 128 sites on the smallest level-1 lattices
with an even number of blocks per direction and, up to 32 sites, more than two blocks in one direction; the dof counts at which
the fused block solver changes its path (coarse_schwarz_reference.path).  Three levels: the fine lattice is twice the level-1
lattice with 2^4 blocks and n / 2 test vectors, the level-2 lattice is the lattice of the level-1 aggregates (= blocks, but for
the 24-site blocks).  No setup: the fine level only has to exist, the level-1 operator is a well-conditioned random one
(random_couplings) installed by set_coarse_operator(level=1).  Four MinRes steps.

fp32 (mixed_precision 1) and fp64 (0), the additive, red-black and sixteen-colour schedule, 1 and 3 cycles from zero and 2 cycles
from a guess; every case that the launch rule calls fused a second time step by step (DDAMG_COARSE_SAP_UNFUSED, read when the
context is created).

Bars: fp64 1e-11 of the norm; fp32 ten times the largest spread of the fp32 restatements around the fp64 reference over all cases
(coarse_schwarz_reference.LARGEST_SPREAD, recomputed by the CPU test), which lies below TOL_SWEEP = 1e-4, the bar this smoother has in
test_gpu_three_levels.py.

Isolation: phi (from zero) is filled with NaN and the vectors allocated right before and after it with a sentinel before every
call; eta must come back as it went in.

Process boundary: the same lattices through the RCCL self-exchange (the process its own neighbour in the directions of the split),
which runs coarse_halo_pack_kernel and the halo branches of coarse_site_kernel under the smoother."""
import os
import numpy as np
import pytest
from ddalphaamg_amd import api
import ddalphaamg_amd as dd
import coarse_schwarz_reference as cr
from test_gpu_intermediate_half import lossless_operator

pytestmark = pytest.mark.gpu

SENTINEL = 30000.5
KNOB = "DDAMG_COARSE_SAP_UNFUSED"


def params(name, n, mp, method, split=""):
    B, L1, A = cr.geometry(name, n)
    p = api.default_params(); p.num_levels = 3
    for mu in range(4):
        p.local_lattice[0][mu] = 2 * L1[mu]; p.block_lattice[0][mu] = 2
        p.local_lattice[1][mu] = L1[mu]; p.block_lattice[1][mu] = B[mu]
        p.local_lattice[2][mu] = L1[mu] // A[mu]
        if str(mu) in split:
            p.process_grid[mu] = -1
    p.num_vect[0], p.num_vect[1] = n // 2, 4
    p.post_smooth_iter[0] = p.post_smooth_iter[1] = 2; p.block_iter[0] = 4; p.block_iter[1] = cr.BLOCK_ITER
    p.setup_iter[0] = p.setup_iter[1] = 1
    p.restart, p.max_restart, p.tol = 20, 5, 1e-10
    p.coarse_iter, p.coarse_restart, p.coarse_tol = 20, 2, 5e-2
    p.kcycle, p.kcycle_restart, p.kcycle_max_restart, p.kcycle_tol = 1, 5, 2, 1e-1
    p.mixed_precision, p.method, p.odd_even = mp, method, 1
    p.m0, p.csw = -0.1, 1.0
    return p


_gauges = {}


def gauge(L0):
    key = tuple(L0)
    if key not in _gauges:
        _gauges.clear()                 # one lattice at a time
        V = int(np.prod(L0))
        _gauges[key] = np.zeros((V, 4, 9, 2)); _gauges[key][:, :, [0, 4, 8], 0] = 1.0      # the level only has to exist: unit links
    return _gauges[key]


def context(name, n, mp, method, unfused=False, split="", operator=None):
    """a context carrying the level-1 operator of the case; the environment is put back before returning"""
    old = os.environ.get(KNOB)
    if unfused:
        os.environ[KNOB] = "1"
    else:
        os.environ.pop(KNOB, None)
    try:
        ctx = dd.Context(params(name, n, mp, method, split))
    finally:
        if old is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = old
    if split:
        ctx.comm_init_rccl(api.rccl_unique_id())
    ctx.set_gauge(gauge([2 * v for v in cr.geometry(name, n)[1]]), anti_pbc=True)
    ctx.set_coarse_operator(*(operator or cr.operator(name, n)), level=1)
    return ctx


def as_stored(a, prec):
    return a.astype(np.float32).astype(np.float64) if prec == 32 else a


def smooth(ctx, eta, phi0, cycles, guess):
    """one level-1 smoother call, from zero or from the guess, with the isolation checks; returns phi [V][n][2]"""
    prec = ctx.vprec()
    e = ctx.vector(1, prec).upload(eta)
    before = ctx.vector(1, prec); phi = ctx.vector(1, prec); after = ctx.vector(1, prec)
    for g in (before, after):
        g.upload(np.full(eta.shape, SENTINEL))
    phi.upload(phi0 if guess else np.full(eta.shape, np.nan))
    ctx.smoother(phi, e, cycles, initial_guess_zero=not guess)
    out = phi.download()
    assert np.array_equal(e.download(), as_stored(eta, prec)), "eta changed"
    for g in (before, after):
        assert np.all(g.download() == SENTINEL), "a vector next to phi changed"
    for v in (e, before, phi, after):
        v.free()
    return out


def bar_of(prec):
    return cr.fp32_bar() if prec == 32 else cr.fp64_bar()


def case_id(c):
    return f"{c[0]}-n{c[1]}"


# ---- every shape x n x precision x method x start, fused and step by step --------------------------------------------------------
@pytest.fixture(scope="module", params=[(name, n, mp) for name, n in cr.CASES for mp in (1, 0)], ids=lambda p: f"{case_id(p)}-mp{p[2]}")
def runs(request):
    """out[(method, form)][start] and, for red-black, out[(2, form)]["guard"]: the outputs of every smoother call of a case"""
    name, n, mp = request.param
    prec = 32 if mp else 64
    fused = cr.path(cr.geometry(name, n)[0], n, prec)["fused"]
    eta, phi0 = cr.vectors(name, n)
    out = {}
    for method in cr.METHODS:
        for form in (["fused"] if fused else []) + ["step by step"]:
            ctx = context(name, n, mp, method, unfused=form == "step by step")
            assert ctx.vprec() == prec
            out[(method, form)] = {s: smooth(ctx, eta, phi0, *cr.STARTS[s]) for s in cr.STARTS}
            if method == 2:
                out[(method, form)]["guard"] = smooth(ctx, cr.guard_eta(name, n), phi0, 1, False)
            ctx.close()
    yield name, n, prec, fused, out
    if not mp:
        cr.forget(name, n)


def test_smoother_vs_reference(runs):
    name, n, prec, fused, out = runs
    bar = bar_of(prec)
    print(f"coarse schwarz {name} n {n} fp{prec}: expected path {cr.path_name(cr.geometry(name, n)[0], n, prec)}")
    assert cr.fp32_bar() <= cr.TOL_SWEEP
    bad = []
    for (method, form), res in out.items():
        dist = {s: cr.relerr(cr.cvec(res[s]), cr.reference(name, n, method, s, prec)) for s in cr.STARTS}
        print(f"coarse schwarz {name} n {n} fp{prec} method {method} {form}: " + ", ".join(f"{s} {d:.3e}" for s, d in dist.items()) + f" (bar {bar:.2e})")
        bad += [(method, form, s, d) for s, d in dist.items() if not d < bar]
    assert not bad, (bar, bad)


def test_both_block_solvers(runs):
    """the two forms against each other (both are held to the bar against the reference above)"""
    name, n, prec, fused, out = runs
    if not fused:
        print(f"coarse schwarz {name} n {n} fp{prec}: step by step only")
        assert all(form == "step by step" for _, form in out)
        return
    for method in cr.METHODS:
        a, b = out[(method, "fused")], out[(method, "step by step")]
        d = {s: cr.relerr(a[s], b[s]) for s in a}
        print(f"coarse schwarz {name} n {n} fp{prec} method {method} fused vs step by step: " + ", ".join(f"{s} {v:.3e}" for s, v in d.items()))
        for s, v in d.items():
            assert v < 2 * bar_of(prec), (method, s, v)


def test_eps_guard(runs):
    """eta zero on a block of either colour, one red-black cycle from zero: <Dr,Dr> = 0 there, alpha would be 0/0 without the guard"""
    name, n, prec, fused, out = runs
    ref = cr.guard_reference(name, n, prec)
    for (method, form), res in out.items():
        if method != 2:
            continue
        got = res["guard"]
        d = cr.relerr(cr.cvec(got), ref)
        print(f"coarse schwarz {name} n {n} fp{prec} eps guard, {form}: {d:.3e} (bar {bar_of(prec):.2e})")
        assert np.all(np.isfinite(got)), form
        assert d < bar_of(prec), (form, d)


# ---- 16-bit couplings --------------------------------------------------------------------------------------------------------
HALF_CASES = [("2", 48), ("8", 48), ("8", 56), ("16", 16), ("16", 40), ("16", 48), ("16", 56), ("32-x", 16), ("32-x", 40)]


@pytest.mark.parametrize("case", HALF_CASES, ids=case_id)
def test_sixteen_bit_couplings(case):
    """coarse_half_block_minres_kernel<2, 5, 6, 7> on an operator that the 16-bit format holds exactly: the 16-bit copy is the
    operator, so the fp32 bar applies unchanged -- against the fp64 reference of THAT operator"""
    from oracle import mg_oracle as mo
    name, n = case
    B, L1, _ = cr.geometry(name, n)
    p = cr.path(B, n, 32)
    assert p["fused"]
    D, cl = lossless_operator(*cr.operator(name, n))
    S = mo.Schwarz(L1, B, mo.coarse_matrix(L1, D, cl, n), cr.BLOCK_ITER, 2, ndof=n, odd_even=False, eps=cr.EPS[32])
    eta, phi0 = cr.vectors(name, n)
    ctx = context(name, n, 1, 2, operator=(D, cl))
    ctx.set_intermediate_storage(16)
    dist = {}
    for s, (cycles, guess) in cr.STARTS.items():
        ref = S.smooth(cr.cvec(eta), cycles, phi0=cr.cvec(phi0) if guess else None)
        dist[s] = cr.relerr(cr.cvec(smooth(ctx, eta, phi0, cycles, guess)), ref)
    ctx.close()
    print(f"coarse schwarz 16-bit {name} n {n} (NT {p['NT']}, {p['half']} resident per wavefront, nres {p['nres']}): "
          + ", ".join(f"{s} {d:.3e}" for s, d in dist.items()) + f" (bar {cr.fp32_bar():.2e})")
    for s, d in dist.items():
        assert d < cr.fp32_bar(), (s, d)


# ---- process boundary ------------------------------------------------------------------------------------------------------------
DIST_CASES = [("2", 48), ("4", 20), ("8", 48), ("16", 20), ("24", 20), ("32-t", 16), ("64", 16), ("128", 8)]      # one per block volume


def splits_of(name, n):
    B, L1, _ = cr.geometry(name, n)
    nblk = np.array(L1) // np.array(B)
    return ["23", "0123"] + ([str(int(np.argmax(nblk)))] if nblk.max() > 2 else [])


@pytest.fixture(scope="module", params=[(name, n, mp) for name, n in DIST_CASES for mp in (1, 0)], ids=lambda p: f"{case_id(p)}-mp{p[2]}")
def divided(request):
    """red-black, the three starts, undivided (split "") and through the self-exchange"""
    name, n, mp = request.param
    eta, phi0 = cr.vectors(name, n)
    out = {}
    for split in [""] + splits_of(name, n):
        ctx = context(name, n, mp, 2, split=split)
        out[split] = {s: smooth(ctx, eta, phi0, *cr.STARTS[s]) for s in cr.STARTS}
        ctx.close()
    yield name, n, mp, out
    if not mp:
        cr.forget(name, n)


def test_process_boundary_vs_reference(divided):
    name, n, mp, out = divided
    prec = 32 if mp else 64
    dist = {(split, s): cr.relerr(cr.cvec(out[split][s]), cr.reference(name, n, 2, s, prec)) for split in splits_of(name, n) for s in cr.STARTS}
    print(f"coarse schwarz divided {name} n {n} fp{prec}: " + ", ".join(f"{k[0]}/{k[1]} {d:.3e}" for k, d in dist.items()) + f" (bar {bar_of(prec):.2e})")
    for k, d in dist.items():
        assert d < bar_of(prec), (k, d)


def test_process_boundary_against_the_undivided_run(divided):
    name, n, mp, out = divided
    far = {(split, s): (cr.relerr(out[split][s], out[""][s]), int(np.count_nonzero(out[split][s] != out[""][s])))
           for split in splits_of(name, n) for s in cr.STARTS}
    print(f"coarse schwarz divided {name} n {n} mp{mp} from the undivided run: " + ", ".join(f"{k[0]}/{k[1]} {d:.3e} ({c} reals)" for k, (d, c) in far.items()))
    for s in cr.STARTS:
        assert np.all(np.isfinite(out[""][s]))
    for k, (d, c) in far.items():
        assert c == 0, f"split {k[0]}, {k[1]}: {d:.3e} from the undivided run, {c} reals differ"


# ---- refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [2, 3])
def test_an_odd_number_of_blocks_is_refused(method):
    """4x4x4x6 under 2^4 blocks: three blocks in X.  The multiplicative schedules need two colours that alternate around the
    lattice; CoarseSap::setup says so when the hierarchy is built (before the coarsest level refuses its odd extent)"""
    p = api.default_params(); p.num_levels = 3
    L1 = [4, 4, 4, 6]
    for mu in range(4):
        p.local_lattice[0][mu] = 2 * L1[mu]; p.block_lattice[0][mu] = 2
        p.local_lattice[1][mu] = L1[mu]; p.block_lattice[1][mu] = 2
        p.local_lattice[2][mu] = L1[mu] // 2
    p.num_vect[0], p.num_vect[1] = 4, 4
    p.block_iter[0] = p.block_iter[1] = 4
    p.mixed_precision, p.method, p.odd_even = 1, method, 1
    p.m0, p.csw = -0.1, 1.0
    ctx = dd.Context(p)
    vecs = []
    try:
        with pytest.raises(api.DDAMGError, match="multiplicative SAP needs an even number of blocks per direction"):
            ctx.set_gauge(gauge([2 * v for v in L1]), anti_pbc=True)
            vecs = [ctx.vector(1, 32), ctx.vector(1, 32)]
            vecs[0].upload(np.ones((int(np.prod(L1)), 8, 2)))
            ctx.smoother(vecs[1], vecs[0], 1, initial_guess_zero=True)
    finally:
        for v in vecs:
            v.free()
        ctx.close()
