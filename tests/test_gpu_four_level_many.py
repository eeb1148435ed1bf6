"""GPU tests (-m gpu) of the many-vector path on a FOUR-level hierarchy: a CoarseMulti per intermediate level, the K-cycles of
level 2 nested in the V-cycles of level 1 for all columns at once (coarse_multi.hip, mg.cpp multi_*), the setup that runs through
it, and the *_many entry points on both intermediate levels.

The hierarchy is the smallest four levels allow with even block counts and an even coarsest extent: 16^4 -> 8^4 -> 4^4 -> 2^4,
2^4 blocks everywhere, 20 / 24 / 28 test vectors (40 / 48 / 56 dof per site), the parameters of tools/four_level_check.py on the
seeded field the reference itself was run on (tests/golden/ref_16x16_4lvl.json).  The kernel-level tests run on the hierarchy of
the initial setup alone: they need a hierarchy, not a converged one.  Every many-vector result is held against the one-vector
entry point of the same context; tolerances are those of tests/test_gpu_three_levels.py."""
import json, os, subprocess, sys
import numpy as np
import pytest
from conftest import relerr, splitmix_uniform
from ddalphaamg_amd import api
import ddalphaamg_amd as dd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "tools"))
pytestmark = pytest.mark.gpu

TOL_SWEEP = 1e-4
TOL_INNER = 5e-2            # where loose inner solves (K-cycle 1e-1, coarsest 5e-2) sit in between
GAUGE_EPS, GAUGE_SEED = 0.35, 20260101
SCALE = 1e6
# coarse_tol of the hand-over tests, tightened until the one-vector coarsest solve needs more steps than the 24 vectors the
# lockstep basis holds.  Measured on the MI355X on the hierarchy of the initial setup, three random level-3 vectors: 8 iterations at
# 1e-6, 10 to 13 at 1e-8, and 103 / 54 / 103 at 1e-9 -- the coarsest operator of this small lattice is well conditioned, so only a
# tolerance below what fp32 Arnoldi reaches in one cycle (the estimate stalls, the restart at 100 recomputes the residual) gets
# past 24.  After one bootstrap iteration 1e-8 is past it as well (70 / 16 / 37): the setup count below uses that, a third of the
# run time of 1e-9.
TIGHT_COARSE_TOL = 1e-9
TIGHT_SETUP_COARSE_TOL = 1e-8


def params(**kw):
    p = api.default_params(); p.num_levels = 4
    for mu in range(4):
        for d in range(4):
            p.local_lattice[d][mu] = 16 >> d; p.block_lattice[d][mu] = 2
    for d in range(3):
        p.num_vect[d] = 20 + 4 * d; p.post_smooth_iter[d] = 2; p.block_iter[d] = 4; p.setup_iter[d] = [3, 2, 2][d]
    p.restart, p.max_restart, p.tol = 50, 20, 1e-10
    p.coarse_iter, p.coarse_restart, p.coarse_tol = 100, 5, 5e-2
    p.mixed_precision, p.method, p.m0, p.csw = 1, 2, -0.3, 1.0
    p.test_vector_rng, p.rng_seed = 1, 3
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def make_ctx(setup_iterations=0, **kw):
    import synth
    ctx = dd.Context(params(**kw))
    ctx.set_gauge(synth.synth_gauge([16] * 4, GAUGE_EPS, GAUGE_SEED), anti_pbc=True)
    ci = ctx.setup(setup_iterations)
    return ctx, ci


@pytest.fixture(scope="module")
def hier():
    ctx, _ = make_ctx(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def deep():
    """the same hierarchy with the K-cycles of both intermediate levels asked for 1e-4 instead of 1e-1.  On the hierarchy of the
    initial setup the smoother alone brings a random right-hand side below 0.1, so every K-cycle above stops after ONE step
    (measured); here the level-1 recurrence takes three steps (measured) with a level-2 K-cycle of several steps inside each,
    and a column that is zero or has stopped is masked out of V-cycles that others still run"""
    ctx, _ = make_ctx(0, kcycle_tol=1e-4)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def tight():
    ctx, _ = make_ctx(0, coarse_tol=TIGHT_COARSE_TOL)
    yield ctx
    ctx.close()


def vec(ctx, lvl, seed):
    return splitmix_uniform(ctx.volume(lvl) * ctx.ndof(lvl) * 2, seed).reshape(ctx.volume(lvl), ctx.ndof(lvl), 2)


def columns(ctx, lvl, ncols, seed, twin=False):
    """ncols host vectors of level lvl: distinct seeds per column, column 2 zero, column 1 scaled by 1e6 (twin: 1e6 x column 0)"""
    hs = [vec(ctx, lvl, seed + c) for c in range(ncols)]
    hs[1] = SCALE * (hs[0] if twin else hs[1])
    if ncols > 2:
        hs[2] = np.zeros_like(hs[0])
    return hs


def put(ctx, lvl, hs):
    return [ctx.vector(lvl, 32).upload(h) for h in hs]


def free(*lists):
    for l in lists:
        for v in l:
            v.free()


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncols", [2, 17, 32])
@pytest.mark.parametrize("lvl", [1, 2])
def test_operator_and_smoother_on_both_intermediate_levels(hier, lvl, ncols):
    """cm_apply_op_kernel and cm_block_minres_op_kernel behind coarse_apply_many / smoother_many on level 1 (40 dof) AND level 2
    (48 dof) of four levels: every column against the one-vector kernel, the zero column exactly zero.  Refused before this
    hierarchy depth was covered."""
    ctx = hier
    hs = columns(ctx, lvl, ncols, 1100 + 100 * lvl)
    ins = put(ctx, lvl, hs); outs = [ctx.vector(lvl, 32) for _ in hs]; one = ctx.vector(lvl, 32)
    ctx.coarse_apply_many(outs, ins)
    for c in range(ncols):
        ctx.coarse_apply(one, ins[c])
        got = outs[c].download()
        if c == 2:
            assert np.all(got == 0.0)
        else:
            e = relerr(got, one.download()); print("apply", lvl, ncols, c, e)
            assert e < TOL_SWEEP, (c, e)
    guess = columns(ctx, lvl, ncols, 1500 + 100 * lvl)
    for cyc in (1, 2):
        for from_zero in (True, False):
            if not from_zero:
                for c in range(ncols):
                    outs[c].upload(guess[c])
            ctx.smoother_many(outs, ins, cyc, initial_guess_zero=from_zero)
            for c in range(ncols):
                if not from_zero:
                    one.upload(guess[c])
                ctx.smoother(one, ins[c], cyc, initial_guess_zero=from_zero)
                got = outs[c].download()
                if c == 2:
                    assert np.all(got == 0.0)        # zero right-hand side and zero guess: the smoother leaves zero
                else:
                    e = relerr(got, one.download()); print("smoother", lvl, ncols, cyc, from_zero, c, e)
                    assert e < TOL_SWEEP, (cyc, from_zero, c, e)
    free(ins, outs, [one])


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncols", [6, 17])
@pytest.mark.parametrize("lvl", [2, 1], ids=["level2-next-coarsest", "level1-nested"])
def test_vcycle_many_on_both_intermediate_levels(hier, lvl, ncols):
    """vcycle_many on level 2 (restriction, coarsest solves in lockstep, interpolation, smoother) and on level 1, where the
    K-cycles of level 2 run for all columns inside the V-cycle: every column against vcycle to the accuracy of the loose inner
    solves (the argument of test_vcycle_of_the_intermediate_level), the zero column exactly zero"""
    ctx = hier
    hs = columns(ctx, lvl, ncols, 2100 + 100 * lvl)
    etas = put(ctx, lvl, hs); phis = [ctx.vector(lvl, 32) for _ in hs]; one = ctx.vector(lvl, 32)
    ctx.vcycle_many(phis, etas)
    for c in range(ncols):
        ctx.vcycle(one, etas[c])
        got = phis[c].download()
        if c == 2:
            assert np.all(got == 0.0)
        else:
            e = relerr(got, one.download()); print("vcycle", lvl, ncols, c, e)
            assert e < TOL_INNER, (c, e)
    free(etas, phis, [one])


# 3 ------------------------------------------------------------------------------------------------------------------------
def check_kcycles(ctx, hs, its, xs, one, Dx):
    """the criterion of test_kcycles_of_many_right_hand_sides_in_lockstep, plus the scaled twin (column 1 = 1e6 x column 0)"""
    sols = {}
    for c in range(len(hs)):
        got = xs[c].download()
        if c == 2:
            assert its[c] == 0 and np.all(got == 0.0)
            continue
        b = ctx.vector(1, 32).upload(hs[c])
        it1 = ctx.kcycle(one, b); b.free()
        ctx.coarse_apply(Dx, xs[c])
        res = np.linalg.norm(Dx.download() - hs[c]) / np.linalg.norm(hs[c])
        ctx.coarse_apply(Dx, one)
        res1 = np.linalg.norm(Dx.download() - hs[c]) / np.linalg.norm(hs[c])
        print("kcycle", len(hs), c, its[c], it1, res, res1)
        assert abs(its[c] - it1) <= 1, (c, its, it1)
        assert res < max(0.11, 1.5 * res1), (c, res, res1)
        if its[c] == it1:
            assert relerr(got, one.download()) < TOL_INNER, c
        sols[c] = got
    assert its[1] == its[0], its
    e = relerr(sols[1], SCALE * sols[0]); print("scaled twin", e)
    assert e < 1e-4, e


@pytest.mark.parametrize("ncols", [6, 17, 32])
@pytest.mark.parametrize("which", ["hier", "deep"], ids=["kcycle-tol-1e-1", "kcycle-tol-1e-4"])
def test_kcycles_of_level_1_with_the_kcycles_of_level_2_nested(request, which, ncols):
    """CoarseMulti::kcycle on level 1 whose V-cycle runs CoarseMulti::kcycle on level 2: two nested lockstep FGMRES recurrences,
    each with its own slab, against the one-at-a-time K-cycle; with the issue's parameters (one step per K-cycle on this
    hierarchy) and with K-cycles of several steps on both levels"""
    ctx = request.getfixturevalue(which)
    hs = columns(ctx, 1, ncols, 3100, twin=True)
    bs = put(ctx, 1, hs); xs = [ctx.vector(1, 32) for _ in hs]; one = ctx.vector(1, 32); Dx = ctx.vector(1, 32)
    its = ctx.kcycle_many(xs, bs)
    check_kcycles(ctx, hs, its, xs, one, Dx)
    free(bs, xs, [one, Dx])


# 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["hier", "deep"], ids=["kcycle-tol-1e-1", "kcycle-tol-1e-4"])
def test_a_column_does_not_depend_on_the_other_columns(request, which):
    """the level-1 K-cycle of one right-hand side bit for bit whatever the other columns hold -- other seeds, a zero, a scaled
    one -- and at index 3 as at index 19: no activity mask and no batch slot leaks between columns across the nested recurrences"""
    ctx = request.getfixturevalue(which)
    t = vec(ctx, 1, 4000)
    a = [vec(ctx, 1, 4100 + c) for c in range(20)]; a[3] = t
    b = [vec(ctx, 1, 4200 + c) for c in range(24)]; b[19] = t; b[3] = np.zeros_like(t); b[5] = SCALE * b[5]; b[20] = 1e-6 * b[20]
    res = []
    for hs, idx in ((a, 3), (b, 19)):
        bs = put(ctx, 1, hs); xs = [ctx.vector(1, 32) for _ in hs]
        its = ctx.kcycle_many(xs, bs)
        res.append((its[idx], xs[idx].download()))
        free(bs, xs)
    print("independence", res[0][0], res[1][0], relerr(res[0][1], res[1][1]))
    assert res[0][0] == res[1][0] and res[0][0] > (1 if which == "deep" else 0)
    assert np.array_equal(res[0][1], res[1][1])


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_hand_over_through_both_levels(tight):
    """a coarsest column that needs more than the 24 vectors of the lockstep basis goes through the one-at-a-time solver, reached
    from a level-2 K-cycle inside a level-1 K-cycle.  With coarse_tol = 1e-9 the one-vector coarsest solve of a random level-3
    vector takes 103 iterations (seed 5000, MI355X), so every coarsest column of every V-cycle below is handed over."""
    ctx = tight
    b3 = ctx.vector(3, 32).upload(vec(ctx, 3, 5000)); x3 = ctx.vector(3, 32)
    it3 = ctx.coarse_solve(x3, b3)
    print("coarsest iterations at coarse_tol", TIGHT_COARSE_TOL, ":", it3)
    free([b3, x3])
    assert it3 > 24, it3
    ncols = 4
    hs = columns(ctx, 1, ncols, 5100, twin=True)
    bs = put(ctx, 1, hs); xs = [ctx.vector(1, 32) for _ in hs]; one = ctx.vector(1, 32); Dx = ctx.vector(1, 32)
    its = ctx.kcycle_many(xs, bs)
    check_kcycles(ctx, hs, its, xs, one, Dx)
    free(bs, xs, [one, Dx])


def test_coarsest_iterations_are_counted_once():
    """the coarsest iterations one bootstrap iteration reports with coarse_tol = 1e-8, where columns are handed over: lockstep counts
    plus hand-over counts against the sum over the one-vector runs of the same setup -- the one-at-a-time path, which a context
    with mixed_precision = 2 takes (its K-cycles read D*phi from the smoother instead of applying the operator: the same
    arithmetic up to rounding).  A count taken twice on the way up through two levels would double it; 15 % covers the
    iterations that move with the rounding (measured: 51803 against 49667)."""
    many, ci_many = make_ctx(1, coarse_tol=TIGHT_SETUP_COARSE_TOL)
    many.close()
    one, ci_one = make_ctx(1, coarse_tol=TIGHT_SETUP_COARSE_TOL, mixed_precision=2)
    one.close()
    print("coarsest iterations of setup(1): many", ci_many, "one vector at a time", ci_one)
    assert ci_one > 0 and abs(ci_many - ci_one) <= 0.15 * ci_one, (ci_many, ci_one)


# 6 ------------------------------------------------------------------------------------------------------------------------
CHILD = """
import sys, json, hashlib, numpy as np
sys.path.insert(0, {repo!r}); sys.path.insert(0, {here!r})
import test_gpu_four_level_many as t
b = np.zeros((16 ** 4, 12, 2)); b[..., 0] = 1.0
for run in range(2):
    ctx, ci = t.make_ctx(3)
    x, it, cit, rr = ctx.solve(b, 1e-10)
    Dx = ctx.vector(0, 64); xv = ctx.vector(0, 64).upload(x)
    ctx.dirac_apply(Dx, xv)
    true_rr = float(np.linalg.norm(b - Dx.download()) / np.linalg.norm(b))
    print("RESULT", json.dumps(dict(it=it, cit=cit, rr=rr, true_rr=true_rr, ci=ci, sha=hashlib.sha256(x.tobytes()).hexdigest())))
    ctx.close()
"""


def test_setup_takes_the_path_and_reproduces_the_reference():
    """setup(3) and a solve in a child process under DDAMG_SETUP_TIMING: both intermediate levels announce the many-vector path,
    no level falls back to one vector at a time, the solve takes the reference's iteration count (+-1, other random test vectors)
    to a true residual below 1e-10, and a second setup + solve gives the same bits"""
    ref = json.load(open(os.path.join(REPO, "tests", "golden", "ref_16x16_4lvl.json")))
    env = dict(os.environ, DDAMG_SETUP_TIMING="1")
    r = subprocess.run([sys.executable, "-c", CHILD.format(repo=REPO, here=HERE)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    print(r.stderr[-3000:])
    assert "one vector at a time" not in r.stderr, r.stderr[-4000:]
    for lvl in (1, 2):
        assert f"[ddamg setup] level {lvl} all vectors at once" in r.stderr, r.stderr[-4000:]
    runs = [json.loads(l.split(" ", 1)[1]) for l in r.stdout.splitlines() if l.startswith("RESULT")]
    print(runs, "reference", ref["iterations"])
    assert len(runs) == 2
    for q in runs:
        assert abs(q["it"] - ref["iterations"]) <= 1, (q, ref["iterations"])
        assert q["rr"] < 1e-10 and q["true_rr"] < 1e-10, q
    assert runs[0] == runs[1]


# 7 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", [dict(mixed_precision=2), dict(kcycle=0)], ids=["mixed-precision-2", "no-kcycle"])
def test_fallbacks_are_still_there(switch):
    """what the many-vector path does not cover sets up and solves one vector at a time as before; the *_many calls that need the
    batched path return an error through ddamg_hip_last_error, and everything the context held is released with it"""
    before = api.memory_in_use()
    ctx, _ = make_ctx(2, **switch)
    V = 16 ** 4
    b = np.zeros((V, 12, 2)); b[..., 0] = 1.0
    x, it, cit, rr = ctx.solve(b, 1e-10)
    print("fallback", switch, it, cit, rr)
    assert rr < 1e-10 and it < 40
    hs = columns(ctx, 1, 4, 7000)
    bs = put(ctx, 1, hs); xs = [ctx.vector(1, 32) for _ in hs]
    refused = [lambda: ctx.kcycle_many(xs, bs), lambda: ctx.vcycle_many(xs, bs)]          # level 1: the K-cycles of level 2 inside
    if "mixed_precision" in switch:
        refused += [lambda: ctx.coarse_apply_many(xs, bs), lambda: ctx.smoother_many(xs, bs, 1)]
    for call in refused:
        with pytest.raises(api.DDAMGError, match="shape not covered"):
            call()
    if "kcycle" in switch:
        # operator and smoother of a level need no K-cycle below them
        ctx.coarse_apply_many(xs, bs)
        one = ctx.vector(1, 32); ctx.coarse_apply(one, bs[0])
        assert relerr(xs[0].download(), one.download()) < TOL_SWEEP
        one.free()
    free(bs, xs)
    ctx.close()
    assert api.memory_in_use() == before
