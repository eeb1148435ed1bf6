"""GPU tests (-m gpu) of the matrix-core kernels that apply a coarse level to up to 32 right-hand sides at once
(coarse_lockstep.hip, coarse_multi.hip, mfma_tile.h), at every dof count and on both halves of the columns.

1. Exactly.  Couplings with integer parts in [-3, 3] and vectors with integer parts in [-4, 4]: every partial sum of a result
   component is an integer of magnitude at most 9 * 64 * 6 * 8 = 27 648 < 2^24, so fp32 in ANY summation order, and the fp32
   matrix instruction, must return the exact integer -- bit for bit, no tolerance.  The bound is asserted on the reference
   (coarse_reference.IntegerOperator) before anything is compared.  Coarsest level (two-level contexts, n = 4, 8, .., 64: the
   8x8-tile form of the couplings at n % 8 == 4, their A-operand copy at n % 8 == 0, one to four row tiles, the last one half
   empty at n = 8, 24, 40, 56) and intermediate level (three-level contexts, n = 8, 16, .., 64), with 2, 15, 16, 17, 31 and 32
   columns; the one-vector kernels (coarse_site_kernel<float / double, NT, *>, coarse_apply_once_kernel) against the same integers.

2. The Schwarz smoother of many columns on well-conditioned random operators at n = 8, 24, 40, 64, every column against the
   one-vector smoother, and column independence bit for bit: the result of a column depends neither on what the other columns
   hold nor on its index (lane r16 = c % 16 of the workgroup of half c / 16 -- moving a column from 3 to 19 keeps the lane).

The lattices.  Coarsest level: 4x4x4x6 (distinct neighbours in every direction, one extent no power of two) and 2x4x4x4 (forward
and backward neighbour coincide in the first direction).  Intermediate level: 4x4x4x12 over a coarsest lattice of 2x2x2x6 with
2^4 Schwarz blocks.  (A coarsest lattice of 2x2x2x3 under a 4x4x4x6 level cannot exist here: odd-even preconditioning refuses an
odd extent, and the many-column path needs odd-even.  For the same reason -- an even number of blocks in every direction,
CoarseMulti::available -- a colour always has a multiple of 8 blocks, so the tail of the block-to-workgroup map of
cm_block_minres_op_kernel cannot be reached through the library.)"""
import numpy as np
import pytest
from conftest import relerr, random_su3, splitmix_uniform
from coarse_reference import IntegerOperator
from coarse_schwarz_reference import random_operator     # well conditioned: MinRes on a Schwarz block never meets its eps guard
from ddalphaamg_amd import api
import ddalphaamg_amd as dd

pytestmark = pytest.mark.gpu

TOL_SWEEP = 1e-4          # the bound of test_gpu_three_levels.py for the many-column smoother against the one-vector smoother
NCOLS = [2, 15, 16, 17, 31, 32]
LATTICES = {"4x4x4x6": [4, 4, 4, 6], "2x4x4x4": [2, 4, 4, 4]}
L1 = [4, 4, 4, 12]        # the intermediate level of the three-level contexts
ZERO, UNIT = 32, 33       # columns of the pool behind the 32 random ones


_gauges = {}


def gauge(L0):
    key = tuple(L0)
    if key not in _gauges:
        V = int(np.prod(L0))
        _gauges[key] = random_su3(V * 4, 2718).reshape(V, 4, 9, 2)     # the level only has to exist
    return _gauges[key]


def two_level_ctx(Lc, nv, mixed_precision=1):
    p = api.default_params()
    p.num_levels = 2
    for mu in range(4):
        p.local_lattice[0][mu] = 2 * Lc[mu]; p.block_lattice[0][mu] = 2; p.local_lattice[1][mu] = Lc[mu]
    p.num_vect[0] = nv
    p.post_smooth_iter[0] = 2; p.block_iter[0] = 4; p.setup_iter[0] = 1
    p.restart, p.max_restart, p.tol = 20, 5, 1e-10
    p.coarse_iter, p.coarse_restart, p.coarse_tol = 20, 2, 5e-2
    p.mixed_precision, p.method, p.odd_even = mixed_precision, 2, 1
    p.m0, p.csw = -0.1, 1.0
    ctx = dd.Context(p)
    ctx.set_gauge(gauge([2 * v for v in Lc]), anti_pbc=True)
    return ctx


def three_level_ctx(nv0):
    p = api.default_params()
    p.num_levels = 3
    for mu in range(4):
        p.local_lattice[0][mu] = 2 * L1[mu]; p.block_lattice[0][mu] = 2
        p.local_lattice[1][mu] = L1[mu]; p.block_lattice[1][mu] = 2
        p.local_lattice[2][mu] = L1[mu] // 2
    p.num_vect[0], p.num_vect[1] = nv0, 4
    p.post_smooth_iter[0] = p.post_smooth_iter[1] = 2; p.block_iter[0] = p.block_iter[1] = 4
    p.setup_iter[0] = p.setup_iter[1] = 1
    p.restart, p.max_restart, p.tol = 20, 5, 1e-10
    p.coarse_iter, p.coarse_restart, p.coarse_tol = 20, 2, 5e-2
    p.kcycle, p.kcycle_restart, p.kcycle_max_restart, p.kcycle_tol = 1, 5, 2, 1e-1
    p.mixed_precision, p.method, p.odd_even = 1, 2, 1
    p.m0, p.csw = -0.1, 1.0
    ctx = dd.Context(p)
    ctx.set_gauge(gauge([2 * v for v in L1]), anti_pbc=True)
    return ctx


def integer_pool(V, n, seed):
    """34 columns [V][n][2]: 32 with integer parts in [-4, 4], a zero column, a unit entry at the last site and dof"""
    pool = np.zeros((34, V, n, 2))
    pool[:32] = np.random.default_rng(seed).integers(-4, 5, size=(32, V, n, 2))
    pool[UNIT, V - 1, n - 1, 0] = 1.0
    return pool


def selections(ncols):
    """the pool columns of a call of ncols columns: random ones, one zero, the unit entry in the LAST column (with 17 columns
    that is the first of the second half); two columns leave no room for all three, so they take two calls"""
    if ncols == 2:
        return [[0, ZERO], [UNIT, 1]]
    sel = list(range(ncols)); sel[1] = ZERO; sel[-1] = UNIT
    return [sel]


def assert_exact(got, ref, what):
    bad = int(np.count_nonzero(got != ref))
    assert bad == 0, f"{what}: {bad} of {ref.size} components differ from the integer result, the largest difference {np.abs(got - ref).max()}"


class Level:
    """a context whose level `lvl` carries an integer operator, the pool of integer columns with its int64 results, and 32 + 32
    device vectors of that level"""

    def __init__(self, ctx, lvl, Lc, seed, precision=32):
        self.ctx, self.lvl, self.Lc, self.precision = ctx, lvl, Lc, precision
        self.n, self.V = ctx.ndof(lvl), int(np.prod(Lc))
        self.op = IntegerOperator(self.n, Lc, seed)
        self.pool = integer_pool(self.V, self.n, seed + 1)
        self.self_ref, m0 = self.op.terms(self.pool, [0])
        self.hop_ref, m1 = self.op.terms(self.pool, range(1, 9))
        # what makes "bit for bit" the right criterion: no partial sum of any component, in any order, leaves the integers fp32 holds
        assert m0 + m1 + 4 < 2 ** 24, (m0, m1)
        self.ref = self.self_ref - self.hop_ref
        self.kind = None
        self.use_integer()
        self.ins = [ctx.vector(lvl, precision) for _ in range(32)]; self.outs = [ctx.vector(lvl, precision) for _ in range(32)]

    def use_integer(self):
        if self.kind != "integer":
            self.ctx.set_coarse_operator(self.op.D, self.op.cl, level=self.lvl)
            self.kind = "integer"

    def apply_many(self, cols, sentinel=7.0):
        k = len(cols)
        for v, h in zip(self.ins, cols):
            v.upload(h)
        for v in self.outs[:k]:
            v.upload(np.full((self.V, self.n, 2), sentinel))
        self.ctx.coarse_apply_many(self.outs[:k], self.ins[:k])
        return [v.download() for v in self.outs[:k]]

    def close(self):
        for v in self.ins + self.outs:
            v.free()
        self.ctx.close()


# ---- 1. the coarsest level: two-level contexts, n = 4, 8, ..., 64 ----------------------------------------------------------
@pytest.fixture(scope="module", params=[(lat, nv) for lat in LATTICES for nv in range(2, 33, 2)], ids=lambda p: f"{p[0]}-n{2 * p[1]}")
def coarsest(request):
    lat, nv = request.param
    lv = Level(two_level_ctx(LATTICES[lat], nv), 1, LATTICES[lat], seed=1000 + 10 * nv + len(lat))
    yield lv
    lv.close()


@pytest.mark.parametrize("ncols", NCOLS)
def test_coarsest_operator_of_many_columns_is_exact(coarsest, ncols):
    """ls_self_kernel / ls_hop_kernel (n % 8 == 4) and ls_self_op_kernel / ls_hop_op_kernel on the copy cm_relayout_kernel makes
    (n % 8 == 0), gather and scatter included: every component of every column"""
    lv = coarsest
    for sel in selections(ncols):
        got = lv.apply_many([lv.pool[c] for c in sel])
        for k, c in enumerate(sel):
            assert_exact(got[k], lv.ref[c], f"n = {lv.n}, {ncols} columns, column {k}")


def test_coarsest_operator_of_one_vector_is_exact(coarsest):
    """coarse_site_kernel<float, NT, MODE_FULL> for NT = 1 .. 8, padding included, on every column of the pool"""
    lv = coarsest
    for c in range(34):
        lv.ins[0].upload(lv.pool[c]); lv.outs[0].upload(np.full((lv.V, lv.n, 2), 7.0))
        lv.ctx.coarse_apply(lv.outs[0], lv.ins[0])
        assert_exact(lv.outs[0].download(), lv.ref[c], f"n = {lv.n}, column {c}")


def hop_and_self(lv):
    """ddamg_hip_coarse_hop for both parities, both signs, with and without accumulation onto an integer vector, and
    ddamg_hip_coarse_self_mul: the sites of the parity get the integer result, the others keep what they held"""
    ctx, odd = lv.ctx, lv.op.odd
    x, o = lv.pool[0], lv.pool[2]
    vi, vo = lv.ins[0].upload(x), lv.outs[0]
    for parity in (0, 1):
        mine = odd if parity else ~odd
        for sign in (1.0, -1.0):
            for acc in (False, True):
                vo.upload(o); ctx.coarse_hop(vo, vi, parity, sign, acc); y = vo.download()
                what = f"n = {lv.n}, hop parity {parity} sign {sign} accumulate {acc}"
                assert np.array_equal(y[~mine], o[~mine]), what + ": the other parity was touched"
                assert_exact(y[mine], (o * acc + sign * lv.hop_ref[0])[mine], what)
        vo.upload(o); ctx.coarse_self_mul(vo, vi, parity, False); y = vo.download()
        assert np.array_equal(y[~mine], o[~mine]), f"n = {lv.n}, self coupling, parity {parity}: the other parity was touched"
        assert_exact(y[mine], lv.self_ref[0][mine], f"n = {lv.n}, self coupling, parity {parity}")
    # the operator in two launches per parity: out = M0 x, out -= H x
    vo.upload(o)
    for parity in (0, 1):
        ctx.coarse_self_mul(vo, vi, parity, False); ctx.coarse_hop(vo, vi, parity, -1.0, True)
    assert_exact(vo.download(), lv.ref[0], f"n = {lv.n}, self coupling then hopping term")


def test_coarsest_hopping_term_and_self_coupling_by_parity_are_exact(coarsest):
    hop_and_self(coarsest)


@pytest.mark.parametrize("nv", range(2, 33, 2), ids=lambda nv: f"n{2 * nv}")
def test_single_read_form_of_the_operator_is_exact(nv, monkeypatch):
    """coarse_apply_once_kernel<float, NT, false> + its finish pass, which a lattice of this size takes only under
    DDAMG_COARSE_APPLY_ONCE_MIN_SITES=0 (a context's switches are the environment at its creation)"""
    monkeypatch.setenv("DDAMG_COARSE_APPLY_ONCE_MIN_SITES", "0")
    Lc = LATTICES["4x4x4x6"]
    ctx = two_level_ctx(Lc, nv)
    n, V = 2 * nv, int(np.prod(Lc))
    op = IntegerOperator(n, Lc, seed=3000 + nv)
    pool = integer_pool(V, n, 3100 + nv)[[0, 1, ZERO, UNIT]]
    ref, mag = op.apply(pool)
    assert mag < 2 ** 24
    ctx.set_coarse_operator(op.D, op.cl)
    vi = ctx.vector(1, 32); vo = ctx.vector(1, 32)
    for c in range(4):
        vi.upload(pool[c]); vo.upload(np.full((V, n, 2), 7.0))
        ctx.coarse_apply(vo, vi)
        assert_exact(vo.download(), ref[c], f"n = {n}, column {c}")
    vi.free(); vo.free(); ctx.close()


@pytest.mark.parametrize("nv", [2, 10, 20, 32], ids=lambda nv: f"n{2 * nv}")
def test_fp64_operator_and_hopping_term_are_exact(nv):
    """coarse_site_kernel<double, NT, *> (mixed_precision = 0)"""
    Lc = LATTICES["4x4x4x6"]
    lv = Level(two_level_ctx(Lc, nv, mixed_precision=0), 1, Lc, seed=4000 + nv, precision=64)
    for c in (0, 1, ZERO, UNIT):
        lv.ins[0].upload(lv.pool[c]); lv.outs[0].upload(np.full((lv.V, lv.n, 2), 7.0))
        lv.ctx.coarse_apply(lv.outs[0], lv.ins[0])
        assert_exact(lv.outs[0].download(), lv.ref[c], f"fp64, n = {lv.n}, column {c}")
    hop_and_self(lv)
    lv.close()


@pytest.mark.parametrize("nv", [3, 5], ids=lambda nv: f"n{2 * nv}")
def test_dof_counts_the_matrix_cores_do_not_cover_are_refused(nv):
    """n % 4 != 0: coarse_apply_many says so, the one-vector kernel still returns the integers"""
    Lc = LATTICES["4x4x4x6"]
    lv = Level(two_level_ctx(Lc, nv), 1, Lc, seed=5000 + nv)
    with pytest.raises(dd.DDAMGError, match="shape not covered"):
        lv.ctx.coarse_apply_many(lv.outs[:4], lv.ins[:4])
    for c in (0, 1, ZERO, UNIT):
        lv.ins[0].upload(lv.pool[c]); lv.outs[0].upload(np.full((lv.V, lv.n, 2), 7.0))
        lv.ctx.coarse_apply(lv.outs[0], lv.ins[0])
        assert_exact(lv.outs[0].download(), lv.ref[c], f"n = {lv.n}, column {c}")
    lv.close()


# ---- 2. the intermediate level: three-level contexts, n = 8, 16, ..., 64 ------------------------------------------------
class Intermediate(Level):
    def __init__(self, nv0):
        super().__init__(three_level_ctx(nv0), 1, L1, seed=2000 + nv0)
        self.one = self.ctx.vector(1, 32)
        self.random = None
        self.sweeps = {}

    def use_random(self):
        if self.random is None:
            self.random = random_operator(self.n, self.Lc, 6000 + self.n)
            nel = self.V * self.n * 2
            self.eta = [splitmix_uniform(nel, 100 + c).reshape(self.V, self.n, 2) for c in range(32)]
            self.phi0 = [splitmix_uniform(nel, 200 + c).reshape(self.V, self.n, 2) for c in range(32)]
        if self.kind != "random":
            self.ctx.set_coarse_operator(*self.random, level=1)
            self.kind = "random"

    def one_vector_sweeps(self, cycles, guess):
        """the one-vector smoother of every column of the pool, once"""
        self.use_random()
        if (cycles, guess) not in self.sweeps:
            res = []
            for c in range(32):
                self.ins[0].upload(self.eta[c])
                if guess:
                    self.one.upload(self.phi0[c])
                self.ctx.smoother(self.one, self.ins[0], cycles, initial_guess_zero=not guess)
                res.append(self.one.download())
            self.sweeps[(cycles, guess)] = res
        return self.sweeps[(cycles, guess)]

    def smooth_many(self, etas, phi0s, cycles):
        k = len(etas)
        for c in range(k):
            self.ins[c].upload(etas[c])
            self.outs[c].upload(phi0s[c] if phi0s is not None else np.full((self.V, self.n, 2), 7.0))
        self.ctx.smoother_many(self.outs[:k], self.ins[:k], cycles, initial_guess_zero=phi0s is None)
        return [v.download() for v in self.outs[:k]]

    def close(self):
        self.one.free()
        super().close()


@pytest.fixture(scope="module")
def intermediate(request):
    lv = Intermediate(request.param)
    yield lv
    lv.close()


every_n1 = pytest.mark.parametrize("intermediate", range(4, 33, 4), indirect=True, ids=lambda nv: f"n{2 * nv}")
smoother_n1 = pytest.mark.parametrize("intermediate", [4, 12, 20, 32], indirect=True, ids=lambda nv: f"n{2 * nv}")


@every_n1
@pytest.mark.parametrize("ncols", NCOLS)
def test_intermediate_operator_of_many_columns_is_exact(intermediate, ncols):
    """cm_relayout_kernel (G5 U^H G5 applied once, at the copy) + cm_apply_op_kernel (mfma_cproduct_op: two passes at a time, the
    tail for an odd n / 8 at n = 8, 24, 40, 56)"""
    lv = intermediate
    lv.use_integer()
    for sel in selections(ncols):
        got = lv.apply_many([lv.pool[c] for c in sel])
        for k, c in enumerate(sel):
            assert_exact(got[k], lv.ref[c], f"n = {lv.n}, {ncols} columns, column {k}")


@smoother_n1
@pytest.mark.parametrize("guess", [False, True], ids=["from-zero", "from-a-guess"])
@pytest.mark.parametrize("cycles", [1, 2])
@pytest.mark.parametrize("ncols", [2, 17, 32])
def test_smoother_of_many_columns_against_the_one_vector_smoother(intermediate, ncols, cycles, guess):
    """cm_block_minres_op_kernel in its three prologues (CM_NONE, CM_UPDATE, CM_FULL), every column on its own"""
    lv = intermediate
    ref = lv.one_vector_sweeps(cycles, guess)
    got = lv.smooth_many(lv.eta[:ncols], lv.phi0[:ncols] if guess else None, cycles)
    errs = [relerr(got[c], ref[c]) for c in range(ncols)]
    print(f"n = {lv.n}, {ncols} columns, {cycles} cycles, guess {guess}: largest relative difference of a column {max(errs):.3e}")
    for c in range(ncols):
        assert errs[c] < TOL_SWEEP, (c, errs[c])


def others(lv, base, keep, at):
    """32 columns with base[keep] at index `at` and every other column replaced: other seeds, one zero, one scaled by 1e6"""
    nel = lv.V * lv.n * 2
    cols = [splitmix_uniform(nel, 900 + c).reshape(lv.V, lv.n, 2) for c in range(32)]
    cols[(at + 5) % 32] = np.zeros((lv.V, lv.n, 2))
    cols[(at + 16) % 32] = cols[(at + 16) % 32] * 1e6
    cols[(at + 1) % 32] = cols[(at + 1) % 32] * 1e6
    cols[at] = base[keep]
    return cols


@smoother_n1
@pytest.mark.parametrize("guess", [False, True], ids=["from-zero", "from-a-guess"])
def test_smoother_column_is_independent_of_the_other_columns_and_of_its_index(intermediate, guess):
    """Bit for bit.  The arithmetic of a column does not depend on its lane or its half: every sum runs over row tiles,
    accumulator entries and wavefronts in a fixed order.  A column that read a neighbour's coefficient, or a workgroup that
    took the wrong half, would change it"""
    lv = intermediate
    lv.use_random()
    first = lv.smooth_many(lv.eta, lv.phi0 if guess else None, 2)[3]
    assert np.all(np.isfinite(first)) and np.any(first != 0.0)
    for at in (3, 19):
        got = lv.smooth_many(others(lv, lv.eta, 3, at), others(lv, lv.phi0, 3, at) if guess else None, 2)[at]
        assert np.array_equal(got, first), f"n = {lv.n}: column 3 at index {at} among other columns differs in {np.count_nonzero(got != first)} components"


@smoother_n1
def test_operator_column_is_independent_of_the_other_columns_and_of_its_index(intermediate):
    lv = intermediate
    lv.use_random()
    first = lv.apply_many(lv.eta)[3]
    assert np.all(np.isfinite(first)) and np.any(first != 0.0)
    for at in (3, 19):
        got = lv.apply_many(others(lv, lv.eta, 3, at))[at]
        assert np.array_equal(got, first), f"n = {lv.n}: column 3 at index {at} among other columns differs in {np.count_nonzero(got != first)} components"
