"""GPU tests (-m gpu) of the Galerkin construction D_c = P^H D P, bit for bit, at every aggregate shape.

The kernels: aggregate_dirac_kernel (gather form) and aggregate_dirac_tile_kernel (LDS tiles) of setup_kernels.hip,
store_column_kernel, restrict5 and the matrix-core restriction with its direct store (transfer.hip); between coarse levels
coarse_batch_apply_kernel<1..4>, coarse_batch_restrict_store_kernel and coarse_batch_restrict_store_mfma_kernel (coarse_batch.hip)
and the column-by-column form on CoarseOp::apply_masked.

Why no tolerance.  The links are monomial SU(3) matrices (entries 0, +-1, +-i; 0, +-1/2, +-i/2 as the operator stores them), the
clover term is an integer Hermitian matrix of the test's own (diagonal 8 or 9, off-diagonal parts in [-1, 1]) and P has integer
parts in [-2, 2] ([-1, 1] between coarse levels, where the operator has integer parts in [-3, 3]).  Every product and every partial
sum of the construction is then a multiple of 1/2 (an integer between coarse levels) whose magnitude in those units stays below
2^24 -- asserted on the reference (galerkin_reference.PartwiseGalerkin.bound: the largest sum |P| |part| |P|) before anything is
compared -- so fp32 in any summation order, the matrix instructions included, returns the exact number.  The reference restricts
the part that stays inside an aggregate, the four forward and the four backward parts one by one, selected by coordinates, so a
forward and a backward coupling never mix, also where the coarse extent is 2.

What is compared, with np.array_equal: every entry get_coarse_operator exports (four forward links, triu(A), triu(D) and B of the
self coupling), and -- for the lower triangles, the C block and the backward couplings, which the export does not carry --
coarse_apply and coarse_self_mul on both parities of integer vectors with parts in [-1, 1] against the product with the full
reference matrices, its bound asserted again.

The asserted bounds, as the seeds give them (every test prints its own): largest sum |P||A_part||P| in half-units 27 704 (2^4
aggregates) .. 381 064 (4^4), 740 312 (8x4x4x4), 1 461 574 (4x4x8x8); between coarse levels 10 092 (n1 = 8) .. 575 548 (n1 = 64,
2^4 aggregates) and 1 191 493 (n1 = 64, 32-site aggregates); |M||x| of the products at most 1 112 457.  2^24 = 16 777 216.

Two rows of the plan this module was written to cannot exist.  (1) N = 33 test vectors: a coarse level holds at most 64 dof per site and the context
refuses 66 (test below); the fp32 column form aggregate_dirac + galerkin_column is reached through DDAMG_GALERKIN_UNBATCHED.
(2) Two-row links (link_reals 10 or 12, the CMP = true kernels) need 256-site Schwarz blocks, and a block divides the aggregate:
aggregates of fewer than 256 sites run on full links (18), which is asserted instead."""
import numpy as np
import pytest
from conftest import random_su3
from coarse_reference import IntegerOperator
import galerkin_reference as gr
from ddalphaamg_amd import api
import ddalphaamg_amd as dd

pytestmark = pytest.mark.gpu

ROT = {"T": [16, 8, 8, 8], "Z": [8, 16, 8, 8], "Y": [8, 8, 16, 8], "X": [8, 8, 8, 16]}      # the long direction has coarse extent 4
BIG, CUBE = [8, 8, 16, 16], [8, 8, 8, 8]
NVECS = [4, 10, 16, 17, 32]
_fine, _refs = {}, {}


def assert_exact(got, ref, what):
    got = np.asarray(got); ref = np.asarray(ref)
    bad = int(np.count_nonzero(got != ref))
    assert bad == 0, f"{what}: {bad} of {ref.size} numbers differ from the exact result, the largest difference {np.abs(got - ref).max()}"


class Exact:
    """the exact next-level operator of a case: its storage as the export returns it, two integer vectors and what the operator
    and the self coupling make of them"""

    def __init__(self, g, seed):
        assert g.bound < 2 ** 24, g.bound          # the condition of "bit for bit", not a result
        self.g, self.bound = g, g.bound
        self.D, self.cl = g.storage()
        self.xs = np.random.default_rng(seed).integers(-1, 2, size=(2, g.V, g.n, 2)).astype(np.float64)
        self.full, self.self_ = [], []
        for x in self.xs:
            y, mag = g.apply(x)
            assert mag < 2 ** 24, mag
            self.full.append(y); self.self_.append(g.terms(x, [0])[0])
            self.apply_bound = mag

    def check(self, ctx, level, what):
        D, cl = ctx.get_coarse_operator(level)
        for mu in range(4):
            assert_exact(D[:, mu], self.D[:, mu], f"{what}: forward coupling {mu}")
        assert_exact(cl, self.cl, f"{what}: self coupling")
        prec = ctx.vprec()
        vi, vo = ctx.vector(level, prec), ctx.vector(level, prec)
        odd = self.g.odd
        for k, x in enumerate(self.xs):
            vi.upload(x); vo.upload(np.full(x.shape, 7.0))
            ctx.coarse_apply(vo, vi)
            assert_exact(vo.download(), self.full[k], f"{what}: operator of vector {k}")
            for parity in (0, 1):
                mine = odd if parity else ~odd
                vo.upload(np.full(x.shape, 7.0)); ctx.coarse_self_mul(vo, vi, parity, False); y = vo.download()
                assert np.all(y[~mine] == 7.0), f"{what}: self coupling, parity {parity}: the other parity was touched"
                assert_exact(y[mine], self.self_[k][mine], f"{what}: self coupling of vector {k}, parity {parity}")
        vi.free(); vo.free()


# ---- A. fine level -> level 1 -------------------------------------------------------------------------------------------------
def fine_case(L):
    """links, the oracle's D, the integer clover term and the nine couplings of a lattice; the two most recent lattices are kept"""
    from oracle import orc
    key = tuple(L)
    if key not in _fine:
        while len(_fine) >= 2:
            _fine.pop(next(iter(_fine)))
        V = int(np.prod(L))
        D, _, _ = orc.gauge_to_operator(L, gr.monomial_gauge(L, 100 + sum(k * v for k, v in enumerate(L))), 1, -1.0, 0.0)
        cl = gr.integer_clover(V, 200 + L[0])
        _fine[key] = (D, cl, gr.fine_couplings(L, D, cl))
    return _fine[key]


def fine_reference(L, Lc, N):
    key = (tuple(L), tuple(Lc), N)
    if key not in _refs:
        V = int(np.prod(L))
        P = np.random.default_rng(300 + N).integers(-2, 3, size=(N, V, 12, 2)).astype(np.float64)
        g = gr.PartwiseGalerkin(L, Lc, fine_case(L)[2], gr.interpolation_blocks(P, 12), unit=2)
        _refs[key] = (P, Exact(g, 400 + N))
        print(f"lattice {L} over {Lc}, N = {N}: largest sum |P||A_part||P| {g.bound} half-units, |M||x| {_refs[key][1].apply_bound} (2^24 = {2 ** 24})")
    return _refs[key]


def fine_ctx(L, Lc, N, mp=1, split=""):
    ext = [l // c for l, c in zip(L, Lc)]
    B = [4] * 4 if all(e % 4 == 0 for e in ext) else [2] * 4
    p = api.default_params(); p.num_levels = 2
    for mu in range(4):
        p.local_lattice[0][mu] = L[mu]; p.block_lattice[0][mu] = B[mu]; p.local_lattice[1][mu] = Lc[mu]
        if str(mu) in split:
            p.process_grid[mu] = -1
    p.num_vect[0] = N
    p.post_smooth_iter[0] = 2; p.block_iter[0] = 4; p.setup_iter[0] = 1
    p.restart, p.max_restart, p.tol = 20, 5, 1e-10
    p.coarse_iter, p.coarse_restart, p.coarse_tol = 20, 2, 5e-2
    p.mixed_precision, p.method, p.odd_even = mp, 2, 1
    p.m0, p.csw = -1.0, 0.0
    ctx = dd.Context(p)
    if split:
        ctx.comm_init_rccl(api.rccl_unique_id())
    return ctx, B


def run_fine(monkeypatch, L, Lc, N, mp=1, split="", env=(), full_links=False):
    for name in ("DDAMG_LINK_COMPRESSION", "DDAMG_AGGREGATE_DIRAC_GATHER", "DDAMG_GALERKIN_FULL_FIELDS", "DDAMG_GALERKIN_STORE_COLUMNS",
                 "DDAMG_GALERKIN_UNBATCHED", "DDAMG_GALERKIN_SLAB_AGGS"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env:
        monkeypatch.setenv(name, value)            # a context's switches are the environment at its creation
    if full_links:
        monkeypatch.setenv("DDAMG_LINK_COMPRESSION", "0")
    P, ref = fine_reference(L, Lc, N)
    D, cl, _ = fine_case(L)
    ctx, B = fine_ctx(L, Lc, N, mp, split)
    ctx.set_operator(D, cl)
    if B == [4] * 4 and not full_links:
        assert ctx.link_reals() in (10, 12)        # the two-row kernels (CMP = true)
    else:
        assert ctx.link_reals() == 18
    ctx.set_interpolation(P, level=0)
    ref.check(ctx, 1, f"{L} over {Lc}, N = {N}, fp{ctx.vprec()}, split '{split}', {dict(env)}")
    ctx.close()


def over(L, ext):
    return [l // e for l, e in zip(L, ext)]


def rotated(ext, d):
    """the aggregate 8x4x4x4 with its long side in direction d"""
    e = list(ext[1:]); e.insert("TZYX".index(d), ext[0])
    return e


@pytest.mark.parametrize("N", NVECS)
@pytest.mark.parametrize("aggregate", ["4x4x4x4", "8x4x4x4"])
def test_every_vector_count(aggregate, N, monkeypatch):
    """16x8x8x8 with 4^4 aggregates (a tile is an aggregate; T has four of them, distinct neighbours) and with 8x4x4x4 aggregates
    (two tiles: the neighbour inside the aggregate but outside the tile, forward and backward, in T); n = 8, n = 20 (padded 8x8
    tiles of the direct store), 2N = 32 (the last restrict_mfma_kernel<1>), 34 (the first <2, true>) and 64"""
    run_fine(monkeypatch, ROT["T"], over(ROT["T"], [4, 4, 4, 4] if aggregate == "4x4x4x4" else [8, 4, 4, 4]), N)


@pytest.mark.parametrize("d", ["Z", "Y", "X"])
@pytest.mark.parametrize("aggregate", ["4x4x4x4", "8x4x4x4"])
def test_every_direction(aggregate, d, monkeypatch):
    """the long direction of the lattice in Z, Y, X: four 4^4 aggregates (distinct forward and backward neighbours in that
    direction), or 512-site aggregates whose two tiles are neighbours in that direction"""
    run_fine(monkeypatch, ROT[d], over(ROT[d], [4, 4, 4, 4] if aggregate == "4x4x4x4" else rotated([8, 4, 4, 4], d)), 16)


def test_1024_site_aggregates(monkeypatch):
    """4x4x8x8 aggregates, four tiles each: the neighbours outside the tile in Y and in X"""
    run_fine(monkeypatch, BIG, over(BIG, [4, 4, 8, 8]), 16)


@pytest.mark.parametrize("slab", [None, "1", "3", "5"], ids=lambda s: f"slab-{s}")
@pytest.mark.parametrize("aggregate", ["2x2x4x4", "2x4x4x4"])
def test_several_aggregates_per_tile_and_slabs(aggregate, slab, monkeypatch):
    """64- and 128-site aggregates on 8^4, two to four per tile; slabs of 1, 3, 5 aggregates: 64 .. 640 sites per launch -- partial
    tiles with dead lanes, tiles that start at no multiple of 256 sites of the lattice, an uneven last slab"""
    ext = [int(v) for v in aggregate.split("x")]
    run_fine(monkeypatch, CUBE, over(CUBE, ext), 16, env=[("DDAMG_GALERKIN_SLAB_AGGS", slab)] if slab else [])


@pytest.mark.parametrize("aggregate", ["2x2x2x2", "2x2x2x4"])
def test_aggregates_whose_faces_are_no_multiple_of_16(aggregate, monkeypatch):
    """16- and 32-site aggregates (faces of 8 sites): full fields, aggregate_dirac_slab + restrict_batch_slab"""
    ext = [int(v) for v in aggregate.split("x")]
    run_fine(monkeypatch, CUBE, over(CUBE, ext), 16)


KNOBS = ["DDAMG_AGGREGATE_DIRAC_GATHER", "DDAMG_GALERKIN_FULL_FIELDS", "DDAMG_GALERKIN_STORE_COLUMNS", "DDAMG_GALERKIN_UNBATCHED"]


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("aggregate", ["2x2x4x4", "8x4x4x4"])
def test_every_form_of_the_construction(aggregate, knob, monkeypatch):
    """the gather form of the field kernel, five full fields per column, the store through coarse column vectors, and column by
    column (aggregate_dirac + galerkin_column: restrict5 + store_column_kernel, in fp32): the same exact matrices"""
    if aggregate == "2x2x4x4":
        run_fine(monkeypatch, CUBE, over(CUBE, [2, 2, 4, 4]), 16, env=[(knob, "1")])
    else:
        run_fine(monkeypatch, ROT["T"], over(ROT["T"], [8, 4, 4, 4]), 16, env=[(knob, "1")])


def test_full_links(monkeypatch):
    """DDAMG_LINK_COMPRESSION=0: the CMP = false instantiation on a two-tile aggregate"""
    run_fine(monkeypatch, ROT["T"], over(ROT["T"], [8, 4, 4, 4]), 16, full_links=True)


@pytest.mark.parametrize("N", [10, 16])
@pytest.mark.parametrize("aggregate", ["2x2x2x2", "2x2x4x4", "4x4x4x4", "8x4x4x4"])
def test_fp64_contexts(aggregate, N, monkeypatch):
    """mixed_precision = 0: aggregate_dirac_kernel<double, false, false> + galerkin_column<double>, CoarseOp<double>"""
    ext = [int(v) for v in aggregate.split("x")]
    L = CUBE if aggregate in ("2x2x2x2", "2x2x4x4") else ROT["T"]
    run_fine(monkeypatch, L, over(L, ext), N, mp=0)


@pytest.mark.parametrize("kernel", ["tile", "gather", "fp64"])
@pytest.mark.parametrize("split", ["0123", "23"])
@pytest.mark.parametrize("aggregate", ["4x4x4x4", "8x4x4x4"])
def test_through_the_self_exchange(aggregate, split, kernel, monkeypatch):
    """the process its own neighbour in the directions of `split`: the distributed instantiations (aggregate_dirac_tile_kernel
    <float, CHIR, true, true>; aggregate_dirac_kernel<float, true, true> under DDAMG_AGGREGATE_DIRAC_GATHER; <double, true, false>
    in an fp64 context) take the neighbours' boundary through the transport; the same exact matrices as the undivided construction"""
    L, ext = (CUBE, [4, 4, 4, 4]) if aggregate == "4x4x4x4" else (ROT["T"], [8, 4, 4, 4])
    run_fine(monkeypatch, L, over(L, ext), 16, mp=0 if kernel == "fp64" else 1, split=split,
             env=[("DDAMG_AGGREGATE_DIRAC_GATHER", "1")] if kernel == "gather" else [])


def test_more_than_64_coarse_dof_are_refused():
    """N = 33 would need n = 66: refused when the hierarchy is made, before any kernel runs"""
    L = CUBE
    with pytest.raises(dd.DDAMGError, match="at most 64"):
        ctx, _ = fine_ctx(L, over(L, [4, 4, 4, 4]), 33)
        D, cl, _ = fine_case(L)
        ctx.set_operator(D, cl)
        ctx.set_interpolation(np.zeros((33, 4096, 12, 2)), level=0)


# ---- B. level 1 -> level 2 ----------------------------------------------------------------------------------------------------
L1 = [4, 4, 4, 8]
L2S = {"2x2x2x2": [2, 2, 2, 4], "2x2x2x4": [2, 2, 2, 2]}       # aggregate -> the coarsest lattice
_gauge = []


def coarse_reference_case(agg, n1, N1):
    key = (agg, n1, N1)
    if key not in _refs:
        op = IntegerOperator(n1, L1, seed=500 + n1)
        P1 = np.random.default_rng(600 + 7 * n1 + N1).integers(-1, 2, size=(N1, op.V, n1, 2)).astype(np.float64)
        g = gr.PartwiseGalerkin(L1, L2S[agg], gr.coarse_couplings(op), gr.interpolation_blocks(P1, n1), unit=1)
        _refs[key] = (op, P1, Exact(g, 700 + n1 + N1))
        print(f"level 1 {L1} over {L2S[agg]}, n1 = {n1}, N1 = {N1}: largest sum |P||M_part||P| {g.bound}, |M||x| {_refs[key][2].apply_bound} (2^24 = {2 ** 24})")
    return _refs[key]


def run_coarse(monkeypatch, agg, n1, N1, mp=1, env=(), split=""):
    for name in ("DDAMG_COARSE_RESTRICT_VALU", "DDAMG_GALERKIN_UNBATCHED"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env:
        monkeypatch.setenv(name, value)
    op, P1, ref = coarse_reference_case(agg, n1, N1)
    L2 = L2S[agg]
    p = api.default_params(); p.num_levels = 3
    for mu in range(4):
        p.local_lattice[0][mu] = 2 * L1[mu]; p.block_lattice[0][mu] = 2
        p.local_lattice[1][mu] = L1[mu]; p.block_lattice[1][mu] = 2
        p.local_lattice[2][mu] = L2[mu]
        if str(mu) in split:
            p.process_grid[mu] = -1
    p.num_vect[0], p.num_vect[1] = n1 // 2, N1
    p.post_smooth_iter[0] = p.post_smooth_iter[1] = 2; p.block_iter[0] = p.block_iter[1] = 4
    p.setup_iter[0] = p.setup_iter[1] = 1
    p.restart, p.max_restart, p.tol = 20, 5, 1e-10
    p.coarse_iter, p.coarse_restart, p.coarse_tol = 20, 2, 5e-2
    p.kcycle, p.kcycle_restart, p.kcycle_max_restart, p.kcycle_tol = 1, 5, 2, 1e-1
    p.mixed_precision, p.method, p.odd_even = mp, 2, 1
    p.m0, p.csw = -0.1, 1.0
    ctx = dd.Context(p)
    if split:
        ctx.comm_init_rccl(api.rccl_unique_id())
    if not _gauge:
        _gauge.append(random_su3(16 * int(np.prod(L1)) * 4, 2718).reshape(-1, 4, 9, 2))      # the fine level only has to exist
    ctx.set_gauge(_gauge[0], anti_pbc=True)
    ctx.set_coarse_operator(op.D, op.cl, level=1)
    ctx.set_interpolation(P1, level=1)
    ref.check(ctx, 2, f"level 1 over {L2}, n1 = {n1}, N1 = {N1}, fp{ctx.vprec()}, split '{split}', {dict(env)}")
    ctx.close()


N1S = [8, 20, 32, 36, 48, 56, 64]
NV1S = [4, 15, 16, 17, 32]


@pytest.mark.parametrize("N1", NV1S)
@pytest.mark.parametrize("n1", N1S)
def test_between_coarse_levels(n1, N1, monkeypatch):
    """4x4x4x8 over 2x2x2x4, 2^4 aggregates, distinct neighbours in X: coarse_batch_apply_kernel<1..4> (n1 = 8; 20, 32; 36, 48; 56,
    64; the last row tile half empty at 8, 20, 36, 56), the matrix-core restriction at n1 % 8 == 0 up to 56, the vector-unit one at
    n1 % 8 == 4 and at 64 (ldp 260 > 232); 8 .. 64 columns"""
    run_coarse(monkeypatch, "2x2x2x2", n1, N1)


@pytest.mark.parametrize("n1,N1", [(8, 16), (20, 4), (32, 16), (36, 17), (64, 32)])
def test_between_coarse_levels_with_32_site_aggregates(n1, N1, monkeypatch):
    """4x4x4x8 over 2^4, 2x2x2x4 aggregates: forward and backward neighbour aggregate coincide in every direction; the matrix-core
    restriction at n1 = 8 (ldp 68), the vector-unit one from n1 = 32 on (ldp 260)"""
    run_coarse(monkeypatch, "2x2x2x4", n1, N1)


@pytest.mark.parametrize("knob", ["DDAMG_COARSE_RESTRICT_VALU", "DDAMG_GALERKIN_UNBATCHED"])
@pytest.mark.parametrize("n1,N1", [(32, 16), (48, 17), (20, 15)])
def test_other_forms_between_coarse_levels(n1, N1, knob, monkeypatch):
    """the vector-unit restriction where the matrix cores would run, and the column-by-column form on CoarseOp::apply_masked"""
    run_coarse(monkeypatch, "2x2x2x2", n1, N1, env=[(knob, "1")])


@pytest.mark.parametrize("agg,n1,N1", [("2x2x2x2", 20, 10), ("2x2x2x2", 48, 16), ("2x2x2x4", 32, 17)])
def test_between_coarse_levels_in_fp64(agg, n1, N1, monkeypatch):
    """mixed_precision = 0: CoarseOp<double>::apply_masked, restrict_to and store_matrix_column in fp64"""
    run_coarse(monkeypatch, agg, n1, N1, mp=0)


def test_between_coarse_levels_through_the_self_exchange(monkeypatch):
    """the process its own neighbour in every direction: the forward parts across the process boundary take their operand from
    the wide halo of the batch (CoarseOp::wide_halo_exchange)"""
    run_coarse(monkeypatch, "2x2x2x2", 32, 16, split="0123")
