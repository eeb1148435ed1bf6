"""The gauge sector of the molecular dynamics on a process grid (-m gpu): ddamg_hip_gauge_loops_device_grid, _gauge_force_device_grid,
_links_update_device_grid, _links_reunitarize_device_grid, _momentum_update_device_grid and _momentum_kinetic_device_grid.
One process: a process-grid entry of -1 makes the process its own neighbour over RCCL, so the shell of the links, one site deep
without rectangles and two with them, travels through pack -> send/recv -> unpack for real (contexts as in test_gpu_force_grid.py),
and the result must be that of the undivided periodic lattice, bit for bit.  Several processes: tests/dist_gauge_md_worker.py over
the host transport.

Lattices and grids: those of test_gpu_force_grid.py.  4x6x8x10 (tile tails of 6 and 10; the extended extents 10 and 14 open a second
tile) with one split direction, with a wrapped and a shell direction in one plane, and with all four; 2x4x6x4 with all four, where
T = 2 is the depth of the shell and the whole local lattice travels both ways.  Actions c1 = 0 (depth 1), -1/12 and -0.331 (depth 2).
Links exp(0.35 algebra), beta 5.6, as test_gpu_gauge_md.py.

Bars.  Against tests/gauge_reference.py: 1e-13 of the field's norm or of the sum, the project's fp64 bar, as test_gpu_gauge_md.py.
Against the same call on an undivided context: no real differs in its bits -- one kernel serves both, and one process holds every
tile in the same order, so the loop sums are equal too.  Messages: two per split direction and collective call, of
72 * 8 * H * prod_{d != mu} (L_d + 2 H if d < mu and split, else L_d) bytes (docs/design/06_multi_gpu.md).  Trajectory: tau = 0.5 in 10, 20 and 40 steps and
backwards at 40, as test_gpu_gauge_md.py; reversibility 1e-12, its bar."""
import os
import numpy as np
import pytest
from conftest import relerr, splitmix_uniform
from ddalphaamg_amd import api
import ddalphaamg_amd as dd
import force_reference as fr
import gauge_reference as gr
from test_gpu_device_interface import Hip, params

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
RAGGED = (4, 6, 8, 10)
SMALL = (2, 4, 6, 4)
ALL = (-1, -1, -1, -1)
CASES = [(RAGGED, (-1, 1, 1, 1)), (RAGGED, (1, -1, 1, -1)), (RAGGED, ALL), (SMALL, ALL)]
IDS = ["4x6x8x10-T", "4x6x8x10-ZX", "4x6x8x10-all", "2x4x6x4-all"]
C1 = [gr.WILSON, gr.SYMANZIK, gr.IWASAKI]
BETA = 5.6
M0, CSW = -0.3, 1.25
EPS = np.finfo(np.float64).eps
_fields, _reference = {}, {}


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.free_all()


def links(L):
    """the links of a lattice, exp(0.35 algebra), made once and never changed"""
    L = tuple(L)
    if L not in _fields:
        V = int(np.prod(L))
        one = np.zeros((V, 4, 9, 2)); one[:, :, [0, 4, 8], 0] = 1.0
        _fields[L] = fr.perturbed(one, fr.random_algebra(np.random.default_rng(5), (V, 4)), 0.35)
        _fields[L].setflags(write=False)
    return _fields[L]


def reference(L):
    """(plaquette sum, rectangle sum, G of the plaquette part, G of the rectangle part) of the whole periodic lattice, computed once"""
    L = tuple(L)
    if L not in _reference:
        _reference[L] = gr.loops(list(L), links(L)) + (gr.force(list(L), links(L), BETA, 0.0, "plaquette"), gr.force(list(L), links(L), BETA, 0.0, "rectangle"))
    return _reference[L]


def reference_force(L, c1):
    _, _, gp, gq = reference(L)
    return (1.0 - 8.0 * c1) * gp + c1 * gq


def context(L, grid, csw=CSW):
    """a one-level context on the grid, RCCL where it is divided"""
    ctx = dd.Context(params(list(L), [2] * 4, M0, csw, grid=grid))
    if min(grid) < 0:
        ctx.comm_init_rccl(api.rccl_unique_id())
    return ctx


def nbytes(L):
    return int(np.prod(L)) * 72 * 8


def shape(L):
    return (int(np.prod(L)), 4, 9, 2)


def different_bits(a, b):
    return int(np.count_nonzero(np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64)))


def shell_bytes(L, grid, depth):
    """bytes sent per call for the shell of the links: both sides of every split direction, each slab `depth` sites thick, spanning
    the extended range of the split directions before it and the own range of those after it"""
    total = 0
    for mu in range(4):
        if grid[mu] != -1:
            continue
        n = 72 * 8 * depth
        for d in range(4):
            if d != mu:
                n *= L[d] + 2 * depth if (d < mu and grid[d] == -1) else L[d]
        total += 2 * n
    return total


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,grid", CASES, ids=IDS)
def test_forces_and_loops_against_the_reference_and_the_undivided_context(L, grid, hip):
    U = links(L)
    plaq, rect, _, _ = reference(L)
    dU = hip.upload(U); out = hip.alloc(nbytes(L))
    ctx = context(L, grid)
    sums = ctx.gauge_loops_device_grid(dU)
    plaquette_only = ctx.gauge_loops_device_grid(dU, rectangles=False)
    forces = {}
    for c1 in C1:
        assert ctx.gauge_force_device_grid(out, dU, BETA, c1) == out
        forces[c1] = hip.download(out, shape(L))
        err = relerr(forces[c1], reference_force(L, c1))
        print(L, grid, f"c1 {c1:+.4f}: force against the reference {err:.1e}")
        assert err < 1e-13
        ctx.gauge_force_device_grid(out, dU, BETA, c1)
        assert different_bits(hip.download(out, shape(L)), forces[c1]) == 0          # two calls, the same bits
    assert ctx.gauge_loops_device_grid(dU) == sums
    assert np.array_equal(hip.download(dU, U.shape), U)                               # the links are read only
    ctx.close()
    p, r = sums
    print(L, grid, f"plaquette sum {p:.12e} ({abs(p - plaq) / abs(plaq):.1e}), rectangle sum {r:.12e} ({abs(r - rect) / abs(rect):.1e})")
    assert plaquette_only[1] is None
    assert abs(p - plaq) <= 1e-13 * abs(plaq) and abs(plaquette_only[0] - plaq) <= 1e-13 * abs(plaq) and abs(r - rect) <= 1e-13 * abs(rect)
    # the undivided context: the same bits
    plain = dd.Context(params(list(L), [2] * 4, M0, CSW))
    assert plain.gauge_loops_device(dU) == sums and plain.gauge_loops_device(dU, rectangles=False) == plaquette_only
    for c1 in C1:
        plain.gauge_force_device(out, dU, BETA, c1)
        differ = different_bits(hip.download(out, shape(L)), forces[c1])
        print(L, grid, f"c1 {c1:+.4f}: reals that differ in their bits from the undivided context's: {differ} of {forces[c1].size}")
        assert differ == 0
    plain.close()


# 2 ------------------------------------------------------------------------------------------------------------------------
def test_inputs_sentinels_coeff_and_accumulate(hip):
    L = RAGGED
    U = links(L)
    n = int(np.prod(L)) * 72
    ctx = context(L, ALL)
    dU = hip.upload(U)
    # sentinel reals before and behind the force array
    guard = 16
    held = np.full(n + 2 * guard, -7.0e300)
    big = hip.upload(held)
    out = big + 8 * guard
    G = {}
    for c1 in C1:
        ctx.gauge_force_device_grid(out, dU, BETA, c1)
        back = hip.download(big, held.shape)
        assert (back[:guard] == -7.0e300).all() and (back[-guard:] == -7.0e300).all()
        G[c1] = back[guard:-guard].reshape(shape(L))
        g = fr.as_matrices(G[c1])
        assert np.array_equal(g, -fr.dag(g)) and np.abs(np.trace(g, axis1=-2, axis2=-1)).max() <= 4 * EPS * np.abs(g).max()
        assert np.array_equal(hip.download(dU, U.shape), U)
    # coeff and accumulate, as test_gpu_gauge_md.py: G is linear in c1
    acc = hip.alloc(nbytes(L))
    ratio = gr.IWASAKI / gr.SYMANZIK
    ctx.gauge_force_device_grid(acc, dU, BETA, gr.WILSON, coeff=1.0 - ratio)
    ctx.gauge_force_device_grid(acc, dU, BETA, gr.SYMANZIK, coeff=ratio, accumulate=True)
    combined = hip.download(acc, shape(L))
    print(f"(1 - r) G(0) + r G(-1/12) against G(-0.331) {relerr(combined, G[gr.IWASAKI]):.1e}, against the reference "
          f"{relerr(combined, reference_force(L, gr.IWASAKI)):.1e}")
    assert relerr(combined, G[gr.IWASAKI]) < 1e-13 and relerr(combined, reference_force(L, gr.IWASAKI)) < 1e-13
    ctx.gauge_force_device_grid(acc, dU, BETA, gr.SYMANZIK, coeff=-2.5)
    assert relerr(hip.download(acc, shape(L)), -2.5 * G[gr.SYMANZIK]) < 1e-15
    start = splitmix_uniform(n, 12).reshape(shape(L))
    acc2 = hip.upload(start)
    ctx.gauge_force_device_grid(acc2, dU, BETA, gr.IWASAKI, coeff=0.7, accumulate=True)
    assert relerr(hip.download(acc2, shape(L)), start + 0.7 * G[gr.IWASAKI]) <= 2 * EPS
    assert np.array_equal(hip.download(dU, U.shape), U)
    ctx.close()


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(1, -1, 1, -1), ALL], ids=["ZX", "all"])
def test_messages_per_call(grid, hip):
    """what docs/design/06_multi_gpu.md states: the loops and the force send two messages per split direction, a shell one site deep
    for c1 = 0 and without the rectangle sum, two sites deep otherwise; the other four send nothing"""
    L = SMALL
    U = links(L)
    nsplit = sum(1 for e in grid if e == -1)
    ctx = context(L, grid)
    dU = hip.upload(U); out = hip.alloc(nbytes(L))
    dP = hip.upload(fr.as_reals(fr.random_algebra(np.random.default_rng(17), (shape(L)[0], 4))))
    dW = hip.upload(U)
    calls = [("force c1 0", lambda: ctx.gauge_force_device_grid(out, dU, BETA, 0.0), 1), ("force c1 -1/12", lambda: ctx.gauge_force_device_grid(out, dU, BETA, gr.SYMANZIK), 2),
             ("force c1 -0.331", lambda: ctx.gauge_force_device_grid(out, dU, BETA, gr.IWASAKI, 0.5, True), 2),
             ("loops", lambda: ctx.gauge_loops_device_grid(dU), 2), ("loops without rectangles", lambda: ctx.gauge_loops_device_grid(dU, rectangles=False), 1),
             ("links_update", lambda: ctx.links_update_device_grid(dW, dP, 0.01), 0), ("momentum_update", lambda: ctx.momentum_update_device_grid(dP, out, 0.01), 0),
             ("momentum_kinetic", lambda: ctx.momentum_kinetic_device_grid(dP), 0),
             ("links_reunitarize", lambda: ctx.links_reunitarize_device_grid(dW), 0),
             ("links_reunitarize without the deviation", lambda: ctx.links_reunitarize_device_grid(dW, deviation=False), 0)]
    for name, call, depth in calls + calls[:4]:      # the second round reuses the extended arrays
        ctx.comm_stats(reset=True)
        call()
        shell = ctx.comm_stats()["device_sendrecv"]
        print(grid, name, shell)
        assert shell["messages"] == (2 * nsplit if depth else 0) and shell["bytes_sent"] == (shell_bytes(L, grid, depth) if depth else 0)
    ctx.close()


# 4 ------------------------------------------------------------------------------------------------------------------------
def leapfrog(ctx, dU, dP, dF, c1, tau, n, grid):
    """n leapfrog steps through the entry points, as gauge_reference.leapfrog takes them: the _grid family or the plain one"""
    force = ctx.gauge_force_device_grid if grid else ctx.gauge_force_device
    momenta = ctx.momentum_update_device_grid if grid else ctx.momentum_update_device
    update = ctx.links_update_device_grid if grid else ctx.links_update_device
    dt = tau / n
    momenta(dP, force(dF, dU, BETA, c1), 0.5 * dt)
    for k in range(n):
        update(dU, dP, dt)
        momenta(dP, force(dF, dU, BETA, c1), dt if k < n - 1 else 0.5 * dt)


def hamiltonian(ctx, dU, dP, V, c1, grid):
    if grid:
        return ctx.momentum_kinetic_device_grid(dP) + gr.action_from_sums(V, BETA, c1, *ctx.gauge_loops_device_grid(dU))
    return ctx.momentum_kinetic_device(dP) + gr.action_from_sums(V, BETA, c1, *ctx.gauge_loops_device(dU))


STEPS = (10, 20, 40)      # the step counts of test_gpu_gauge_md.py, which goes backwards at the last


@pytest.mark.parametrize("c1", C1)
def test_a_pure_gauge_leapfrog_trajectory_through_the_grid_calls(c1, hip):
    """tau = 0.5 in 10, 20 and 40 steps, as test_gpu_gauge_md.py, on the grid and on the undivided lattice: at every step count the
    links, the momenta, H before and after and the deviation the reunitarisation finds have the same bits; the 40-step trajectory
    with -P returns to the start within 1e-12"""
    L = RAGGED
    V = int(np.prod(L))
    U = links(L)
    P = fr.as_reals(fr.random_algebra(np.random.default_rng(21), (V, 4)))
    end = {}
    for grid in (True, False):
        ctx = context(L, ALL if grid else (1, 1, 1, 1))
        dF = hip.alloc(nbytes(L))
        for n in STEPS:
            dU = hip.upload(U); dP = hip.upload(P)
            H0 = hamiltonian(ctx, dU, dP, V, c1, grid)
            leapfrog(ctx, dU, dP, dF, c1, 0.5, n, grid)
            H1 = hamiltonian(ctx, dU, dP, V, c1, grid)
            u, p = hip.download(dU, U.shape), hip.download(dP, P.shape)
            dR = hip.upload(u)      # reunitarised apart: the trajectory's own links go backwards below
            dev = ctx.links_reunitarize_device_grid(dR) if grid else ctx.links_reunitarize_device(dR)
            end[grid, n] = (u, p, hip.download(dR, U.shape), H0, H1, dev)
        if grid:      # backwards: the n = 40 trajectory with -P returns to the start
            dM = hip.upload(-end[grid, 40][1])
            leapfrog(ctx, dU, dM, dF, c1, 0.5, 40, grid)
            back_u, back_p = np.abs(hip.download(dU, U.shape) - U).max(), np.abs(hip.download(dM, P.shape) + P).max()
            dH = {n: end[grid, n][4] - end[grid, n][3] for n in STEPS}
            print(f"c1 {c1:+.4f}: H0 {end[grid, 10][3]:.6e}, Delta H {dH[10]:+.6e} {dH[20]:+.6e} {dH[40]:+.6e}, ratios {dH[10] / dH[20]:.3f} "
                  f"{dH[20] / dH[40]:.3f}, reversibility U {back_u:.1e} P {back_p:.1e}")
            assert back_u <= 1e-12 and back_p <= 1e-12
        ctx.close()
    for n in STEPS:
        g, u = end[True, n], end[False, n]
        differ = [different_bits(g[k], u[k]) for k in range(3)]
        print(f"c1 {c1:+.4f} n {n}: reals that differ in their bits (links, momenta, reunitarised links): {differ}; H0, H1, deviation {g[3:]} {u[3:]}")
        assert differ == [0, 0, 0]
        assert g[3:] == u[3:]                                       # H before and after, and the deviation: the same bits
        assert g[4] != g[3] and different_bits(g[0], U) > 0         # a trajectory was run


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_one_step_with_fermions(hip):
    """gauge_force_device_grid writes, force_bilinear_device_grid accumulates, momentum_update_device_grid: the bits of the undivided
    sequence of plain calls"""
    L = RAGGED
    V = int(np.prod(L))
    U = links(L)
    X = splitmix_uniform(V * 24, 9).reshape(V, 12, 2); Y = splitmix_uniform(V * 24, 10).reshape(V, 12, 2)
    P = fr.as_reals(fr.random_algebra(np.random.default_rng(21), (V, 4)))
    got = {}
    for grid in (True, False):
        ctx = context(L, ALL if grid else (1, 1, 1, 1))
        dU = hip.upload(U); dP = hip.upload(P); dF = hip.alloc(nbytes(L)); dx = hip.upload(X); dy = hip.upload(Y)
        if grid:
            ctx.set_gauge_device_grid(dU, anti_pbc=True)
            ctx.gauge_force_device_grid(dF, dU, BETA, gr.SYMANZIK)
            ctx.force_bilinear_device_grid(dF, dy, dx, -2.0, True)
            ctx.momentum_update_device_grid(dP, dF, 0.05)
        else:
            ctx.set_gauge_device(dU, anti_pbc=True)
            ctx.gauge_force_device(dF, dU, BETA, gr.SYMANZIK)
            ctx.force_bilinear_device(dF, dy, dx, -2.0, True)
            ctx.momentum_update_device(dP, dF, 0.05)
        got[grid] = (hip.download(dF, shape(L)), hip.download(dP, shape(L)))
        assert np.array_equal(hip.download(dU, U.shape), U)
        ctx.close()
    gauge = reference_force(L, gr.SYMANZIK)
    assert relerr(got[True][0], gauge) > 1e-3                  # the fermion force went in
    print("reals that differ in their bits, force and momenta:", different_bits(got[True][0], got[False][0]), different_bits(got[True][1], got[False][1]))
    assert different_bits(got[True][0], got[False][0]) == 0 and different_bits(got[True][1], got[False][1]) == 0
    assert np.abs(got[True][1] - (P + 0.05 * got[True][0])).max() <= 2 * EPS * (np.abs(P).max() + 0.05 * np.abs(got[True][0]).max())


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_undivided_context_runs_the_plain_calls_and_memory_returns(hip):
    L = RAGGED
    V = int(np.prod(L))
    U = links(L)
    P = fr.as_reals(fr.random_algebra(np.random.default_rng(21), (V, 4)))
    dU = hip.upload(U); a, b = hip.alloc(nbytes(L)), hip.alloc(nbytes(L))
    before = api.memory_in_use()
    ctx = context(L, (1, 1, 1, 1))
    assert ctx.gauge_loops_device_grid(dU) == ctx.gauge_loops_device(dU)
    assert ctx.gauge_loops_device_grid(dU, rectangles=False) == ctx.gauge_loops_device(dU, rectangles=False)
    for c1 in C1:
        ctx.gauge_force_device(a, dU, BETA, c1, 0.7); ctx.gauge_force_device_grid(b, dU, BETA, c1, 0.7)
        assert different_bits(hip.download(a, shape(L)), hip.download(b, shape(L))) == 0
    pa, pb = hip.upload(P), hip.upload(P)
    ctx.momentum_update_device(pa, a, -0.3); ctx.momentum_update_device_grid(pb, b, -0.3)
    assert different_bits(hip.download(pa, shape(L)), hip.download(pb, shape(L))) == 0
    assert ctx.momentum_kinetic_device(pa) == ctx.momentum_kinetic_device_grid(pb)
    ua, ub = hip.upload(U), hip.upload(U)
    ctx.links_update_device(ua, pa, 0.1); ctx.links_update_device_grid(ub, pb, 0.1)
    assert different_bits(hip.download(ua, shape(L)), hip.download(ub, shape(L))) == 0
    assert ctx.links_reunitarize_device(ua) == ctx.links_reunitarize_device_grid(ub)
    assert different_bits(hip.download(ua, shape(L)), hip.download(ub, shape(L))) == 0
    ctx.close()
    assert api.memory_in_use() == before
    # a divided context keeps the extended arrays of both depths and their slab buffers from the first call on, and lets go of them
    ctx = context(L, ALL)
    ctx.gauge_force_device_grid(a, dU, BETA, 0.0); ctx.gauge_loops_device_grid(dU, rectangles=False)
    one = api.memory_in_use()[0]
    ctx.gauge_force_device_grid(a, dU, BETA, gr.SYMANZIK); ctx.gauge_loops_device_grid(dU)
    two = api.memory_in_use()[0]
    ctx.gauge_force_device_grid(a, dU, BETA, gr.IWASAKI); ctx.gauge_loops_device_grid(dU); ctx.gauge_force_device_grid(a, dU, BETA, 0.0)
    extended = lambda h: 72 * 8 * int(np.prod([e + 2 * h for e in L]))
    print("device bytes: before", before[0], "after the depth-1 force", one, "after the depth-2 force", two, "extended arrays", extended(1), extended(2))
    assert two - one >= extended(2) and one - before[0] >= extended(1)
    assert api.memory_in_use()[0] == two                       # reused, not made again
    ctx.close()
    assert api.memory_in_use() == before


# 7 ------------------------------------------------------------------------------------------------------------------------
def refused(call, *words):
    with pytest.raises(api.DDAMGError) as e:
        call()
    assert all(w in str(e.value) for w in words), str(e.value)


def test_refusals(hip):
    L = SMALL
    V = int(np.prod(L))
    U = links(L)
    dU = hip.upload(U); dP = hip.upload(np.ones(shape(L))); dF = hip.upload(2.0 * np.ones(shape(L)))
    host = np.zeros(V * 72)
    small = hip.alloc(nbytes(L))
    ctx = context(L, ALL)
    ctx.gauge_force_device_grid(dF, dU, BETA, gr.SYMANZIK)
    good = hip.download(dF, shape(L))
    ctx.comm_stats(reset=True)
    calls = {"gauge_loops": lambda a: ctx.gauge_loops_device_grid(a), "gauge_force (output)": lambda a: ctx.gauge_force_device_grid(a, dU, BETA, gr.SYMANZIK),
             "gauge_force (links)": lambda a: ctx.gauge_force_device_grid(dF, a, BETA, gr.SYMANZIK),
             "links_update (links)": lambda a: ctx.links_update_device_grid(a, dP, 0.1), "links_update (momenta)": lambda a: ctx.links_update_device_grid(dU, a, 0.1),
             "links_reunitarize": lambda a: ctx.links_reunitarize_device_grid(a), "momentum_update (momenta)": lambda a: ctx.momentum_update_device_grid(a, dF, 0.1),
             "momentum_update (force)": lambda a: ctx.momentum_update_device_grid(dP, a, 0.1), "momentum_kinetic": lambda a: ctx.momentum_kinetic_device_grid(a)}
    for name, call in calls.items():
        refused(lambda: call(int(host.ctypes.data)), "not a pointer into device memory")
        refused(lambda: call(small + 64), "smaller than the array")
        refused(lambda: call(0), "null")
    refused(lambda: ctx.gauge_force_device_grid(dU, dU, BETA, 0.0), "overlap")
    big = hip.alloc(2 * nbytes(L))
    refused(lambda: ctx.links_update_device_grid(big, big + 8, 0.1), "overlap")
    refused(lambda: ctx.momentum_update_device_grid(big + nbytes(L) - 8, big, 0.1), "overlap")
    refused(lambda: ctx.gauge_force_device_grid(dF, dU, float("nan"), 0.0), "beta", "not finite")
    refused(lambda: ctx.gauge_force_device_grid(dF, dU, BETA, float("inf")), "c1", "not finite")
    refused(lambda: ctx.links_update_device_grid(dU, dP, float("inf")), "eps", "not finite")
    # the plain forms keep refusing a grid, and name the twin
    for name, call in (("gauge_loops", lambda: ctx.gauge_loops_device(dU)), ("gauge_force", lambda: ctx.gauge_force_device(dF, dU, BETA, 0.0)),
                       ("links_update", lambda: ctx.links_update_device(dU, dP, 0.1)), ("links_reunitarize", lambda: ctx.links_reunitarize_device(dU)),
                       ("momentum_update", lambda: ctx.momentum_update_device(dP, dF, 0.1)), ("momentum_kinetic", lambda: ctx.momentum_kinetic_device(dP))):
        refused(call, "process grid", "not built yet", f"ddamg_hip_{name}_device_grid")
    # nothing was sent and nothing was written, and the context still serves
    assert ctx.comm_stats()["device_sendrecv"]["messages"] == 0
    assert np.array_equal(hip.download(dU, U.shape), U) and (hip.download(dP, shape(L)) == 1.0).all() and not host.any()
    ctx.gauge_force_device_grid(dF, dU, BETA, gr.SYMANZIK)
    assert different_bits(hip.download(dF, shape(L)), good) == 0
    ctx.close()
    # a grid without a transport: the collective ones are refused, the two that send nothing run
    bare = dd.Context(params(list(L), [2] * 4, M0, CSW, grid=ALL))
    for call in (lambda: bare.gauge_loops_device_grid(dU), lambda: bare.gauge_force_device_grid(dF, dU, BETA, gr.SYMANZIK),
                 lambda: bare.momentum_kinetic_device_grid(dP), lambda: bare.links_reunitarize_device_grid(dU)):
        refused(call, "install a transport first")
    assert np.array_equal(hip.download(dU, U.shape), U)
    bare.momentum_update_device_grid(dP, dF, 0.5)
    assert np.array_equal(hip.download(dP, shape(L)), 1.0 + 0.5 * good)
    bare.close()


# several processes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nproc,grid", [(2, "2,1,1,1"), (2, "1,1,1,2"), (4, "2,2,1,1")])
def test_gauge_sector_on_a_process_grid(nproc, grid):
    """every rank computes its part of the gauge force of the golden 8^4 links over the host transport against its part of the
    reference of the whole lattice, and the global sums, the kinetic energy and the largest deviation, which must be the same on every
    rank; 2,2,1,1: corners from a diagonal process.  1,1,1,2 also runs the refusal of a shell deeper than the local lattice, which
    every rank must return"""
    from launcher import torchrun
    r = torchrun(nproc, os.path.join(HERE, "dist_gauge_md_worker.py"), "--grid", grid, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "DIST_GAUGE_MD_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout[-2500:])
