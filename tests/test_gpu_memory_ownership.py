"""GPU tests (-m gpu) of who owns device and pinned host memory: every buffer of the library is a DeviceBuffer / PinnedBuffer
(csrc/device_buffer.h) that gives its memory back in its destructor, on the error paths too.  The library counts the bytes its
live buffers hold (ddamg_hip_memory_in_use); every case reads the counters first and asserts on the DIFFERENCE, exactly: contexts
of other test modules and the static diagnostic buffer may be alive.  The leaks these cases guard against do not depend on the
volume, so the lattices are the smallest each configuration accepts."""
import numpy as np
import pytest
from conftest import random_su3
from ddalphaamg_amd import api
import ddalphaamg_amd as dd

pytestmark = pytest.mark.gpu


def two_level(L=8, **kw):
    """L^4 with 4^4 Schwarz blocks = aggregates; fp32 V-cycle with the paired Schwarz kernel unless kw says otherwise"""
    p = api.default_params(); p.num_levels = 2
    for mu in range(4):
        p.local_lattice[0][mu] = L; p.block_lattice[0][mu] = 4; p.local_lattice[1][mu] = L // 4
    p.num_vect[0] = 8; p.setup_iter[0] = 1
    p.restart, p.max_restart, p.tol = 20, 10, 1e-8
    p.coarse_iter, p.coarse_restart, p.coarse_tol = 50, 5, 5e-2
    p.mixed_precision, p.method, p.odd_even = 2, 2, 1
    p.m0, p.csw = 0.3, 1.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def gauge(p, seed=7):
    V = int(np.prod([p.local_lattice[0][mu] for mu in range(4)]))
    return V, random_su3(V * 4, seed).reshape(V, 4, 9, 2)


def rhs(V):
    b = np.zeros((V, 12, 2)); b[..., 0] = 1.0
    return b


def lifetime(p, scale=False):
    """create, set gauge, set up with one iteration, one solve, one vector per level, close"""
    ctx = dd.Context(p)
    V, U = gauge(p)
    ctx.set_gauge(U, anti_pbc=True)
    if p.num_levels > 1:
        ctx.setup(1)
    if scale:
        ctx.scale_clover(1.0, 1.1)
    ctx.solve(rhs(V), 1e-6)
    for lvl in range(p.num_levels):
        ctx.vector(lvl, 32).free()
    assert api.memory_in_use()[0] > 0
    ctx.close()


CONFIGS = {
    "paired-schwarz-mp2": dict(),
    "mp0": dict(mixed_precision=0),
    "mp1": dict(mixed_precision=1),
    "additive": dict(method=1),
    "gmres-smoother": dict(method=4),
    "bicgstab-no-hierarchy": dict(method=5, mixed_precision=1, num_levels=1),
    "no-odd-even": dict(odd_even=0),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_everything_comes_back(name):
    start = api.memory_in_use()
    lifetime(two_level(**CONFIGS[name]))
    assert api.memory_in_use() == start


def test_everything_comes_back_with_a_scaled_clover_term():
    start = api.memory_in_use()
    lifetime(two_level(), scale=True)
    assert api.memory_in_use() == start


def test_everything_comes_back_three_levels_many_vectors():
    """the configuration of test_gpu_three_levels.py, with one kcycle_many and one coarse_solve_many call: the many-vector
    workspaces of the intermediate and of the coarsest level allocate"""
    from test_gpu_three_levels import make_ctx
    start = api.memory_in_use()
    g, ctx = make_ctx("ref_8x8_3lvl_small.npz")
    ctx.setup(1)
    V = ctx.volume(0)
    ctx.solve(rhs(V), 1e-6)
    for lvl in (1, 2):
        xs = [ctx.vector(lvl, 32) for _ in range(4)]; bs = [ctx.vector(lvl, 32) for _ in range(4)]
        rng = np.random.default_rng(lvl)
        for b in bs:
            b.upload(rng.standard_normal((ctx.volume(lvl), b.ndof, 2)))
        if lvl == 1:
            ctx.kcycle_many(xs, bs)
        else:
            ctx.coarse_solve_many(xs, bs)
        for v in xs + bs:
            v.free()
    ctx.vector(0, 32).free()
    ctx.close()
    assert api.memory_in_use() == start


def test_a_refused_setup_gives_everything_back():
    """12^4 with 4^4 aggregates: three blocks per direction.  ddamg_hip_create accepts it; the Multigrid constructor allocates the
    level buffers and is then refused by the parity check of the multiplicative Schwarz method -- an argument check on the host"""
    start = api.memory_in_use()
    p = two_level(L=12)
    ctx = dd.Context(p)
    V, U = gauge(p)
    ctx.set_gauge(U, anti_pbc=True)
    before = api.memory_in_use()
    for _ in range(3):
        with pytest.raises(api.DDAMGError, match="multiplicative SAP needs an even number of blocks per direction"):
            ctx.setup(1)
        assert api.memory_in_use() == before
    ctx.close()
    assert api.memory_in_use() == start


def test_a_refused_setup_with_the_gmres_smoother_gives_everything_back():
    """the same lattice with method 4: no Schwarz smoother; the coarsest 3^4 lattice fails the even-extent check of the odd-even
    solve after both levels have allocated their buffers, Krylov slabs and reduction workspaces"""
    start = api.memory_in_use()
    p = two_level(L=12, method=4)
    ctx = dd.Context(p)
    V, U = gauge(p)
    ctx.set_gauge(U, anti_pbc=True)
    before = api.memory_in_use()
    for _ in range(3):
        with pytest.raises(api.DDAMGError, match="the coarsest lattice must have even global extents"):
            ctx.setup(1)
        assert api.memory_in_use() == before
    ctx.close()
    assert api.memory_in_use() == start


def test_a_refused_create_gives_everything_back():
    """a coarse lattice that does not divide the fine one: refused after the stream, the events and nothing else exist"""
    start = api.memory_in_use()
    p = two_level()
    p.local_lattice[1][3] = 3
    with pytest.raises(api.DDAMGError, match="coarse lattice must divide the finer lattice"):
        dd.Context(p)
    assert api.memory_in_use() == start
    dd.Context(two_level()).close()
    assert api.memory_in_use() == start


def test_reallocation_paths():
    """setup, solve, the calls that release the setup workspace (a new operator, a clover scaling there and back), setup and solve
    again in one context: the second solve repeats the first, and everything returns on close.  The test vectors of a setup come
    from libc rand() (test_vector_rng = 0), which the library seeds once per context: seeding it here before either setup gives
    both the same random vectors, so that the two solves can be compared exactly"""
    import ctypes
    libc = ctypes.CDLL(None)
    start = api.memory_in_use()
    p = two_level()
    ctx = dd.Context(p)
    V, U = gauge(p)
    ctx.set_gauge(U, anti_pbc=True)
    results = []
    for _ in range(2):
        libc.srand(2718)
        ctx.setup(1)
        _, it, _, rr = ctx.solve(rhs(V), 1e-6)
        results.append((it, rr))
        print("setup + solve:", it, "iterations, relative residual", repr(rr))
        ctx.scale_clover(1.0, 1.1); ctx.scale_clover(1.0, 1.0)
        ctx.set_gauge(U, anti_pbc=True)
    assert results[1] == results[0]
    ctx.close()
    assert api.memory_in_use() == start
